// Host logic of the C ABI that needs no GPU (used by slf_api.hip; exercised on the CPU by tests/abi_bind_main.cpp):
// a module descriptor into the module's configuration, the table of kernels the library serves with their argument
// lists, the index arithmetic of the reference's face kernels, and (part (f)) what a launch and the x-face setters check.  Calls no HIP function, allocates nothing, and reads
// no global state beyond the environment knobs SLF_BC_LEVEL, SLF_VARIANT and SLF_BLOCK_X.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/sailfish_hip.h"
#include "slf_kernels.h"
#include "slf_node.h"
#include "slf_variant.h"

#ifndef SLF_DEFAULT_VARIANT
#define SLF_DEFAULT_VARIANT 11
#endif

namespace slf {

enum KernelKind {
  KK_COLLIDE_AND_PROPAGATE,
  KK_SET_INITIAL_CONDITIONS,
  KK_PBC,
  KK_PBC_SWAP,
  KK_MACRO_PBC,
  KK_COLLECT_SPARSE,
  KK_DISTRIBUTE_SPARSE,
  KK_COLLECT_BOX,
  KK_DISTRIBUTE_BOX,
  KK_COLLECT_FACE_SWAP,       // reference argument lists (kernel_utils.mako): ...ContinuousDataWithSwap
  KK_DISTRIBUTE_FACE_SWAP,
  KK_COLLECT_MACRO_FACE,      // ...ContinuousMacroData
  KK_DISTRIBUTE_MACRO_FACE,
  KK_COMPUTE_MACRO,
  KK_SC_MACRO,
  KK_SC_SWEEP0,
  KK_SC_SWEEP1,
  KK_SC_FUSED,
  KK_SC_INIT,
  KK_SCS_MACRO,
  KK_SCS_SWEEP,
  KK_FE_MACRO,                // free-energy binary fluid (slf_fe.hip)
  KK_FE_FLUID,
  KK_FE_ORDER,
  KK_FE_INIT,
  KK_SC3_MACRO,               // ternary Shan-Chen mixture (slf_sc3.hip)
  KK_SC3_SWEEP0,              // ... the sweeps of lattices 0, 1, 2 in this order
  KK_SC3_SWEEP1,
  KK_SC3_SWEEP2,
  KK_SC3_FUSED,
  KK_SC3_INIT,
  KK_RESIDENT,              // several steps inside one launch (slf_resident.hip)
};

// a refusal: the message for slf_last_error() and the code to return
inline int refuse(const char** err, int code, const char* msg) {
  *err = msg;
  return code;
}
inline int refuse(std::string* err, int code, const std::string& msg) {
  *err = msg;
  return code;
}

// ---- (a) module configuration ------------------------------------------------------------------------------------
// What slf_module_create() derives from the descriptor; the module adds its device allocations.
struct ModuleConfig {
  KernelSelector sel;
  Geometry geo;
  Physics phys;
  ShanChen sc;
  FreeEnergy fe;
  ShanChen3 sc3;
  int access_pattern;
  int block_x;
  int n_node_params;
};

inline bool is_lat_lattice(int lattice) { return lattice == SLF_D3Q15 || lattice == SLF_D3Q27; }

// ---- what each feature is served with ------------------------------------------------------------------------------
// A column is one field of the descriptor, with its values as the user knows them (`names`; NULL: not worth listing).
enum Column { COL_LATTICE, COL_SIMTYPE, COL_MODEL, COL_ENTROPIC, COL_REGULARIZED, COL_SUBGRID, COL_DENSITY, COL_ADDRESSING,
              COL_FORCE, COL_ACCEL_FIELD, COL_EDM, COL_KINDS, N_COLUMNS };
inline constexpr struct { int32_t slf_module_desc::*field; const char* field_name; int n; const char* names[17]; } COLUMNS[N_COLUMNS] = {
  {&slf_module_desc::lattice, "lattice", 4, {"D2Q9", "D3Q19", "D3Q15", "D3Q27"}},
  {&slf_module_desc::simtype, "simtype", 5, {"single-fluid modules", "the Shan-Chen models", "the Shan-Chen models", "the free-energy model",
                                             "the ternary Shan-Chen model"}},
  {&slf_module_desc::model, "model", 3, {"--model=bgk", "--model=mrt", "--model=elbm"}},
  {&slf_module_desc::entropic_equilibrium, "entropic_equilibrium", 2, {nullptr, "entropic_equilibrium"}},
  {&slf_module_desc::regularized, "regularized", 2, {nullptr, "--regularized"}},
  {&slf_module_desc::subgrid, "subgrid", 2, {nullptr, "--subgrid"}},
  {&slf_module_desc::incompressible, "incompressible", 3, {"the compressible density model", "--incompressible", "--minimize_roundoff"}},
  {&slf_module_desc::node_addressing, "node_addressing", 2, {"--node_addressing=direct", "--node_addressing=indirect"}},
  {&slf_module_desc::has_force, "has_force", 2, {nullptr, "body forces"}},
  {&slf_module_desc::accel_field, "accel_field", 2, {nullptr, "accel_field"}},
  {&slf_module_desc::force_implementation, "force_implementation", 2, {nullptr, "force_implementation = EDM"}},
  {nullptr, "type_kind", 17,      // one value per node type
   {"fluid", nullptr, nullptr, nullptr, "NTFullBBWall", "NTHalfBBWall", "NTRegularizedVelocity", "NTEquilibriumDensity", "NTEquilibriumVelocity",
    "NTZouHeVelocity", "NTZouHeDensity", "NTRegularizedDensity", "NTCopy", "NTYuOutflow", "NTDoNothing", "NTSlip", "NTWallTMS"}},
};

// A row is a feature that restricts what a module combines it with: per column, the mask of the field's values it is served
// with (bit v: the value v; a yes / no field is served switched OFF only, or with ANY value).  `has`: the descriptor has the
// feature.  `per_node_only`: the tuned, whole-row and slot kernels do not implement it (module_config clears
// Geometry::variant).  `notes`: a reason worth telling, by column.  A new feature is one row here and one in sailfish_amd/serves.py.
constexpr uint32_t bit(int v) { return 1u << ((v >= 0 && v < 31) ? v : 31); }      // (bit 31: every other value)
constexpr uint32_t ANY = ~0u, OFF = bit(0), NO_EDM = ~bit(SLF_FORCE_EDM), NO_ELBM = ~bit(SLF_ELBM), NO_ROUNDOFF = ~bit(SLF_DENSITY_ROUNDOFF);
constexpr uint32_t LBM = bit(SLF_SIM_LBM), BGK = bit(SLF_BGK), DIRECT = bit(SLF_ADDR_DIRECT), COMPRESSIBLE = bit(SLF_DENSITY_COMPRESSIBLE),
                   INCOMPRESSIBLE = bit(SLF_DENSITY_INCOMPRESSIBLE);
constexpr uint32_t KINDS_PLAIN = bit(SLF_NK_FLUID) | bit(SLF_NK_GHOST) | bit(SLF_NK_UNUSED) | bit(SLF_NK_PROPAGATION_ONLY) | bit(SLF_NK_FULL_BB),
                   HALF_BB = bit(SLF_NK_HALF_BB), SLIP = bit(SLF_NK_SLIP), TMS = bit(SLF_NK_WALL_TMS),
                   EQUILIBRIUM = bit(SLF_NK_EQUILIBRIUM_DENSITY) | bit(SLF_NK_EQUILIBRIUM_VELOCITY);
struct Serves {
  const char* name;
  bool (*has)(const slf_module_desc*);
  bool per_node_only;
  uint32_t serves[N_COLUMNS];
  struct { int column; const char* text; } notes[2];
};
#define SLF_HAS(expr) [](const slf_module_desc* d) -> bool { return expr; }
#define SLF_LAT_ROW(name, id) /* the BGK sweep of slf_lat.hip and nothing else */ \
  {name, SLF_HAS(d->lattice == id), true, {ANY, LBM, BGK, OFF, OFF, OFF, NO_ROUNDOFF, DIRECT, ANY, ANY, ANY, KINDS_PLAIN | HALF_BB}, {}}
enum Row { ROW_SHALLOW_WATER, ROW_ACCEL_FIELD, ROW_D3Q15, ROW_D3Q27, ROW_REGULARIZED_SUBGRID, ROW_TMS, ROW_ELBM, ROW_ROUNDOFF, ROW_SHAN_CHEN,
           ROW_FREE_ENERGY, ROW_TERNARY, N_ROWS };
inline const Serves SERVES[N_ROWS] = {
  // masks: lattice, simtype, model, entropic, regularized, subgrid, density, addressing, force, accel_field, edm, kinds
  {"shallow water", SLF_HAS(d->equilibrium == SLF_EQ_SHALLOW_WATER), true,      // the SW instantiations of the per-node sweep
   {bit(SLF_D2Q9), LBM, BGK, OFF, OFF, OFF, COMPRESSIBLE, DIRECT, ANY, ANY, ANY, KINDS_PLAIN | HALF_BB | SLIP},
   {{COL_DENSITY, "the density is the water depth"},
    {COL_KINDS, "the node types that carry a density or a velocity assume the pressure rho / 3"}}},
  {"accel_field", SLF_HAS(d->accel_field == 1), true,                           // the ACCF instantiations of the per-node sweep
   {bit(SLF_D2Q9) | bit(SLF_D3Q19), LBM, NO_ELBM, ANY, OFF, OFF, NO_ROUNDOFF, DIRECT, ANY, ANY, ANY, ~TMS},
   {{COL_LATTICE, "the sweep of D3Q15 / D3Q27 takes a constant acceleration"}, {COL_MODEL, "the entropic collision takes no body force"}}},
  SLF_LAT_ROW("D3Q15", SLF_D3Q15),
  SLF_LAT_ROW("D3Q27", SLF_D3Q27),
  // the options of the BGK relaxation preamble (relaxation_common.mako:166-237): the reference's MRT relaxation does not call it
  // (its kernels would silently ignore both flags), and its expressions were never written for the rest
  {"regularized / subgrid", SLF_HAS(d->regularized || d->subgrid), true,
   {ANY, LBM, BGK, ANY, ANY, ANY, NO_ROUNDOFF, ANY, ANY, ANY, NO_EDM, ANY}, {}},
  // the per-node kernels and the slot sweep carry the walls' code; module_config does not walk this row: the other models' own
  // rows refuse the type among their node kinds, where the ladders did
  {"NTWallTMS", [](const slf_module_desc* d) -> bool {
     for (int i = 0; i < d->n_types && i < SLF_MAX_NODE_TYPES; i++)
       if (d->type_kind[i] == SLF_NK_WALL_TMS) return true;
     return false;
   }, true, {ANY, LBM, ANY, ANY, ANY, ANY, ANY, ANY, ANY, ANY, ANY, ANY}, {}},
  // what ELBM_relaxate (relaxation.mako:56-97) was written for, and what this library has fixtures for
  {"elbm", SLF_HAS(d->model == SLF_ELBM), true, {ANY, LBM, ANY, ANY, OFF, OFF, NO_ROUNDOFF, ANY, OFF, ANY, ANY, ANY},
   {{COL_DENSITY, "it stores f_i - w_i, the entropy needs the populations themselves"}}},
  // "BGK-like models" in the reference (lb_base.py:72-76), whose regularized and Zou-He expressions are inconsistent under the option
  {"minimize_roundoff", SLF_HAS(d->incompressible == SLF_DENSITY_ROUNDOFF), true,
   {ANY, LBM, BGK, ANY, ANY, ANY, ANY, ANY, ANY, ANY, ANY, KINDS_PLAIN | HALF_BB | TMS | EQUILIBRIUM}, {}},
  {"Shan-Chen", SLF_HAS(d->simtype == SLF_SIM_SHAN_CHEN_BINARY || d->simtype == SLF_SIM_SHAN_CHEN_SINGLE), false,
   {ANY, ANY, BGK, ANY, ANY, ANY, ANY, ANY, ANY, ANY, ANY, KINDS_PLAIN}, {}},
  {"free energy", SLF_HAS(d->simtype == SLF_SIM_FREE_ENERGY), false,          // slf_fe.hip, of the reference's lb_binary.py:139-372
   {ANY, ANY, BGK, ANY, ANY, ANY, COMPRESSIBLE, DIRECT, OFF, ANY, ANY, KINDS_PLAIN},
   {{COL_MODEL, "the FE-MRT collision, relaxation.mako:15-54"}, {COL_FORCE, "free_energy_external_force, use_force_for_equilibrium"}}},
  {"ternary Shan-Chen", SLF_HAS(d->simtype == SLF_SIM_SHAN_CHEN_TERNARY), false,      // slf_sc3.hip, of the reference's lb_ternary.py
   {ANY, ANY, BGK, ANY, ANY, ANY, COMPRESSIBLE, DIRECT, ANY, ANY, ANY, KINDS_PLAIN}, {}},
};
#undef SLF_LAT_ROW
#undef SLF_HAS

// The first conflict of the descriptor with those of the rows first .. last that apply to it, rows and columns in table order:
// "<feature>: <offender> is not served (<note>); <what the row serves> only".  NULL: served.  The message lives in a buffer of
// the calling thread until its next call.  module_config walks each row where the descriptor is well-formed enough for it.
inline const char* serves_conflict(const slf_module_desc* d, int first, int last) {
  thread_local char msg[512];
  for (int r = first; r <= last; r++) {
    const Serves& row = SERVES[r];
    for (int col = 0; row.has(d) && col < N_COLUMNS; col++) {
      const auto& c = COLUMNS[col];
      const uint32_t serves = row.serves[col];
      for (int i = 0; i < (c.field ? 1 : d->n_types) && i < SLF_MAX_NODE_TYPES; i++) {
        const int v = c.field ? d->*c.field : d->type_kind[i];
        if (serves & bit(v)) continue;
        size_t len = 0;
        auto say = [&len](const char* a, const char* b, const char* end) {
          if (len < sizeof msg) len += snprintf(msg + len, sizeof msg - len, "%s%s%s", a, b, end);
        };
        const char* offender = v >= 0 && v < c.n ? c.names[v] : nullptr;
        char value[32];
        snprintf(value, sizeof value, " = %d", v);
        say(row.name, ": ", offender ? offender : c.field_name);
        say(offender ? "" : value, offender && offender[strlen(offender) - 1] == 's' ? " are" : " is", " not served");
        for (const auto& note : row.notes)      // (a value without a name is malformed: the reason is not about it)
          if (note.text && note.column == col && offender) say(" (", note.text, ")");
        const char* listed[17];
        int n = 0;
        for (int s = 0; s < c.n; s++)
          if ((serves & bit(s)) && c.names[s]) listed[n++] = c.names[s];
        if (n > 6) n = 0;      // (a longer list says little more than the offender did)
        for (int k = 0; k < n; k++) say(k == 0 ? "; " : (k == n - 1 ? " and " : ", "), listed[k], "");
        if (n) say(c.field ? " only" : " nodes only", "", "");
        return msg;
      }
    }
  }
  return nullptr;
}

// Single-fluid D2Q9 / D3Q19 modules can always end up in the per-node sweep (launch_sweep, slf_kernels.hip: whatever the tuned
// and whole-row kernels decline).  NULL: every variant of it the module's steps select exists (slf_variant.h); otherwise the
// rule the missing one breaks -- a combination that the refusals above let through and no instantiation serves.
inline const char* per_node_variants_exist(const ModuleConfig& c) {
  for (Prop prop : {PROP_AB, PROP_AA_EVEN, PROP_AA_ODD}) {
    if ((prop == PROP_AB) != (c.access_pattern == SLF_AB)) continue;
    if (const char* why = per_node_variant_conflict(c.sel.lattice, per_node_variant_of(c.sel, c.geo, c.phys, prop))) return why;
  }
  return nullptr;
}

inline int module_config(const slf_module_desc* d, ModuleConfig* c, const char** err) {
  *c = ModuleConfig{};
  if (d->struct_size != sizeof(slf_module_desc)) return refuse(err, SLF_ERR_INVALID, "slf_module_desc size mismatch (ABI)");
  if (d->lattice != SLF_D2Q9 && d->lattice != SLF_D3Q19 && d->lattice != SLF_D3Q15 && d->lattice != SLF_D3Q27)
    return refuse(err, SLF_ERR_UNSUPPORTED, "unsupported lattice");
  if (d->equilibrium != SLF_EQ_BGK && d->equilibrium != SLF_EQ_SHALLOW_WATER)
    return refuse(err, SLF_ERR_INVALID, "equilibrium must be SLF_EQ_BGK or SLF_EQ_SHALLOW_WATER");
  if (d->equilibrium == SLF_EQ_SHALLOW_WATER && !(d->gravity > 0.0)) return refuse(err, SLF_ERR_INVALID, "shallow water: gravity must be > 0");
  // which options each feature is served with: the table SERVES, each row walked where its ladder stood
  if (const char* why = serves_conflict(d, ROW_SHALLOW_WATER, ROW_SHALLOW_WATER)) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  if (d->accel_field != 0 && d->accel_field != 1) return refuse(err, SLF_ERR_INVALID, "accel_field must be 0 or 1");
  if (const char* why = serves_conflict(d, ROW_ACCEL_FIELD, ROW_D3Q27)) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  if (d->model != SLF_BGK && d->model != SLF_MRT && d->model != SLF_ELBM)
    return refuse(err, SLF_ERR_UNSUPPORTED, "unsupported collision model");
  if (d->precision != 4 && d->precision != 8) return refuse(err, SLF_ERR_UNSUPPORTED, "precision must be 4 or 8");
  if (d->access_pattern != SLF_AB && d->access_pattern != SLF_AA)
    return refuse(err, SLF_ERR_UNSUPPORTED, "unsupported access pattern");
  const int dim = d->lattice == SLF_D2Q9 ? 2 : 3;
  if (d->envelope != 1) return refuse(err, SLF_ERR_UNSUPPORTED, "envelope size must be 1");
  if (d->lat_nx < 3 || d->lat_ny < 3 || (dim == 3 && d->lat_nz < 3) || (dim == 2 && d->lat_nz != 1))
    return refuse(err, SLF_ERR_INVALID, "bad lattice size");
  if (d->arr_nx < d->lat_nx || d->arr_ny < d->lat_ny || d->arr_nz < d->lat_nz)
    return refuse(err, SLF_ERR_INVALID, "padded size smaller than lattice size");
  if (d->tau <= 0.5 && d->relaxation_enabled) return refuse(err, SLF_ERR_INVALID, "tau must be > 0.5");
  if (d->n_types < 0 || d->n_types > SLF_MAX_NODE_TYPES) return refuse(err, SLF_ERR_INVALID, "too many node types");
  const unsigned long long total = (unsigned long long)d->arr_nx * d->arr_ny * d->arr_nz;
  if (total >= 0xFFFFFFFFull || d->dist_stride >= 0xFFFFFFFFull)
    return refuse(err, SLF_ERR_UNSUPPORTED, "subdomain too large for 32-bit node indices");

  c->sel.lattice = d->lattice;
  c->sel.model = d->model;
  c->sel.precision = d->precision;
  c->sel.general = !d->fluid_only;
  if (d->node_addressing != SLF_ADDR_DIRECT && d->node_addressing != SLF_ADDR_INDIRECT)
    return refuse(err, SLF_ERR_INVALID, "node_addressing must be SLF_ADDR_DIRECT or SLF_ADDR_INDIRECT");
  if (d->node_addressing == SLF_ADDR_INDIRECT) {
    if (d->fluid_only) return refuse(err, SLF_ERR_INVALID, "indirect addressing needs the node map (fluid_only = 0)");
    if (d->simtype != SLF_SIM_LBM && d->simtype != SLF_SIM_SHAN_CHEN_BINARY && d->simtype != SLF_SIM_SHAN_CHEN_SINGLE &&
        d->simtype != SLF_SIM_FREE_ENERGY && d->simtype != SLF_SIM_SHAN_CHEN_TERNARY) {      // (free energy, ternary: refused below, by their rows)
      return refuse(err, SLF_ERR_UNSUPPORTED, "indirect addressing: unknown simtype");
    }
  }
  c->access_pattern = d->access_pattern;
  slf::Geometry& g = c->geo;
  g.dim = dim;
  g.lat_nx = d->lat_nx; g.lat_ny = d->lat_ny; g.lat_nz = d->lat_nz;
  g.arr_nx = d->arr_nx; g.arr_ny = d->arr_ny; g.arr_nz = d->arr_nz;
  g.arr_nxy = d->arr_nx * d->arr_ny;
  g.dist_size = (uint32_t)(d->dist_stride ? d->dist_stride : total);
  if (d->node_addressing == SLF_ADDR_INDIRECT) {
    // the stride is the number of active-node slots: the caller's business (it owns the address table)
    if (d->dist_stride == 0) return refuse(err, SLF_ERR_INVALID, "indirect addressing: dist_stride (number of slots) must be given");
  } else if (g.dist_size < total) {
    return refuse(err, SLF_ERR_INVALID, "dist_stride smaller than the subdomain");
  }
  for (int i = 0; i < 3; i++) {
    g.wrap[i] = (i < dim) ? (d->periodic_fused[i] != 0) : 0;
    g.axis_mode[i] = g.wrap[i] ? 2 : ((i < dim && d->periodic_local[i]) ? 1 : 0);
  }
  g.type_mask = d->nt_type_mask;
  g.param_shift = d->nt_misc_shift;
  g.param_mask = (1u << d->nt_param_shift) - 1u;
  g.orient_shift = d->nt_misc_shift + d->nt_param_shift + d->nt_scratch_shift;
  g.type_lut = 0;
  c->phys.tms_mask = 0;
  for (int i = 0; i < d->n_types; i++) {
    int k = d->type_kind[i];
    if (k < 0 || k >= slf::NK_COUNT) return refuse(err, SLF_ERR_UNSUPPORTED, "node type kind not supported by the HIP backend");
    if (k == SLF_NK_WALL_TMS) {      // inside the kernels: a half-way bounce-back type with a flag (slf_kernels.h)
      c->phys.tms_mask |= 1u << i;
      k = slf::NK_HALF_BB;
    }
    g.type_lut |= (unsigned long long)k << (4 * i);
  }
  for (int i = 0; i < d->n_types; i++) {
    const int k = d->type_kind[i];
    if ((k == SLF_NK_COPY || k == SLF_NK_YU_OUTFLOW) && d->access_pattern != SLF_AB)
      return refuse(err, SLF_ERR_UNSUPPORTED, "NTCopy / NTYuOutflow nodes read neighbouring nodes of the input lattice: "
                                       "two-copy (AB) access pattern only, as in the reference (boundary.mako:626-628)");
  }
  for (int i = 0; i < d->n_types; i++) {
    if (d->type_kind[i] == SLF_NK_DO_NOTHING && d->access_pattern != SLF_AB && d->node_addressing == SLF_ADDR_INDIRECT)
      return refuse(err, SLF_ERR_UNSUPPORTED, "NTDoNothing nodes of the in-place (AA) pattern keep their unknown populations in the ghost "
                                       "nodes behind them, which own no slot under indirect addressing (the reference indexes "
                                       "nodes[] unguarded there, boundary.mako:862-876 with propagation.mako:93-99)");
  }
  g.bc_level = 0;
  for (int i = 0; i < d->n_types; i++) {
    const int k = d->type_kind[i];
    const bool plain = (KINDS_PLAIN & bit(k)) != 0;
    const int level = (k == SLF_NK_COPY || k == SLF_NK_YU_OUTFLOW || k == SLF_NK_DO_NOTHING || k == SLF_NK_SLIP) ? 2 : (plain ? 0 : 1);
    if (level > g.bc_level) g.bc_level = level;
  }
  if (const char* ev = getenv("SLF_BC_LEVEL")) {      // tests: force the full instantiation
    if (atoi(ev) > g.bc_level) g.bc_level = atoi(ev);
  }
  g.x_ghost_unused = 0;
  g.use_link_tags = d->use_link_tags;
  g.indirect = d->node_addressing == SLF_ADDR_INDIRECT;
  g.variant = SLF_DEFAULT_VARIANT;
  if (d->sparse_geometry) g.variant |= 64;
  if (const char* ev = getenv("SLF_VARIANT")) g.variant = atoi(ev);
  for (const Serves& row : SERVES)
    if (row.per_node_only && row.has(d)) g.variant = 0;      // the tuned, whole-row and slot kernels implement the plain module (wins over the knob)
  slf::Physics& ph = c->phys;
  ph.tau = d->tau;
  ph.visc = d->visc;
  for (int i = 0; i < 3; i++) ph.accel[i] = d->accel[i];
  for (int i = 0; i < 27; i++) ph.mrt_rates[i] = d->mrt_rates[i];
  ph.incompressible = d->incompressible;
  ph.accel_field = d->accel_field;
  ph.equilibrium = d->equilibrium;
  ph.gravity = d->equilibrium == SLF_EQ_SHALLOW_WATER ? d->gravity : 0.0;
  ph.has_force = d->has_force || d->accel_field;      // a field is a body force
  ph.relaxation_enabled = d->relaxation_enabled;
  ph.force_edm = d->force_implementation == SLF_FORCE_EDM;
  if (ph.force_edm && d->model != SLF_BGK)
    return refuse(err, SLF_ERR_UNSUPPORTED, "the exact difference method (force_implementation = EDM) needs the BGK collision");
  ph.regularized = d->regularized != 0;
  ph.subgrid = d->subgrid;
  ph.smagorinsky_const = d->smagorinsky_const;
  if (d->subgrid != SLF_SUBGRID_NONE && d->subgrid != SLF_SUBGRID_LES_SMAGORINSKY)
    return refuse(err, SLF_ERR_INVALID, "subgrid must be one of SLF_SUBGRID_*");
  if (const char* why = serves_conflict(d, ROW_REGULARIZED_SUBGRID, ROW_REGULARIZED_SUBGRID)) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  if (ph.subgrid && !(d->smagorinsky_const > 0.0))
    return refuse(err, SLF_ERR_INVALID, "subgrid = les-smagorinsky needs smagorinsky_const > 0");
  if (ph.tms_mask && d->fluid_only)
    return refuse(err, SLF_ERR_UNSUPPORTED, "NTWallTMS nodes are node types: the module must read the node map (fluid_only = 0)");
  ph.entropic_equilibrium = d->entropic_equilibrium != 0;
  ph.entropy_tolerance = d->entropy_tolerance;
  ph.alpha_tolerance = d->alpha_tolerance;
  if (ph.entropic_equilibrium && d->model != SLF_ELBM)
    return refuse(err, SLF_ERR_INVALID, "entropic_equilibrium needs model = SLF_ELBM");
  if (d->model == SLF_ELBM) {
    bool rates = false;            // a host that filled in MRT relaxation rates expects them to act
    for (int i = 0; i < 27; i++) rates = rates || d->mrt_rates[i] != 0.0;
    if (rates)
      return refuse(err, SLF_ERR_UNSUPPORTED, "elbm: MRT relaxation rates are set (mrt_rates must be all zero: the entropic collision has one rate)");
    if (const char* why = serves_conflict(d, ROW_ELBM, ROW_ELBM)) return refuse(err, SLF_ERR_UNSUPPORTED, why);
    if (d->incompressible == SLF_DENSITY_INCOMPRESSIBLE && ph.entropic_equilibrium)
      return refuse(err, SLF_ERR_UNSUPPORTED, "elbm: the product-form equilibrium (entropic_equilibrium) is compressible; not with the "
                                              "incompressible density model");
    if (!(d->entropy_tolerance > 0.0) || !(d->alpha_tolerance >= 0.0))
      return refuse(err, SLF_ERR_UNSUPPORTED, "elbm: entropy_tolerance must be > 0 and alpha_tolerance >= 0");
  }
  if (const char* why = serves_conflict(d, ROW_ROUNDOFF, ROW_ROUNDOFF)) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  if (d->incompressible < SLF_DENSITY_COMPRESSIBLE || d->incompressible > SLF_DENSITY_ROUNDOFF)
    return refuse(err, SLF_ERR_INVALID, "incompressible must be one of SLF_DENSITY_*");
  c->sc.enabled = (d->simtype == SLF_SIM_SHAN_CHEN_BINARY) ? 1 : ((d->simtype == SLF_SIM_SHAN_CHEN_SINGLE) ? 2 : 0);
  c->sc.tau_phi = d->tau_phi;
  for (int i = 0; i < 4; i++) c->sc.G[i] = d->sc_G[i];
  c->sc.potential = d->sc_potential;
  for (int i = 0; i < 3; i++) c->sc.accel1[i] = d->accel1[i];
  if (const char* why = serves_conflict(d, ROW_SHAN_CHEN, ROW_TERNARY)) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  if (c->sc.enabled == 1 && d->tau_phi <= 0.5) return refuse(err, SLF_ERR_INVALID, "tau_phi must be > 0.5");
  if (c->sc.enabled == 2) c->sc.tau_phi = d->tau;
  c->fe = slf::FreeEnergy{};
  if (d->simtype == SLF_SIM_FREE_ENERGY) {
    // what slf_fe.hip implements of the reference's model (lb_binary.py:139-372); everything else is named and refused
    slf::FreeEnergy& fe = c->fe;
    fe.enabled = 1;
    fe.Gamma = d->fe_Gamma; fe.kappa = d->fe_kappa; fe.A = d->fe_A;
    fe.tau_a = d->fe_tau_a; fe.tau_b = d->fe_tau_b; fe.tau_phi = d->tau_phi;
    fe.wall_phase = d->bc_wall_grad_phase;
    fe.wall_order = d->bc_wall_grad_order;
    for (int i = 0; i < 3; i++) fe.rim[i] = d->fe_zero_grad_rim[i];
    const char* why = nullptr;
    if (d->accel1[0] != 0.0 || d->accel1[1] != 0.0 || d->accel1[2] != 0.0)
      why = "free energy: body forces (free_energy_external_force, use_force_for_equilibrium) are not implemented";
    else if (!(d->fe_tau_a > 0.5) || !(d->fe_tau_b > 0.5) || !(d->tau_phi > 0.5)) why = "free energy: tau_a, tau_b and tau_phi must be > 0.5";
    else if (d->bc_wall_grad_order != 1 && d->bc_wall_grad_order != 2) why = "free energy: bc_wall_grad_order must be 1 or 2";
    for (int i = 0; !why && i < 3; i++) {
      if (d->fe_zero_grad_rim[i] < 0 || d->fe_zero_grad_rim[i] > 2) why = "free energy: fe_zero_grad_rim entries are 0, 1 (low rim) or 2 (high rim)";
    }
    if (why) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  }
  c->sc3 = slf::ShanChen3{};
  if (d->simtype == SLF_SIM_SHAN_CHEN_TERNARY) {
    // what slf_sc3.hip implements of the reference's model (lb_ternary.py); everything else is named and refused
    slf::ShanChen3& t = c->sc3;
    t.enabled = 1;
    t.tau_phi = d->tau_phi;
    t.tau_theta = d->tau_theta;
    for (int i = 0; i < 9; i++) t.G[i] = d->sc3_G[i];
    t.potential = d->sc_potential;
    for (int i = 0; i < 3; i++) { t.accel1[i] = d->accel1[i]; t.accel2[i] = d->accel2[i]; }
    const char* why = nullptr;
    if (!(d->tau_phi > 0.5) || !(d->tau_theta > 0.5)) why = "ternary Shan-Chen: tau_phi and tau_theta must be > 0.5";
    else if (d->sc_potential != 0 && d->sc_potential != 1) why = "ternary Shan-Chen: sc_potential is 0 (linear) or 1 (classic)";
    if (why) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  }
  // Workgroup = an x-chunk of one row.  Whole rows up to 1024 nodes are one
  // workgroup; longer rows are cut into 256-thread chunks.
  int bx = ((d->lat_nx - 2 + 63) / 64) * 64;
  if (bx > 1024) bx = 256;
  const char* env = getenv("SLF_BLOCK_X");
  if (env && atoi(env) >= 64 && atoi(env) <= 1024 && atoi(env) % 64 == 0) bx = atoi(env);
  const bool per_node = !c->sc.enabled && !c->fe.enabled && !c->sc3.enabled && !is_lat_lattice(d->lattice);
  if (per_node) {      // the launch bound of the module's per-node instantiations (the same for every step)
    const int bound = sweep_max_threads(per_node_variant_of(c->sel, g, ph, PROP_AB));
    if (bx > bound) bx = bound;
  }
  c->block_x = bx;
  c->n_node_params = d->n_node_params > 0 ? d->n_node_params : 0;
  if (per_node) {
    if (const char* why = per_node_variants_exist(*c)) return refuse(err, SLF_ERR_UNSUPPORTED, why);
  }
  return SLF_OK;
}

// ---- (b) the kernel table ------------------------------------------------------------------------------------------
// Module families: a name resolves to the row whose `families` holds the module's.
enum Family { F_SINGLE = 1, F_SC2 = 2, F_SCS = 4, F_FE = 8, F_SC3 = 16, F_ALL = 31 };

inline int family_of(const ModuleConfig& c) {
  if (c.sc3.enabled) return F_SC3;
  if (c.fe.enabled) return F_FE;
  return c.sc.enabled == 1 ? F_SC2 : (c.sc.enabled == 2 ? F_SCS : F_SINGLE);
}

// One row per (kernel name, module family).  `slots`: the pointer arguments in order, one letter each, named after the
// member of SweepArgs (Sc3Args for the ternary kinds) that receives them:
//   m map | a A b B c C  dist_in, dist_out, dist_in2, dist_out2 (ternary: dist_in[0], dist_out[0], ... [2]) |
//   r rho  p phi  t theta (ternary: field[0..2]) | v velocity, one pointer per dimension | l phi_laplacian |
//   x a pointer the launch reads from BoundArgs::ptrs by position (halo and PBC kernels)
// n_ints: the integer arguments; in the sweeps the first one is the options word.  FACE_INTS / BOX_INTS: see bind().
// launch: what slf_kernel_launch checks for this kind, one letter per check in order (part (f), launch_check()).
// nodes_in_front: modules with indirect addressing put the `nodes` table in front of the list (reference
// _add_indirect_args, subdomain_runner.py:1153-1157).  local_velocity: SweepArgs::sc_local_velocity.
constexpr int FACE_INTS = -1, BOX_INTS = -2;
struct KernelRow {
  const char* name;
  KernelKind kind;
  int families;
  const char* slots;
  int n_ints;
  bool nodes_in_front, local_velocity;
  const char* launch;      // the checks of slf_kernel_launch, in order: part (f), launch_check()
};

inline constexpr KernelRow KERNEL_TABLE[] = {
  // single fluid (lb_single.py:72-133); single-component Shan-Chen shares the lists
  {"CollideAndPropagate", KK_COLLIDE_AND_PROPAGATE, F_SINGLE, "maArv", 1, true, false, "pfmns"},     // [, alpha]: bind()
  {"CollideAndPropagate", KK_SCS_SWEEP, F_SCS, "maArv", 1, true, false, "nms"},
  {"ComputeMacroFields", KK_COMPUTE_MACRO, F_SINGLE | F_SCS, "maArv", 1, true, false, "pmnS"},
  {"PrepareMacroFields", KK_SCS_MACRO, F_SCS, "mar", 1, true, false, "nmS"},
  {"SetInitialConditions", KK_SET_INITIAL_CONDITIONS, F_SINGLE | F_SCS, "avrm", 0, true, false, "n"},
  {"SetInitialConditions", KK_SC_INIT, F_SC2, "mabvrp", 0, true, false, "n"},                    // lb_binary.py:107-127
  {"SetInitialConditions", KK_FE_INIT, F_FE, "mabvrp", 0, false, false, ""},
  {"SetInitialConditions", KK_SC3_INIT, F_SC3, "mabcvrpt", 0, false, false, ""},                // lb_ternary.py:118-142
  // several steps inside one launch: map, src a, src b, dst a, dst b | options, steps, tile x, tile y, halo
  {"CollideAndPropagateResident", KK_RESIDENT, F_ALL & ~F_SC3, "mabAB", 5, false, false, "m"},
  // binary Shan-Chen (lb_binary.py:457-465): the pass reads both lattices (dist_in, dist_out)
  {"ShanChenPrepareMacroFields", KK_SC_MACRO, F_SC2, "maArpv", 1, true, false, "nms"},
  {"ShanChenCollideAndPropagate0", KK_SC_SWEEP0, F_SC2, "maArpv", 1, true, false, "nms"},
  {"ShanChenCollideAndPropagate1", KK_SC_SWEEP1, F_SC2, "maArpv", 1, true, false, "nms"},
  {"ShanChenCollideAndPropagateFused", KK_SC_FUSED, F_SC2, "maAbBrpv", 1, false, false, "nms"},
  {"ShanChenPrepareDensities", KK_SC_MACRO, F_SC2, "maArpv", 1, true, true, "nms"},
  {"ShanChenCollideAndPropagateFusedV", KK_SC_FUSED, F_SC2, "maAbBrpv", 1, false, true, "nms"},
  // ternary Shan-Chen (lb_ternary.py:220-333): the names it shares with the binary model take the ternary lists
  {"ShanChenPrepareMacroFields", KK_SC3_MACRO, F_SC3, "mabcrptv", 1, false, false, "Ms"},
  {"ShanChenCollideAndPropagate0", KK_SC3_SWEEP0, F_SC3, "maArptv", 1, false, false, "Ms"},
  {"ShanChenCollideAndPropagate1", KK_SC3_SWEEP1, F_SC3, "maArptv", 1, false, false, "Ms"},
  {"ShanChenCollideAndPropagate2", KK_SC3_SWEEP2, F_SC3, "maArptv", 1, false, false, "Ms"},
  {"ShanChenCollideAndPropagateFused", KK_SC3_FUSED, F_SC3, "maAbBcCrptv", 1, false, false, "Ms"},
  // free energy (lb_binary.py:295-308)
  {"FreeEnergyPrepareMacroFields", KK_FE_MACRO, F_FE, "maArp", 1, false, false, "ms"},
  {"FreeEnergyCollideAndPropagateFluid", KK_FE_FLUID, F_FE, "maArpvl", 1, false, false, "ms"},
  {"FreeEnergyCollideAndPropagateOrderParam", KK_FE_ORDER, F_FE, "maApvl", 1, false, false, "ms"},
  // ghost layers and halo, every family: dist | field, axis
  {"ApplyPeriodicBoundaryConditions", KK_PBC, F_ALL, "x", 1, false, false, ""},
  {"ApplyPeriodicBoundaryConditionsWithSwap", KK_PBC_SWAP, F_ALL, "x", 1, false, false, ""},
  {"ApplyMacroPeriodicBoundaryConditions", KK_MACRO_PBC, F_ALL, "x", 1, false, false, ""},
  {"CollectSparseData", KK_COLLECT_SPARSE, F_ALL, "xxx", 1, false, false, ""},                  // idx_array, dist, buffer, n
  {"DistributeSparseData", KK_DISTRIBUTE_SPARSE, F_ALL, "xxx", 1, false, false, ""},
  {"CollectContinuousData", KK_COLLECT_BOX, F_ALL, "xx", BOX_INTS, false, false, "b"},
  {"DistributeContinuousData", KK_DISTRIBUTE_BOX, F_ALL, "xx", BOX_INTS, false, false, "b"},
  {"CollectContinuousDataWithSwap", KK_COLLECT_FACE_SWAP, F_ALL, "xx", FACE_INTS, false, false, "F"},
  {"DistributeContinuousDataWithSwap", KK_DISTRIBUTE_FACE_SWAP, F_ALL, "xx", FACE_INTS, false, false, "F"},
  {"CollectContinuousMacroData", KK_COLLECT_MACRO_FACE, F_ALL, "xx", FACE_INTS, false, false, "F"},
  {"DistributeContinuousMacroData", KK_DISTRIBUTE_MACRO_FACE, F_ALL, "xx", FACE_INTS, false, false, "F"},
};

inline bool is_ternary_kind(KernelKind kk) { return kk >= KK_SC3_MACRO && kk <= KK_SC3_INIT; }
inline bool is_face_kind(KernelKind kk) { return kk >= KK_COLLECT_FACE_SWAP && kk <= KK_DISTRIBUTE_MACRO_FACE; }
inline bool is_box_kind(KernelKind kk) { return kk == KK_COLLECT_BOX || kk == KK_DISTRIBUTE_BOX; }

// the name exists, but not in this module's family: which message says so
inline int wrong_family(const ModuleConfig& c, const KernelRow& named, std::string* err) {
  const std::string name(named.name);
  const int fam = family_of(c);
  if (fam == F_SC3) {
    if (named.local_velocity)
      return refuse(err, SLF_ERR_NOT_FOUND, name + " does not exist in a module built with simtype = SLF_SIM_SHAN_CHEN_TERNARY "
                                            "(the fused sweep reads the velocity of the pass in front)");
    return refuse(err, SLF_ERR_NOT_FOUND, name + " does not exist in a module built with simtype = "
                                          "SLF_SIM_SHAN_CHEN_TERNARY: single-fluid, binary and free-energy kernels are other modules'");
  }
  switch (named.kind) {
    case KK_SC3_SWEEP2:
      return refuse(err, SLF_ERR_NOT_FOUND, name + " only exists in modules built with simtype = SLF_SIM_SHAN_CHEN_TERNARY");
    case KK_SCS_MACRO:
      return refuse(err, SLF_ERR_NOT_FOUND, "PrepareMacroFields only exists in single-component Shan-Chen modules");
    case KK_SC_MACRO: case KK_SC_SWEEP0: case KK_SC_SWEEP1: case KK_SC_FUSED:
      return refuse(err, SLF_ERR_NOT_FOUND, "Shan-Chen kernels only exist in modules built with simtype = SLF_SIM_SHAN_CHEN_BINARY");
    case KK_FE_MACRO: case KK_FE_FLUID: case KK_FE_ORDER:
      return refuse(err, SLF_ERR_NOT_FOUND, "FreeEnergy... kernels only exist in modules built with simtype = SLF_SIM_FREE_ENERGY");
    default:      // CollideAndPropagate, ComputeMacroFields
      return refuse(err, SLF_ERR_NOT_FOUND, fam == F_FE ? "single-fluid kernels do not exist in a free-energy module"
                                                         : "single-fluid kernels do not exist in a Shan-Chen module");
  }
}

// what the resident kernel serves (slf_resident.hip): 2-D single-fluid modules, direct addressing, the standard
// density formulation, node kinds whose code touches nothing but the node's own populations
inline int resident_refusal(const ModuleConfig& c, std::string* err) {
  const Geometry& g = c.geo;
  if (g.dim != 2 || c.sc.enabled || c.fe.enabled || g.indirect || c.phys.incompressible == SLF_DENSITY_ROUNDOFF || c.phys.regularized ||
      c.phys.subgrid || c.sel.model == SLF_ELBM)
    return refuse(err, SLF_ERR_UNSUPPORTED, "CollideAndPropagateResident: 2-D single-fluid modules with direct addressing and the "
                                            "standard density formulation only");
  if (g.axis_mode[0] == 1 || g.axis_mode[1] == 1)
    return refuse(err, SLF_ERR_UNSUPPORTED, "CollideAndPropagateResident: periodic axes must be wrapped in-sweep (periodic_fused)");
  for (int t = 0; t < 16; t++) {
    const int kind = type_kind(g.type_lut, (uint32_t)t);
    if (kind == NK_HALF_BB || kind == NK_COPY || kind == NK_YU_OUTFLOW || kind == NK_DO_NOTHING)
      return refuse(err, SLF_ERR_UNSUPPORTED, "CollideAndPropagateResident: half-way bounce-back, TMS wall, outflow and do-nothing nodes read / "
                                              "write memory from their node code");
  }
  return SLF_OK;
}

// The row that serves `name` in a module of this configuration, or why there is none.
inline int resolve(const ModuleConfig& c, const char* name, const KernelRow** out, std::string* err) {
  const int fam = family_of(c);
  const KernelRow* named = nullptr;
  const KernelRow* row = nullptr;
  for (const KernelRow& r : KERNEL_TABLE) {
    if (strcmp(r.name, name)) continue;
    if (!named) named = &r;
    if (r.families & fam) {
      row = &r;
      break;
    }
  }
  if (!named) return refuse(err, SLF_ERR_NOT_FOUND, std::string("unknown kernel: ") + name);
  if (!row) return wrong_family(c, *named, err);
  const KernelKind kk = row->kind;
  if (is_lat_lattice(c.sel.lattice)) {
    // D3Q15 / D3Q27: CollideAndPropagate, ComputeMacroFields, SetInitialConditions and the ghost-layer kernels are served by
    // slf_lat.hip; the sparse, box and macro-field kernels never look at a direction; everything else is refused here
    const std::string lat = c.sel.lattice == SLF_D3Q15 ? "D3Q15" : "D3Q27";
    if (kk == KK_RESIDENT)
      return refuse(err, SLF_ERR_UNSUPPORTED, lat + ": CollideAndPropagateResident is not implemented on this lattice (2-D lattices only)");
    if (is_face_kind(kk))
      return refuse(err, SLF_ERR_UNSUPPORTED, lat + ": " + name + " (the reference's face argument lists) is not implemented on this "
                                              "lattice; faces travel through Collect / DistributeContinuousData with a direction mask or "
                                              "through index lists");
  }
  if (kk == KK_RESIDENT) {
    if (c.phys.accel_field)
      return refuse(err, SLF_ERR_UNSUPPORTED, "CollideAndPropagateResident: accel_field modules are not served (the resident kernel "
                                              "takes a constant acceleration)");
    if (c.phys.equilibrium == SLF_EQ_SHALLOW_WATER)
      return refuse(err, SLF_ERR_UNSUPPORTED, "CollideAndPropagateResident: shallow-water modules are not served (the resident kernel "
                                              "implements the BGK polynomial)");
    if (int rc = resident_refusal(c, err)) return rc;
  }
  if ((kk == KK_PBC || kk == KK_PBC_SWAP) && c.geo.indirect)
    return refuse(err, SLF_ERR_UNSUPPORTED, "indirect addressing: periodic boundaries are wrapped inside the sweep "
                                            "(periodic_fused), there are no ghost-layer PBC kernels");
  if (kk == KK_PBC_SWAP && c.access_pattern != SLF_AA)
    return refuse(err, SLF_ERR_NOT_FOUND, "ApplyPeriodicBoundaryConditionsWithSwap only exists for the AA access pattern");
  if ((kk == KK_COLLECT_FACE_SWAP || kk == KK_DISTRIBUTE_FACE_SWAP) && c.access_pattern != SLF_AA)
    return refuse(err, SLF_ERR_NOT_FOUND, "Collect / DistributeContinuousDataWithSwap only exist for the AA access pattern "
                                          "(reference kernel_utils.mako:536, 638, 700, 786)");
  if (is_face_kind(kk) && c.geo.indirect)
    return refuse(err, SLF_ERR_UNSUPPORTED, "indirect addressing: halo through index lists (Collect / DistributeSparseData)");
  *out = row;
  return SLF_OK;
}

// The arguments of one kernel as slf_kernel_set_args() bound them: by member for the sweeps, by position for the rest.
constexpr int MAX_BOUND_PTRS = 16, MAX_BOUND_INTS = 8;
struct BoundArgs {
  SweepArgs sweep;
  Sc3Args sc3;                                  // the ternary kinds
  unsigned long long ptrs[MAX_BOUND_PTRS];      // 'P' args in order
  long long ints[MAX_BOUND_INTS];               // 'i' args in order
  int n_ptrs, n_ints;
  bool alpha_arg;      // CollideAndPropagate of an entropic module: the last pointer is the alpha field
  bool build_slots;    // indirect sweep over the slots: the slot -> node table of sweep.nodes has to be built
};

inline void put_slot(BoundArgs* b, bool ternary, char slot, int d, unsigned long long value) {
  void* p = (void*)value;
  SweepArgs& a = b->sweep;
  Sc3Args& t = b->sc3;
  switch (slot) {
    case 'm': (ternary ? t.map : a.map) = p; break;
    case 'a': (ternary ? t.dist_in[0] : a.dist_in) = p; break;
    case 'A': (ternary ? t.dist_out[0] : a.dist_out) = p; break;
    case 'b': (ternary ? t.dist_in[1] : a.dist_in2) = p; break;
    case 'B': (ternary ? t.dist_out[1] : a.dist_out2) = p; break;
    case 'c': t.dist_in[2] = p; break;
    case 'C': t.dist_out[2] = p; break;
    case 'r': (ternary ? t.field[0] : a.rho) = p; break;
    case 'p': (ternary ? t.field[1] : a.phi) = p; break;
    case 't': t.field[2] = p; break;
    case 'v': (ternary ? t.v[d] : a.v[d]) = p; break;
    case 'l': a.lap = p; break;
  }
}

// Checks format and counts of an argument list against the row and writes the arguments into *b, once.
inline int bind(const ModuleConfig& c, const KernelRow& row, const char* fmt, const void* const* argv, int argc, BoundArgs* b,
                std::string* err) {
  if ((int)strlen(fmt) != argc) return refuse(err, SLF_ERR_INVALID, "format / argc mismatch");
  *b = BoundArgs{};
  for (int i = 0; i < argc; i++) {
    switch (fmt[i]) {
      case 'P':
        if (b->n_ptrs < MAX_BOUND_PTRS) b->ptrs[b->n_ptrs] = *(const unsigned long long*)argv[i];
        b->n_ptrs++;
        break;
      case 'i':
        if (b->n_ints < MAX_BOUND_INTS) b->ints[b->n_ints] = *(const int32_t*)argv[i];
        b->n_ints++;
        break;
      default: return refuse(err, SLF_ERR_INVALID, std::string("unsupported format char: ") + fmt[i]);
    }
  }
  const int dim = c.geo.dim;
  const KernelKind kk = row.kind;
  int want_p = 0, want_i = row.n_ints;
  for (const char* s = row.slots; *s; s++) want_p += *s == 'v' ? dim : 1;
  const char* face_fmt = dim == 3 ? "PiiiiiP" : "PiiiP";
  if (is_box_kind(kk)) {
    // dist, buffer, dirs, base, col_stride, ncols, row_stride, nrows [, buffer stride between directions, between rows]
    want_i = (b->n_ints == 8) ? 8 : 6;
    // ... or the reference's own argument list (kernel_utils.mako:526-543, 629-645, 692-708, 777-793):
    // 3-D (dist, face, base_gx, base_other, max_lx, max_other, buffer), 2-D (dist, face, base_gx, max_lx, buffer)
    if (b->n_ints == (dim == 3 ? 5 : 3)) {
      want_i = b->n_ints;
      if (is_lat_lattice(c.sel.lattice))
        return refuse(err, SLF_ERR_UNSUPPORTED, "D3Q15 / D3Q27: the reference's face argument list is not implemented on these lattices; "
                                                "pass the direction mask and the box");
      if (strcmp(fmt, face_fmt)) return refuse(err, SLF_ERR_INVALID, "reference form: the buffer is the last argument");
      if (c.geo.indirect) return refuse(err, SLF_ERR_UNSUPPORTED, "indirect addressing: halo through index lists");
    }
  } else if (is_face_kind(kk)) {
    // 3-D (dist | field, face, base_gx, base_other, max_lx, max_other, buffer); 2-D (dist, face, base_gx, max_lx, buffer),
    // macro (field, base_gx, max_lx, gy, buffer)   kernel_utils.mako:839-953
    want_i = dim == 3 ? 5 : 3;
    if (strcmp(fmt, face_fmt))
      return refuse(err, SLF_ERR_INVALID, (kk == KK_COLLECT_MACRO_FACE || kk == KK_DISTRIBUTE_MACRO_FACE)
                                              ? "arguments: (field, [face,] base_gx, ..., buffer)"
                                              : "arguments: (dist, face, base_gx[, base_other], max_lx[, max_other], buffer)");
  }
  if (c.geo.indirect && (kk == KK_SC_FUSED || row.local_velocity))
    return refuse(err, SLF_ERR_UNSUPPORTED, "indirect addressing: the binary model runs the reference's pass and its two per-lattice sweeps");
  const bool nodes = c.geo.indirect && row.nodes_in_front;
  if (nodes) want_p += 1;
  if (kk == KK_COLLIDE_AND_PROPAGATE && c.sel.model == SLF_ELBM && b->n_ptrs == want_p + 1 && fmt[argc - 1] == 'P') {
    // entropic modules: the alpha field, the LAST argument (reference lb_single.py:129-133: behind the options word)
    want_p += 1;
    b->alpha_arg = true;
  }
  const bool ternary = is_ternary_kind(kk);
  if (ternary && (b->n_ptrs != want_p || b->n_ints != want_i))
    return refuse(err, SLF_ERR_INVALID, "argument list does not match the kernel's signature: in a module built with simtype = "
                                        "SLF_SIM_SHAN_CHEN_TERNARY the Shan-Chen kernels and SetInitialConditions take the ternary "
                                        "argument lists (three lattices; rho, phi, theta)");
  if (b->n_ptrs != want_p || b->n_ints != want_i)
    return refuse(err, SLF_ERR_INVALID, "argument list does not match the kernel's signature");
  int next = 0;
  if (nodes) b->sweep.nodes = (const void*)b->ptrs[next++];
  for (const char* s = row.slots; *s; s++) {
    if (*s == 'v') {
      for (int d = 0; d < dim; d++) put_slot(b, ternary, 'v', d, b->ptrs[next++]);
    } else {
      put_slot(b, ternary, *s, 0, b->ptrs[next++]);
    }
  }
  if (b->alpha_arg) b->sweep.alpha = (void*)b->ptrs[next];
  if (row.slots[0] != 'x' && want_i > 0) (ternary ? b->sc3.options : b->sweep.options) = (uint32_t)b->ints[0];
  b->sweep.sc_local_velocity = row.local_velocity;
  b->build_slots = kk == KK_COLLIDE_AND_PROPAGATE && c.geo.indirect && b->n_ptrs > 0 &&
                   c.phys.incompressible != SLF_DENSITY_ROUNDOFF && !c.phys.regularized && !c.phys.subgrid &&
                   c.sel.model != SLF_ELBM;
  return SLF_OK;
}

// ---- (c) the face box ------------------------------------------------------------------------------------------------
// The reference's face kernels (kernel_utils.mako:476-953), mapped onto the box kernel.  face: 2 Y_LOW, 3 Y_HIGH,
// 4 Z_LOW, 5 Z_HIGH (subdomain.py:30-36); the layer a kernel reads / writes is lat_linear / lat_linear_macro /
// lat_linear_dist / lat_linear_with_swap of subdomain_runner.py:486-510; the populations are
// get_interblock_dists(grid, normal(face)) in ascending order -- their opposite slots in the ...WithSwap kernels --
// buffer [k][other][x] (2-D: [k][x]).  `ints`: the integer arguments of the reference form (bind()).
struct FaceBox {
  bool collect, macro;
  int layer;
  int dirs[32], nd;
  unsigned long long base;
  long long row_stride;
  int ncols, nrows;
  long long col_stride, buf_k_stride, buf_row_stride;      // a face: 1 and the dense buffer [k][r][c] (0, 0)
};

inline int face_box(const Geometry& g, KernelKind kind, const long long* ints, FaceBox* box, const char** err) {
  const bool collect = kind == KK_COLLECT_BOX || kind == KK_COLLECT_FACE_SWAP || kind == KK_COLLECT_MACRO_FACE;
  const bool swap = kind == KK_COLLECT_FACE_SWAP || kind == KK_DISTRIBUTE_FACE_SWAP;
  const bool macro = kind == KK_COLLECT_MACRO_FACE || kind == KK_DISTRIBUTE_MACRO_FACE;
  int face, base_gx, base_other = 0, max_lx, max_other = 1, layer = -1;
  if (g.dim == 3) {
    face = (int)ints[0]; base_gx = (int)ints[1]; base_other = (int)ints[2];
    max_lx = (int)ints[3]; max_other = (int)ints[4];
  } else if (macro) {
    face = 2; base_gx = (int)ints[0]; max_lx = (int)ints[1]; layer = (int)ints[2];
  } else {
    face = (int)ints[0]; base_gx = (int)ints[1]; max_lx = (int)ints[2];
  }
  if (face < 2 || face >= 2 * g.dim) return refuse(err, SLF_ERR_INVALID, "face must be a Y or Z face (X faces travel through index lists / x-face buffers)");
  const int axis = face >> 1;
  const bool low = (face & 1) == 0;
  const int lat = axis == 1 ? g.lat_ny : g.lat_nz;
  if (layer < 0) {
    if (macro) layer = collect ? (low ? 1 : lat - 2) : (low ? 0 : lat - 1);             // lat_linear_macro / lat_linear
    else if (collect) layer = swap ? (low ? 1 : lat - 2) : (low ? 0 : lat - 1);        // lat_linear_macro / lat_linear
    else layer = swap ? (low ? lat - 1 : 0) : (low ? lat - 2 : 1);                     // lat_linear_with_swap / lat_linear_dist
  }
  int dirs[32], nd = 0;
  if (macro) {
    dirs[nd++] = 0;
  } else {
    const int sign = low ? -1 : 1;
    for (int q = 1; q < (g.dim == 3 ? 19 : 9); q++) {
      const int ea = g.dim == 3 ? slf::e_comp<slf::D3Q19>(q, axis) : slf::e_comp<slf::D2Q9>(q, axis);
      if (ea == sign) dirs[nd++] = swap ? (g.dim == 3 ? slf::D3Q19::opp(q) : slf::D2Q9::opp(q)) : q;
    }
  }
  int ncols, nrows;
  if (g.dim == 3) {
    if (max_other % nd) return refuse(err, SLF_ERR_INVALID, "max_other must be a multiple of the number of populations that cross the face");
    ncols = max_lx; nrows = max_other / nd;
  } else {
    if (!macro && max_lx % nd) return refuse(err, SLF_ERR_INVALID, "max_lx must be a multiple of the number of populations that cross the face");
    ncols = macro ? max_lx : max_lx / nd; nrows = 1;
  }
  const long long row_stride = axis == 1 ? (long long)g.arr_nxy : (long long)g.arr_nx;   // rows run along the other axis
  const unsigned long long base = (unsigned long long)base_gx +
      (axis == 1 ? (unsigned long long)g.arr_nx * layer + (unsigned long long)g.arr_nxy * base_other
                 : (unsigned long long)g.arr_nx * base_other + (unsigned long long)g.arr_nxy * layer);
  const int lat_other = g.dim == 3 ? (axis == 1 ? g.lat_nz : g.lat_ny) : 1;       // extent along the rows' axis
  if (base_gx < 0 || base_gx + ncols > g.arr_nx || base_other < 0 || base_other + nrows > lat_other || layer < 0 || layer >= lat)
    return refuse(err, SLF_ERR_INVALID, "face box outside the subdomain (base_gx + max_lx, base_other + rows or the layer exceed the arrays)");
  box->collect = collect; box->macro = macro; box->layer = layer;
  for (int i = 0; i < nd; i++) box->dirs[i] = dirs[i];
  box->nd = nd; box->base = base; box->row_stride = row_stride; box->ncols = ncols; box->nrows = nrows;
  box->col_stride = 1; box->buf_k_stride = box->buf_row_stride = 0;
  return SLF_OK;
}

// ---- (d) immersed boundary markers (slf_ibm_*; kernels: slf_ibm.hip) ---------------------------------------------------
// The arguments of one slf_ibm_* call.  `what`: the entry point's name, for the message.  has_field: the module holds an
// acceleration field (slf_module_set_accel_field was called).  ptrs / names: the pointers that must not be NULL.
constexpr int IBM_MAX_MARKERS = 1 << 24;
inline int ibm_check(const ModuleConfig& c, bool has_field, const char* what, int n_markers, const int32_t* origin,
                     const void* const* ptrs, const char* const* names, int n_ptrs, std::string* err) {
  const std::string w = std::string(what) + ": ";
  if (c.sel.lattice != SLF_D2Q9 && c.sel.lattice != SLF_D3Q19)
    return refuse(err, SLF_ERR_UNSUPPORTED, w + "D2Q9 and D3Q19 modules only (D3Q15 / D3Q27 have no acceleration field)");
  if (!c.phys.accel_field)
    return refuse(err, SLF_ERR_INVALID, w + "the module was created without an acceleration field (accel_field): the markers "
                                            "have nothing to spread their forces into");
  if (c.sc.enabled || c.fe.enabled || c.sc3.enabled || c.geo.indirect)
    return refuse(err, SLF_ERR_UNSUPPORTED, w + "single-fluid modules with direct addressing only");
  if (!has_field)
    return refuse(err, SLF_ERR_INVALID, w + "no field is set (slf_module_set_accel_field): the kernels rewrite that buffer");
  if (n_markers <= 0) return refuse(err, SLF_ERR_INVALID, w + "the marker count must be positive");
  if (n_markers > IBM_MAX_MARKERS) return refuse(err, SLF_ERR_INVALID, w + "at most 2^24 markers per call");
  if (!origin) return refuse(err, SLF_ERR_INVALID, w + "origin is NULL");
  for (int d = 0; d < 3; d++) {
    if (origin[d] < -(1 << 30) || origin[d] > (1 << 30))
      return refuse(err, SLF_ERR_INVALID, w + "origin beyond +-2^30");
  }
  for (int i = 0; i < n_ptrs; i++) {
    if (!ptrs[i]) return refuse(err, SLF_ERR_INVALID, w + names[i] + " is NULL");
  }
  return SLF_OK;
}

// ---- (e) thermal flows (slf_thermal_*; kernels: slf_thermal.hip) ----------------------------------------------------------
// The arguments of one slf_thermal_* call.  `what`: the entry point's name, for the message.  has_field: the module holds an
// acceleration field (slf_module_set_accel_field was called).  map: the node map argument.  ptrs / names: the pointers that
// must not be NULL.  src / dst: the two copies of the temperature lattice (NULL / NULL where the call takes one: init).
inline int thermal_check(const ModuleConfig& c, bool has_field, const char* what, const slf_thermal_params* params, const void* map,
                         const void* const* ptrs, const char* const* names, int n_ptrs, const void* src, const void* dst,
                         std::string* err) {
  const std::string w = std::string(what) + ": ";
  if (c.sel.lattice != SLF_D2Q9 && c.sel.lattice != SLF_D3Q19)
    return refuse(err, SLF_ERR_UNSUPPORTED, w + "D2Q9 and D3Q19 modules only (D3Q15 / D3Q27 have no acceleration field)");
  if (!c.phys.accel_field)
    return refuse(err, SLF_ERR_INVALID, w + "the module was created without an acceleration field (accel_field): the buoyancy "
                                            "has nothing to be written into");
  if (c.sc.enabled || c.fe.enabled || c.sc3.enabled || c.geo.indirect)
    return refuse(err, SLF_ERR_UNSUPPORTED, w + "single-fluid modules with direct addressing only");
  if (!has_field)
    return refuse(err, SLF_ERR_INVALID, w + "no field is set (slf_module_set_accel_field): the kernels rewrite that buffer");
  if (!params) return refuse(err, SLF_ERR_INVALID, w + "params is NULL");
  if (!(params->omega_T > 0.0 && params->omega_T < 2.0))
    return refuse(err, SLF_ERR_INVALID, w + "omega_T must lie in (0, 2): tau_T > 1/2, a positive diffusivity");
  const double consts[4] = {params->T_ref, params->b[0], params->b[1], params->b[2]};
  for (double x : consts) {
    if (!(x - x == 0.0)) return refuse(err, SLF_ERR_INVALID, w + "T_ref and b must be finite");
  }
  if (!map && c.sel.general)
    return refuse(err, SLF_ERR_INVALID, w + "map is NULL, but the module has node types (which nodes are wet is read off the "
                                            "node map)");
  for (int i = 0; i < n_ptrs; i++) {
    if (!ptrs[i]) return refuse(err, SLF_ERR_INVALID, w + names[i] + " is NULL");
  }
  if (src && src == dst)
    return refuse(err, SLF_ERR_INVALID, w + "g_src == g_dst: the temperature lattice is two-copy, a step reads one copy and "
                                            "writes the other");
  if (c.geo.lat_ny - 2 > 4 * 65535 || c.geo.lat_nz - 2 > 65535)
    return refuse(err, SLF_ERR_UNSUPPORTED, w + "more than 262140 rows or 65535 layers (the launch grid runs over them)");
  return SLF_OK;
}

// ---- (f) the launch (slf_kernel_launch) and the setters' argument checks ------------------------------------------------------
// What stands between a caller and an out-of-bounds kernel.  Which checks a kind gets, and in which order, is the column
// `launch` of its row in KERNEL_TABLE, one letter per check; the first that fails answers:
//   p  a pair sweep is armed (slf_kernel_set_pair): whole-box launches only, and nothing further is asked
//   f  an accel_field module has its field (slf_module_set_accel_field)
//   m  the node map is not NULL in a module with node types; M: the same for the ternary kinds' own argument list
//   n  the `nodes` table is not NULL under indirect addressing
//   s  the kernel takes a propagation step and rows: an AA kernel has its iteration, the region lies inside the real nodes
//      (y0 == y1 is an empty launch; 2-D: z0 = 0, z1 = 1, the region's z is not read); S: the same for a kernel that
//      always covers every real node (the region is neither read nor validated)
//   b  a box transfer: at most 12 directions per launch, or the reference's face argument list (face_box)
//   F  the reference's face argument list (face_box)
// A kind without s / S uses no propagation step.  A new kernel kind puts its rule into that column.
struct LaunchState {      // what the kernel and module objects hold when the launch is asked for
  int needs_iteration;
  uint32_t iteration;
  bool has_field;         // slf_module_set_accel_field was called
  bool pair_armed;        // slf_kernel_set_pair accepted
};
struct LaunchShape {
  Prop prop;
  int y0, y1, z0, z1;
};

// *shape: the step and the rows of the launch; *box: what a box / face kind moves (those kinds only).  Builds no string and
// allocates nothing unless a check fails.
inline int launch_check(const ModuleConfig& c, const KernelRow& row, const BoundArgs& b, const LaunchState& st,
                        const slf_region* region, LaunchShape* shape, FaceBox* box, std::string* err) {
  const Geometry& g = c.geo;
  *shape = LaunchShape{PROP_AB, 1, g.lat_ny - 1, g.dim == 2 ? 0 : 1, g.dim == 2 ? 1 : g.lat_nz - 1};
  for (const char* rule = row.launch; *rule; rule++) {
    switch (*rule) {
      case 'p':
        if (!st.pair_armed) break;
        if (region) return refuse(err, SLF_ERR_UNSUPPORTED, "pair sweep: whole-box launches only");
        return SLF_OK;
      case 'f':
        if (c.phys.accel_field && !st.has_field)
          return refuse(err, SLF_ERR_INVALID, "CollideAndPropagate: the module was created with accel_field, but no field is set "
                                              "(slf_module_set_accel_field)");
        break;
      case 'm': case 'M':
        if (c.sel.general && !(*rule == 'M' ? b.sc3.map : b.sweep.map))
          return refuse(err, SLF_ERR_INVALID, "node map is NULL but the module is not fluid_only");
        break;
      case 'n':
        if (g.indirect && !b.sweep.nodes) return refuse(err, SLF_ERR_INVALID, "indirect addressing: the nodes table is NULL");
        break;
      case 's': case 'S':
        if (c.access_pattern == SLF_AA) {
          if (!st.needs_iteration) return refuse(err, SLF_ERR_INVALID, "AA kernels need the iteration argument");
          shape->prop = (st.iteration & 1u) ? PROP_AA_ODD : PROP_AA_EVEN;
        }
        if (region && *rule == 's') {
          shape->y0 = region->y0; shape->y1 = region->y1;
          if (g.dim == 3) { shape->z0 = region->z0; shape->z1 = region->z1; }
          if (shape->y0 < 1 || shape->y1 > g.lat_ny - 1 || shape->y0 > shape->y1 ||
              (g.dim == 3 && (shape->z0 < 1 || shape->z1 > g.lat_nz - 1 || shape->z0 > shape->z1)))
            return refuse(err, SLF_ERR_INVALID, "region outside the real nodes of the subdomain");
        }
        break;
      case 'b':
        if (b.n_ints >= 6) {      // dirs (a bit mask, ascending), base, col_stride, ncols, row_stride, nrows [, buffer strides]
          *box = FaceBox{};
          box->collect = row.kind == KK_COLLECT_BOX;
          for (int q = 0; q < 32; q++) if (((unsigned int)b.ints[0] >> q) & 1u) box->dirs[box->nd++] = q;
          if (box->nd > 12)
            return refuse(err, SLF_ERR_INVALID, "Collect/DistributeContinuousData: at most 12 directions per launch (a face of D3Q19 carries 5)");
          box->base = (unsigned long long)(uint32_t)b.ints[1]; box->col_stride = b.ints[2]; box->ncols = (int)b.ints[3];
          box->row_stride = b.ints[4]; box->nrows = (int)b.ints[5];
          if (b.n_ints == 8) { box->buf_k_stride = b.ints[6]; box->buf_row_stride = b.ints[7]; }
          break;
        }
        [[fallthrough]];      // the reference's own argument list
      case 'F': {
        const char* why = nullptr;
        if (int rc = face_box(g, row.kind, b.ints, box, &why)) return refuse(err, rc, why);
        break;
      }
    }
  }
  return SLF_OK;
}

// CollideAndPropagateResident: what its integer arguments (options, steps, tile x, tile y, halo) and arrays must satisfy
inline int resident_check(const ModuleConfig& c, const BoundArgs& b, int needs_iteration, std::string* err) {
  const SweepArgs& a = b.sweep;      // dist_in / dist_in2: source a / b, dist_out / dist_out2: destination a / b
  const bool aa = c.access_pattern == SLF_AA;
  const int steps = (int)b.ints[1], tx = (int)b.ints[2], ty = (int)b.ints[3], halo = (int)b.ints[4];
  if (!needs_iteration) return refuse(err, SLF_ERR_INVALID, "CollideAndPropagateResident needs the iteration argument (its first step)");
  if (steps < 1 || tx < 1 || ty < 1 || halo < 1) return refuse(err, SLF_ERR_INVALID, "steps, tile and halo must be positive");
  if (!a.dist_in || !a.dist_out || (!aa && (!a.dist_in2 || !a.dist_out2)))
    return refuse(err, SLF_ERR_INVALID, "CollideAndPropagateResident: source and destination arrays (both copies of the two-copy pattern)");
  if (a.dist_in == a.dist_out || (!aa && a.dist_in2 == a.dist_out2))
    return refuse(err, SLF_ERR_INVALID, "CollideAndPropagateResident: source and destination must be different buffers");
  // the halo that `steps` steps need depends on the parity of the first one: the worse of the two must fit
  const int even = resident_halo(aa, 0, steps), odd = resident_halo(aa, 1, steps);
  if (halo < (even > odd ? even : odd)) return refuse(err, SLF_ERR_INVALID, "CollideAndPropagateResident: halo too small for this many steps");
  const long long nw = (long long)(tx + 2 * halo) * (long long)(ty + 2 * halo);
  if (nw > 2 * 1024) return refuse(err, SLF_ERR_INVALID, "CollideAndPropagateResident: window larger than 2048 nodes");
  const int q = 9;
  // the window (dynamic LDS) + the kernel's own tables (static: the list of a window's boundary-condition nodes,
  // slf_resident.hip) share the 160 KiB of a workgroup
  if (resident_lds_bytes(q, c.sel.precision, aa, tx + 2 * halo, ty + 2 * halo) + 4352 > 160 * 1024)
    return refuse(err, SLF_ERR_INVALID, "CollideAndPropagateResident: window does not fit the 160 KiB of LDS");
  return SLF_OK;
}

// slf_module_set_xface_buffers / slf_plan_add_xface_buffers: [0] send low, [1] send high, [2] receive low, [3] receive high
inline int xface_buffers_check(const ModuleConfig* c, const void* const xf[4], std::string* err) {
  if (!c) return refuse(err, SLF_ERR_INVALID, "module is NULL");
  if (!xf[0] && !xf[1] && !xf[2] && !xf[3]) return SLF_OK;
  const Geometry& g = c->geo;
  if (is_lat_lattice(c->sel.lattice))
    return refuse(err, SLF_ERR_UNSUPPORTED, std::string(c->sel.lattice == SLF_D3Q15 ? "D3Q15" : "D3Q27") +
                                                ": x-face buffers are not implemented on this lattice (D3Q19 only)");
  if (c->sel.lattice != 1 || g.indirect || c->sc.enabled || c->fe.enabled || c->sc3.enabled || !(g.variant & 8))
    return refuse(err, SLF_ERR_UNSUPPORTED, "x-face buffers: D3Q19 single-fluid modules with direct addressing (whole-row kernels) only");
  if (g.wrap[0]) return refuse(err, SLF_ERR_INVALID, "x-face buffers make no sense with x wrapped inside the sweep");
  if (g.lat_nx - 2 > 1024) return refuse(err, SLF_ERR_UNSUPPORTED, "x-face buffers: rows of at most 1024 nodes");
  if ((xf[0] == nullptr) != (xf[2] == nullptr) || (xf[1] == nullptr) != (xf[3] == nullptr))
    return refuse(err, SLF_ERR_INVALID, "a connected face needs both its send and its receive buffer");
  return SLF_OK;
}

// slf_module_set_xface_planes / slf_plan_add_xface_planes: the planes of set `which`, in the order of xface_buffers_check
inline int xface_planes_check(const ModuleConfig* c, int32_t which, const void* const xf[4], std::string* err) {
  if (!c) return refuse(err, SLF_ERR_INVALID, "module is NULL");
  if (which < 0 || which > 2) return refuse(err, SLF_ERR_INVALID, "x-face planes: 0 / 1 = populations of lattice 0 / 1, 2 = densities");
  if (!xf[0] && !xf[1] && !xf[2] && !xf[3]) return SLF_OK;
  const Geometry& g = c->geo;
  if (c->sc3.enabled)
    return refuse(err, SLF_ERR_UNSUPPORTED, "x-face planes: not implemented for simtype = SLF_SIM_SHAN_CHEN_TERNARY (the planes carry two "
                                            "lattices and two density fields); connected x faces go through ghost columns and index lists");
  if (is_lat_lattice(c->sel.lattice))
    return refuse(err, SLF_ERR_UNSUPPORTED, std::string(c->sel.lattice == SLF_D3Q15 ? "D3Q15" : "D3Q27") +
                                                ": x-face planes are not implemented on this lattice (D3Q19 only)");
  if (c->sel.lattice != 1 || g.indirect || !c->sc.enabled || !(g.variant & 8))
    return refuse(err, SLF_ERR_UNSUPPORTED, "x-face planes: D3Q19 Shan-Chen modules with direct addressing (whole-row kernels)");
  if (c->sc.enabled == 2 && which == 1) return refuse(err, SLF_ERR_INVALID, "x-face planes: the single-component model has one lattice");
  if (g.wrap[0]) return refuse(err, SLF_ERR_INVALID, "x-face planes make no sense with x wrapped inside the sweep");
  if (g.lat_nx - 2 > 1024 || g.lat_nx - 2 < 2) return refuse(err, SLF_ERR_UNSUPPORTED, "x-face planes: rows of 2 .. 1024 nodes");
  if ((xf[0] == nullptr) != (xf[2] == nullptr) || (xf[1] == nullptr) != (xf[3] == nullptr))
    return refuse(err, SLF_ERR_INVALID, "a connected face needs both its send and its receive plane");
  return SLF_OK;
}

}  // namespace slf
