// Walks the host logic of the C ABI (sailfish_amd/csrc/slf_bind.h) on the CPU and prints one line per case:
//   section \t subject \t configuration \t try \t code \t message \t detail
// tests/test_abi_bind.py builds it with AddressSanitizer and UBSan, runs it and compares the lines with
// tests/golden/abi_binding.json, tests/golden/abi_support.tsv and tests/golden/abi_launch.tsv.  Nothing here touches a GPU.
#include <stdio.h>

#include <string>
#include <vector>

#include "slf_bind.h"

namespace {

struct Config {
  std::string name;
  slf_module_desc desc;
  slf::ModuleConfig cfg;
  int code;
};

void line(const char* section, const std::string& subject, const std::string& config, const std::string& what, int code,
          const std::string& message, const std::string& detail) {
  printf("%s\t%s\t%s\t%s\t%d\t%s\t%s\n", section, subject.c_str(), config.c_str(), what.c_str(), code, message.c_str(),
         detail.c_str());
}

std::string num(double v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}
template <class T>
std::string list(const T* v, int n) {
  std::string s = "[";
  for (int i = 0; i < n; i++) s += (i ? "," : "") + num((double)v[i]);
  return s + "]";
}

// every field of the structs a module is configured with
std::string dump(const slf::ModuleConfig& c) {
  const slf::Geometry& g = c.geo;
  const slf::Physics& p = c.phys;
  std::string s;
  s += "sel=" + num(c.sel.lattice) + "," + num(c.sel.model) + "," + num(c.sel.precision) + "," + num(c.sel.general);
  s += " access=" + num(c.access_pattern) + " block_x=" + num(c.block_x) + " n_node_params=" + num(c.n_node_params);
  s += " geo: dim=" + num(g.dim) + " lat=" + num(g.lat_nx) + "," + num(g.lat_ny) + "," + num(g.lat_nz) + " arr=" + num(g.arr_nx) +
       "," + num(g.arr_ny) + "," + num(g.arr_nz) + "," + num(g.arr_nxy) + " dist_size=" + num(g.dist_size) + " wrap=" + list(g.wrap, 3) +
       " axis_mode=" + list(g.axis_mode, 3) + " type_mask=" + num(g.type_mask) + " param=" + num(g.param_shift) + "," +
       num(g.param_mask) + " orient_shift=" + num(g.orient_shift) + " type_lut=" + std::to_string(g.type_lut) + " link_tags=" +
       num(g.use_link_tags) + " variant=" + num(g.variant) + " indirect=" + num(g.indirect) + " bc_level=" + num(g.bc_level) +
       " x_ghost_unused=" + num(g.x_ghost_unused);
  s += " phys: tau=" + num(p.tau) + " visc=" + num(p.visc) + " accel=" + list(p.accel, 3) + " mrt=" + list(p.mrt_rates, 27) +
       " incompressible=" + num(p.incompressible) + " has_force=" + num(p.has_force) + " relax=" + num(p.relaxation_enabled) +
       " edm=" + num(p.force_edm) + " regularized=" + num(p.regularized) + " subgrid=" + num(p.subgrid) + "," +
       num(p.smagorinsky_const) + " entropic=" + num(p.entropic_equilibrium) + "," + num(p.entropy_tolerance) + "," +
       num(p.alpha_tolerance) + " tms_mask=" + num(p.tms_mask);
  s += " sc: " + num(c.sc.enabled) + " tau_phi=" + num(c.sc.tau_phi) + " G=" + list(c.sc.G, 4) + " potential=" + num(c.sc.potential) +
       " accel1=" + list(c.sc.accel1, 3);
  s += " fe: " + num(c.fe.enabled) + " " + num(c.fe.Gamma) + "," + num(c.fe.kappa) + "," + num(c.fe.A) + " tau=" + num(c.fe.tau_a) + "," +
       num(c.fe.tau_b) + "," + num(c.fe.tau_phi) + " wall=" + num(c.fe.wall_phase) + "," + num(c.fe.wall_order) + " rim=" + list(c.fe.rim, 3);
  s += " sc3: " + num(c.sc3.enabled) + " tau=" + num(c.sc3.tau_phi) + "," + num(c.sc3.tau_theta) + " G=" + list(c.sc3.G, 9) +
       " potential=" + num(c.sc3.potential) + " accel1=" + list(c.sc3.accel1, 3) + " accel2=" + list(c.sc3.accel2, 3);
  return s;
}

// A valid descriptor: 6 x 5 (x 4) nodes, rows padded to 8; fluid, ghost, unused, propagation-only and full-way bounce-back nodes
slf_module_desc base_desc(int lattice, int access, int simtype, int model, int addressing) {
  static const double params[3] = {0.5, 0.25, 0.125};
  slf_module_desc d = {};
  d.struct_size = sizeof(slf_module_desc);
  d.lattice = lattice; d.model = model; d.precision = 4; d.access_pattern = access;
  d.lat_nx = 6; d.lat_ny = 5; d.lat_nz = lattice == SLF_D2Q9 ? 1 : 4;
  d.arr_nx = 8; d.arr_ny = 5; d.arr_nz = d.lat_nz;
  d.envelope = 1;
  d.relaxation_enabled = 1;
  d.tau = 0.8; d.visc = 0.1;
  d.nt_type_mask = 7; d.nt_misc_shift = 3; d.nt_param_shift = 2; d.nt_scratch_shift = 1;
  d.n_types = 5;
  for (int i = 0; i < 5; i++) d.type_kind[i] = i;
  d.n_node_params = 3; d.node_params = params;
  d.simtype = simtype;
  d.tau_phi = 0.9;
  d.sc_G[0] = 0.1; d.sc_G[1] = 1.2; d.sc_G[2] = 1.2; d.sc_G[3] = 0.2;
  d.node_addressing = addressing;
  d.dist_stride = addressing == SLF_ADDR_INDIRECT ? 100 : 0;
  d.fe_Gamma = 0.5; d.fe_kappa = 0.04; d.fe_A = 0.03; d.fe_tau_a = 0.9; d.fe_tau_b = 0.7;
  d.bc_wall_grad_phase = 0.1; d.bc_wall_grad_order = 1;
  d.tau_theta = 1.1;
  for (int i = 0; i < 9; i++) d.sc3_G[i] = 0.1 * (i + 1);
  d.entropy_tolerance = 1e-6; d.alpha_tolerance = 1e-10;
  if (model == SLF_MRT) for (int i = 0; i < 19; i++) d.mrt_rates[i] = 1.0 + 0.01 * i;
  return d;
}

std::vector<Config> all_configs() {
  std::vector<Config> out;
  auto add = [&out](const std::string& name, const slf_module_desc& d) { out.push_back(Config{name, d, {}, 0}); };
  struct Fam { const char* name; int simtype, model; bool indirect; };
  const Fam fams[] = {{"bgk", SLF_SIM_LBM, SLF_BGK, true}, {"mrt", SLF_SIM_LBM, SLF_MRT, true}, {"elbm", SLF_SIM_LBM, SLF_ELBM, true},
                      {"sc2", SLF_SIM_SHAN_CHEN_BINARY, SLF_BGK, true}, {"scs", SLF_SIM_SHAN_CHEN_SINGLE, SLF_BGK, true},
                      {"fe", SLF_SIM_FREE_ENERGY, SLF_BGK, false}, {"sc3", SLF_SIM_SHAN_CHEN_TERNARY, SLF_BGK, false}};
  for (const Fam& f : fams)
    for (int lattice : {SLF_D2Q9, SLF_D3Q19})
      for (int access : {SLF_AB, SLF_AA})
        for (int addr : {SLF_ADDR_DIRECT, SLF_ADDR_INDIRECT}) {
          if (addr == SLF_ADDR_INDIRECT && !f.indirect) continue;
          add(std::string(f.name) + (lattice == SLF_D2Q9 ? "-d2q9" : "-d3q19") + (access == SLF_AB ? "-ab" : "-aa") +
                  (addr == SLF_ADDR_DIRECT ? "-direct" : "-indirect"), base_desc(lattice, access, f.simtype, f.model, addr));
        }
  // valid modules in which CollideAndPropagateResident does not exist (3-D: above)
  slf_module_desc d = base_desc(SLF_D2Q9, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
  d.regularized = 1; add("resident-regularized", d);
  d = base_desc(SLF_D2Q9, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
  d.incompressible = SLF_DENSITY_ROUNDOFF; add("resident-roundoff", d);
  d = base_desc(SLF_D2Q9, SLF_AA, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
  d.periodic_local[1] = 1; add("resident-ghost-periodic", d);
  d = base_desc(SLF_D2Q9, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
  d.n_types = 6; d.type_kind[5] = SLF_NK_HALF_BB; add("resident-half-bb", d);
  d = base_desc(SLF_D2Q9, SLF_AA, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
  d.periodic_fused[0] = d.periodic_fused[1] = 1; d.fluid_only = 1; d.n_types = 0; d.has_force = 1; d.accel[0] = 1e-5;
  d.force_implementation = SLF_FORCE_EDM; d.sparse_geometry = 1; d.use_link_tags = 1; add("bgk-d2q9-aa-fused-fluid-only", d);
  d = base_desc(SLF_D3Q19, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
  d.n_types = 8; d.type_kind[5] = SLF_NK_WALL_TMS; d.type_kind[6] = SLF_NK_ZOUHE_VELOCITY; d.type_kind[7] = SLF_NK_YU_OUTFLOW;
  d.subgrid = SLF_SUBGRID_LES_SMAGORINSKY; d.smagorinsky_const = 0.1; d.lat_nx = 2000; d.arr_nx = 2048; add("bgk-d3q19-ab-les-tms-long-rows", d);

  // every refusal of the descriptor
  const int B = SLF_BGK, LBM = SLF_SIM_LBM, DIR = SLF_ADDR_DIRECT, IND = SLF_ADDR_INDIRECT;
#define REFUSAL(name, lattice, access, simtype, model, addr, change) \
  d = base_desc(lattice, access, simtype, model, addr);              \
  change;                                                            \
  add("refuse-" name, d);
  REFUSAL("struct-size", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.struct_size -= 4)
  REFUSAL("lattice", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.lattice = 7)
  REFUSAL("model", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.model = 7)
  REFUSAL("precision", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.precision = 2)
  REFUSAL("access", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.access_pattern = 2)
  REFUSAL("envelope", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.envelope = 2)
  REFUSAL("size-small", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.lat_ny = 2)
  REFUSAL("size-2d-nz", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.lat_nz = d.arr_nz = 3)
  REFUSAL("size-3d-nz", SLF_D3Q19, SLF_AB, LBM, B, DIR, d.lat_nz = 2)
  REFUSAL("padding", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.arr_nx = 5)
  REFUSAL("tau", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.tau = 0.5)
  REFUSAL("n-types", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.n_types = 17)
  REFUSAL("n-types-negative", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.n_types = -1)
  REFUSAL("too-large", SLF_D3Q19, SLF_AB, LBM, B, DIR, (d.lat_nx = d.arr_nx = 2048, d.lat_ny = d.arr_ny = 2048, d.lat_nz = d.arr_nz = 1024))
  REFUSAL("stride-too-large", SLF_D3Q19, SLF_AB, LBM, B, DIR, d.dist_stride = 0xFFFFFFFFull)
  REFUSAL("addressing", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.node_addressing = 2)
  REFUSAL("indirect-fluid-only", SLF_D2Q9, SLF_AB, LBM, B, IND, d.fluid_only = 1)
  REFUSAL("indirect-simtype", SLF_D2Q9, SLF_AB, LBM, B, IND, d.simtype = 9)
  REFUSAL("indirect-no-stride", SLF_D2Q9, SLF_AB, LBM, B, IND, d.dist_stride = 0)
  REFUSAL("stride-small", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.dist_stride = 39)
  REFUSAL("node-kind", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.type_kind[2] = 17)
  REFUSAL("node-kind-negative", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.type_kind[2] = -1)
  REFUSAL("copy-aa", SLF_D2Q9, SLF_AA, LBM, B, DIR, d.type_kind[4] = SLF_NK_COPY)
  REFUSAL("yu-outflow-aa", SLF_D3Q19, SLF_AA, LBM, B, DIR, d.type_kind[4] = SLF_NK_YU_OUTFLOW)
  REFUSAL("do-nothing-aa-indirect", SLF_D2Q9, SLF_AA, LBM, B, IND, d.type_kind[4] = SLF_NK_DO_NOTHING)
  REFUSAL("edm-mrt", SLF_D2Q9, SLF_AB, LBM, SLF_MRT, DIR, d.force_implementation = SLF_FORCE_EDM)
  REFUSAL("subgrid-value", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.subgrid = 2)
  REFUSAL("regularized-mrt", SLF_D2Q9, SLF_AB, LBM, SLF_MRT, DIR, d.regularized = 1)
  REFUSAL("regularized-sc2", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_BINARY, B, DIR, d.regularized = 1)
  REFUSAL("subgrid-roundoff", SLF_D2Q9, SLF_AB, LBM, B, DIR, (d.subgrid = 1, d.smagorinsky_const = 0.1, d.incompressible = 2))
  REFUSAL("subgrid-edm", SLF_D2Q9, SLF_AB, LBM, B, DIR, (d.subgrid = 1, d.smagorinsky_const = 0.1, d.force_implementation = 1))
  REFUSAL("subgrid-constant", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.subgrid = 1)
  REFUSAL("tms-fluid-only", SLF_D2Q9, SLF_AB, LBM, B, DIR, (d.type_kind[4] = SLF_NK_WALL_TMS, d.fluid_only = 1))
  REFUSAL("entropic-equilibrium-bgk", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.entropic_equilibrium = 1)
  REFUSAL("elbm-rates", SLF_D2Q9, SLF_AB, LBM, SLF_ELBM, DIR, d.mrt_rates[3] = 1.0)
  REFUSAL("elbm-sc2", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_BINARY, SLF_ELBM, DIR, (void)0)
  REFUSAL("elbm-roundoff", SLF_D2Q9, SLF_AB, LBM, SLF_ELBM, DIR, d.incompressible = 2)
  REFUSAL("elbm-incompressible-entropic", SLF_D2Q9, SLF_AB, LBM, SLF_ELBM, DIR, (d.incompressible = 1, d.entropic_equilibrium = 1))
  REFUSAL("elbm-force", SLF_D2Q9, SLF_AB, LBM, SLF_ELBM, DIR, d.has_force = 1)
  REFUSAL("elbm-entropy-tolerance", SLF_D2Q9, SLF_AB, LBM, SLF_ELBM, DIR, d.entropy_tolerance = 0.0)
  REFUSAL("elbm-alpha-tolerance", SLF_D2Q9, SLF_AB, LBM, SLF_ELBM, DIR, d.alpha_tolerance = -1.0)
  REFUSAL("roundoff-mrt", SLF_D2Q9, SLF_AB, LBM, SLF_MRT, DIR, d.incompressible = 2)
  REFUSAL("roundoff-node-kind", SLF_D2Q9, SLF_AB, LBM, B, DIR, (d.incompressible = 2, d.type_kind[4] = SLF_NK_ZOUHE_VELOCITY))
  REFUSAL("density-model", SLF_D2Q9, SLF_AB, LBM, B, DIR, d.incompressible = 3)
  REFUSAL("sc2-mrt", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_BINARY, SLF_MRT, DIR, (void)0)
  REFUSAL("sc2-tau-phi", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_BINARY, B, DIR, d.tau_phi = 0.5)
  REFUSAL("sc2-node-kind", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_BINARY, B, DIR, d.type_kind[4] = SLF_NK_HALF_BB)
  REFUSAL("scs-node-kind", SLF_D3Q19, SLF_AA, SLF_SIM_SHAN_CHEN_SINGLE, B, DIR, d.type_kind[4] = SLF_NK_EQUILIBRIUM_DENSITY)
  REFUSAL("fe-mrt", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, SLF_MRT, DIR, (void)0)
  REFUSAL("fe-force", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.has_force = 1)
  REFUSAL("fe-accel1", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.accel1[1] = 1e-5)
  REFUSAL("fe-indirect", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, IND, (void)0)
  REFUSAL("fe-incompressible", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.incompressible = 1)
  REFUSAL("fe-tau", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.fe_tau_b = 0.5)
  REFUSAL("fe-wall-order", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.bc_wall_grad_order = 3)
  REFUSAL("fe-rim", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.fe_zero_grad_rim[1] = 3)
  REFUSAL("fe-half-bb", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.type_kind[4] = SLF_NK_HALF_BB)
  REFUSAL("fe-node-kind", SLF_D2Q9, SLF_AB, SLF_SIM_FREE_ENERGY, B, DIR, d.type_kind[4] = SLF_NK_ZOUHE_DENSITY)
  REFUSAL("sc3-mrt", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_TERNARY, SLF_MRT, DIR, (void)0)
  REFUSAL("sc3-indirect", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_TERNARY, B, IND, (void)0)
  REFUSAL("sc3-incompressible", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_TERNARY, B, DIR, d.incompressible = 1)
  REFUSAL("sc3-tau", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_TERNARY, B, DIR, d.tau_theta = 0.5)
  REFUSAL("sc3-potential", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_TERNARY, B, DIR, d.sc_potential = 2)
  REFUSAL("sc3-node-kind", SLF_D2Q9, SLF_AB, SLF_SIM_SHAN_CHEN_TERNARY, B, DIR, d.type_kind[4] = SLF_NK_HALF_BB)
#undef REFUSAL
  return out;
}

// The support matrix: every feature that restricts what a module combines it with (in its served base case) x every
// option that can offend it, one at a time: the `cross` section, which answers with what the support table decides of a module.
std::vector<Config> cross_configs() {
  struct Change { std::string name; void (*apply)(slf_module_desc*); };
  typedef slf_module_desc D;
  const Change features[] = {
    {"d2q9", [](D*) {}}, {"d3q19", [](D* d) { *d = base_desc(SLF_D3Q19, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT); }},
    {"d3q15", [](D* d) { *d = base_desc(SLF_D3Q15, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT); }},
    {"d3q27", [](D* d) { *d = base_desc(SLF_D3Q27, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT); }},
    {"accf-d2q9", [](D* d) { d->accel_field = 1; }},
    {"accf-d3q19", [](D* d) { *d = base_desc(SLF_D3Q19, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT); d->accel_field = 1; }},
    {"sw", [](D* d) { d->equilibrium = SLF_EQ_SHALLOW_WATER; d->gravity = 0.001; }},
    {"sc2", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_BINARY; }}, {"scs", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_SINGLE; }},
    {"fe", [](D* d) { d->simtype = SLF_SIM_FREE_ENERGY; }}, {"sc3", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_TERNARY; }},
    {"roundoff", [](D* d) { d->incompressible = SLF_DENSITY_ROUNDOFF; }}, {"elbm", [](D* d) { d->model = SLF_ELBM; }},
    {"regularized", [](D* d) { d->regularized = 1; }},
    {"subgrid", [](D* d) { d->subgrid = SLF_SUBGRID_LES_SMAGORINSKY; d->smagorinsky_const = 0.1; }},
    {"tms", [](D* d) { d->n_types = 6; d->type_kind[5] = SLF_NK_WALL_TMS; }},
  };
  std::vector<Change> offenders = {
    {"model-bgk", [](D* d) { d->model = SLF_BGK; for (double& r : d->mrt_rates) r = 0.0; }},
    {"model-mrt", [](D* d) { d->model = SLF_MRT; for (int i = 0; i < 19; i++) d->mrt_rates[i] = 1.0 + 0.01 * i; }},
    {"model-elbm", [](D* d) { d->model = SLF_ELBM; for (double& r : d->mrt_rates) r = 0.0; }},
    {"simtype-lbm", [](D* d) { d->simtype = SLF_SIM_LBM; }}, {"simtype-sc2", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_BINARY; }},
    {"simtype-scs", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_SINGLE; }}, {"simtype-fe", [](D* d) { d->simtype = SLF_SIM_FREE_ENERGY; }},
    {"simtype-sc3", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_TERNARY; }},
    {"regularized", [](D* d) { d->regularized = 1; }},
    {"subgrid", [](D* d) { d->subgrid = SLF_SUBGRID_LES_SMAGORINSKY; d->smagorinsky_const = 0.1; }},
    {"density-compressible", [](D* d) { d->incompressible = SLF_DENSITY_COMPRESSIBLE; }},
    {"density-incompressible", [](D* d) { d->incompressible = SLF_DENSITY_INCOMPRESSIBLE; }},
    {"density-roundoff", [](D* d) { d->incompressible = SLF_DENSITY_ROUNDOFF; }},
    {"indirect", [](D* d) { d->node_addressing = SLF_ADDR_INDIRECT; d->dist_stride = 100; d->fluid_only = 0; }},
    {"edm", [](D* d) { d->force_implementation = SLF_FORCE_EDM; }},
    {"force", [](D* d) { d->has_force = 1; d->accel[0] = 1e-5; }},
    {"accel-field", [](D* d) { d->accel_field = 1; }},
    {"shallow-water", [](D* d) { d->equilibrium = SLF_EQ_SHALLOW_WATER; d->gravity = 0.001; }},
    {"entropic-equilibrium", [](D* d) { d->entropic_equilibrium = 1; }},
    {"access-ab", [](D* d) { d->access_pattern = SLF_AB; }}, {"access-aa", [](D* d) { d->access_pattern = SLF_AA; }},
    {"fluid-only", [](D* d) { d->fluid_only = 1; }},
  };
  std::vector<Config> out;
  for (const Change& f : features) {
    for (int o = 0; o < (int)offenders.size() + slf::NK_COUNT; o++) {
      slf_module_desc d = base_desc(SLF_D2Q9, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
      f.apply(&d);
      std::string name;
      if (o < (int)offenders.size()) {
        offenders[o].apply(&d);
        name = offenders[o].name;
      } else {      // one more node type, of each kind
        d.type_kind[d.n_types++] = o - (int)offenders.size();
        name = "node-kind-" + num(o - (int)offenders.size());
      }
      out.push_back(Config{"x-" + f.name + "+" + name, d, {}, 0});
    }
  }
  // malformed fields and double faults: which check answers first decides the code
  const Change malformed[] = {
    {"regularized+density-7", [](D* d) { d->regularized = 1; d->incompressible = 7; }},
    {"elbm+density-negative", [](D* d) { d->model = SLF_ELBM; d->incompressible = -1; }},
    {"d3q15+density-7", [](D* d) { *d = base_desc(SLF_D3Q15, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT); d->incompressible = 7; }},
    {"accf+density-7", [](D* d) { d->accel_field = 1; d->incompressible = 7; }},
    {"sw+density-7", [](D* d) { d->equilibrium = SLF_EQ_SHALLOW_WATER; d->gravity = 0.001; d->incompressible = 7; }},
    {"sw+addressing-5", [](D* d) { d->equilibrium = SLF_EQ_SHALLOW_WATER; d->gravity = 0.001; d->node_addressing = 5; }},
    {"sw+model-7", [](D* d) { d->equilibrium = SLF_EQ_SHALLOW_WATER; d->gravity = 0.001; d->model = 7; }},
    {"sw+mrt+accel-field-2", [](D* d) { d->equilibrium = SLF_EQ_SHALLOW_WATER; d->gravity = 0.001; d->model = SLF_MRT; d->accel_field = 2; }},
    {"accf+model-7", [](D* d) { d->accel_field = 1; d->model = 7; }},
    {"fe+addressing-5", [](D* d) { d->simtype = SLF_SIM_FREE_ENERGY; d->node_addressing = 5; }},
    {"sc3+addressing-5", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_TERNARY; d->node_addressing = 5; }},
    {"fe+indirect+fluid-only", [](D* d) { d->simtype = SLF_SIM_FREE_ENERGY; d->node_addressing = SLF_ADDR_INDIRECT; d->dist_stride = 100; d->fluid_only = 1; }},
    {"fe+density-7", [](D* d) { d->simtype = SLF_SIM_FREE_ENERGY; d->incompressible = 7; }},
    {"sc2+mrt+tau", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_BINARY; d->model = SLF_MRT; d->tau = 0.4; }},
    {"sc2+mrt+tau-phi", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_BINARY; d->model = SLF_MRT; d->tau_phi = 0.4; }},
    {"sc2+node-kind+tau-phi", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_BINARY; d->type_kind[4] = SLF_NK_HALF_BB; d->tau_phi = 0.4; }},
    {"sc2+node-kind+entropic", [](D* d) { d->simtype = SLF_SIM_SHAN_CHEN_BINARY; d->type_kind[4] = SLF_NK_HALF_BB; d->entropic_equilibrium = 1; }},
    {"elbm+force+size", [](D* d) { d->model = SLF_ELBM; d->has_force = 1; d->lat_nx = 1; }},
    {"elbm+force+precision", [](D* d) { d->model = SLF_ELBM; d->has_force = 1; d->precision = 2; }},
    {"regularized+mrt+subgrid-9", [](D* d) { d->regularized = 1; d->model = SLF_MRT; d->subgrid = 9; }},
    {"regularized+simtype-9", [](D* d) { d->regularized = 1; d->simtype = 9; }},
    {"roundoff+zouhe+entropic", [](D* d) { d->incompressible = SLF_DENSITY_ROUNDOFF; d->type_kind[4] = SLF_NK_ZOUHE_VELOCITY; d->entropic_equilibrium = 1; }},
    {"tms+simtype-9", [](D* d) { d->n_types = 6; d->type_kind[5] = SLF_NK_WALL_TMS; d->simtype = 9; }},
    {"tms+sc2+entropic", [](D* d) { d->n_types = 6; d->type_kind[5] = SLF_NK_WALL_TMS; d->simtype = SLF_SIM_SHAN_CHEN_BINARY; d->entropic_equilibrium = 1; }},
    {"d3q27+node-kind-20", [](D* d) { *d = base_desc(SLF_D3Q27, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT); d->type_kind[4] = 20; }},
    {"d3q15+mrt+access-2", [](D* d) { *d = base_desc(SLF_D3Q15, SLF_AB, SLF_SIM_LBM, SLF_MRT, SLF_ADDR_DIRECT); d->access_pattern = 2; }},
  };
  for (const Change& m : malformed) {
    slf_module_desc d = base_desc(SLF_D2Q9, SLF_AB, SLF_SIM_LBM, SLF_BGK, SLF_ADDR_DIRECT);
    m.apply(&d);
    out.push_back(Config{"m-" + m.name, d, {}, 0});
  }
  return out;
}

// ---- binding ---------------------------------------------------------------------------------------------------------
struct Call {
  std::string fmt;
  int argc;
};

std::string arg_of(const void* p) {          // pointer argument i carries 0x1000 * (i + 1)
  const unsigned long long v = (unsigned long long)p;
  return v ? std::to_string(v / 0x1000 - 1) : "-";
}

std::string dump(const slf::BoundArgs& b) {
  const slf::SweepArgs& a = b.sweep;
  const slf::Sc3Args& t = b.sc3;
  std::string s = "sweep: nodes=" + arg_of(a.nodes) + " map=" + arg_of(a.map) + " dist_in=" + arg_of(a.dist_in) + " dist_out=" +
                  arg_of(a.dist_out) + " dist_in2=" + arg_of(a.dist_in2) + " dist_out2=" + arg_of(a.dist_out2) + " rho=" + arg_of(a.rho) +
                  " phi=" + arg_of(a.phi) + " v=" + arg_of(a.v[0]) + "," + arg_of(a.v[1]) + "," + arg_of(a.v[2]) + " alpha=" +
                  arg_of(a.alpha) + " lap=" + arg_of(a.lap) + " options=" + num(a.options) + " local_velocity=" + num(a.sc_local_velocity);
  s += " sc3: map=" + arg_of(t.map);
  for (int l = 0; l < 3; l++) s += " in" + num(l) + "=" + arg_of(t.dist_in[l]) + " out" + num(l) + "=" + arg_of(t.dist_out[l]);
  s += " field=" + arg_of(t.field[0]) + "," + arg_of(t.field[1]) + "," + arg_of(t.field[2]) + " v=" + arg_of(t.v[0]) + "," +
       arg_of(t.v[1]) + "," + arg_of(t.v[2]) + " options=" + num(t.options);
  s += " ptrs=[";
  for (int i = 0; i < b.n_ptrs && i < slf::MAX_BOUND_PTRS; i++) s += (i ? "," : "") + arg_of((const void*)b.ptrs[i]);
  s += "] ints=" + list(b.ints, b.n_ints < slf::MAX_BOUND_INTS ? b.n_ints : slf::MAX_BOUND_INTS) + " n=" + num(b.n_ptrs) + "," + num(b.n_ints) +
       " alpha_arg=" + num(b.alpha_arg) + " build_slots=" + num(b.build_slots);
  return s;
}

// the argument list the table holds for this name and kind
const slf::KernelRow* signature_of(const char* name, slf::KernelKind kind) {
  for (const slf::KernelRow& r : slf::KERNEL_TABLE)
    if (!strcmp(r.name, name) && r.kind == kind) return &r;
  return nullptr;
}

std::vector<std::pair<std::string, Call>> calls_for(const slf::ModuleConfig& c, const slf::KernelRow& sig) {
  const int dim = c.geo.dim;
  std::string exact;
  if (slf::is_face_kind(sig.kind)) {
    exact = dim == 3 ? "PiiiiiP" : "PiiiP";
  } else {
    if (c.geo.indirect && sig.nodes_in_front) exact += 'P';
    for (const char* s = sig.slots; *s; s++) exact += std::string(*s == 'v' ? dim : 1, 'P');
    exact += std::string(sig.n_ints == slf::BOX_INTS ? 6 : sig.n_ints, 'i');
  }
  const int n = (int)exact.size();
  std::vector<std::pair<std::string, Call>> calls;
  calls.push_back({"exact", {exact, n}});
  std::string s = exact;
  s.erase(s.rfind('P'), 1);
  calls.push_back({"pointer-fewer", {s, n - 1}});
  calls.push_back({"pointer-more", {exact + "P", n + 1}});            // entropic CollideAndPropagate: the alpha field
  calls.push_back({"two-pointers-more", {exact + "PP", n + 2}});
  calls.push_back({"int-more", {exact + "i", n + 1}});
  s = exact;
  s[0] = 'f';
  calls.push_back({"bad-format-char", {s, n}});
  calls.push_back({"argc-short", {exact, n - 1}});
  std::string ints_first, ptrs_last;
  for (char ch : exact) (ch == 'i' ? ints_first : ptrs_last) += ch;
  calls.push_back({"ints-first", {ints_first + ptrs_last, n}});
  calls.push_back({"pointers-first", {ptrs_last + ints_first, n}});
  calls.push_back({"thirty-pointers", {std::string(30, 'P'), 30}});
  if (slf::is_box_kind(sig.kind)) {
    calls.push_back({"box-8-ints", {"PPiiiiiiii", 10}});
    calls.push_back({"box-7-ints", {"PPiiiiiii", 9}});
    calls.push_back({"box-reference-form", {dim == 3 ? "PiiiiiP" : "PiiiP", dim == 3 ? 7 : 5}});
    calls.push_back({"box-reference-form-buffer-second", {dim == 3 ? "PPiiiii" : "PPiii", dim == 3 ? 7 : 5}});
    calls.push_back({"box-reference-form-of-the-other-dimension", {dim == 3 ? "PiiiP" : "PiiiiiP", dim == 3 ? 5 : 7}});
  }
  return calls;
}

// ---- face box --------------------------------------------------------------------------------------------------------
void face_boxes(const slf::ModuleConfig& c2, const slf::ModuleConfig& c3) {
  const slf::KernelKind kinds[] = {slf::KK_COLLECT_BOX, slf::KK_DISTRIBUTE_BOX, slf::KK_COLLECT_FACE_SWAP, slf::KK_DISTRIBUTE_FACE_SWAP,
                                   slf::KK_COLLECT_MACRO_FACE, slf::KK_DISTRIBUTE_MACRO_FACE};
  for (const slf::ModuleConfig* c : {&c2, &c3}) {
    const int dim = c->geo.dim;
    for (slf::KernelKind kind : kinds) {
      const bool macro = kind == slf::KK_COLLECT_MACRO_FACE || kind == slf::KK_DISTRIBUTE_MACRO_FACE;
      struct Try { std::string name; long long ints[5]; };
      std::vector<Try> tries;
      for (int face = 1; face <= 6; face++) {
        if (dim == 3) tries.push_back({"face" + num(face), {face, 1, 1, 4, macro ? 2 : 10}});
        else if (macro) tries.push_back({"layer" + num(face - 2), {1, 4, face - 2, 0, 0}});      // 2-D macro: (base_gx, max_lx, gy)
        else tries.push_back({"face" + num(face), {face, 1, 12, 0, 0}});
      }
      if (dim == 3) {
        tries.push_back({"max-other-7", {2, 1, 1, 4, 7}});
        tries.push_back({"base-gx-6", {2, 6, 1, 4, macro ? 2 : 10}});
        tries.push_back({"base-gx-negative", {4, -1, 1, 4, macro ? 2 : 10}});
        tries.push_back({"base-other-3", {5, 1, 3, 4, macro ? 2 : 10}});
        tries.push_back({"whole-face", {3, 0, 0, 8, macro ? 4 : 20}});
      } else if (macro) {
        tries.push_back({"layer-5", {1, 4, 5, 0, 0}});
        tries.push_back({"base-gx-6", {6, 4, 2, 0, 0}});
      } else {
        tries.push_back({"max-lx-7", {2, 1, 7, 0, 0}});
        tries.push_back({"base-gx-6", {3, 6, 12, 0, 0}});
        tries.push_back({"whole-face", {2, 0, 24, 0, 0}});
      }
      for (const Try& t : tries) {
        slf::FaceBox box = {};
        const char* err = "";
        const int rc = slf::face_box(c->geo, kind, t.ints, &box, &err);
        std::string detail;
        if (!rc)
          detail = "collect=" + num(box.collect) + " macro=" + num(box.macro) + " layer=" + num(box.layer) + " dirs=" +
                   list(box.dirs, box.nd) + " base=" + std::to_string(box.base) + " row_stride=" + std::to_string(box.row_stride) +
                   " ncols=" + num(box.ncols) + " nrows=" + num(box.nrows);
        line("face", "kind" + num(kind), dim == 2 ? "d2q9" : "d3q19", t.name, rc, err, detail);
      }
    }
  }
}

// ---- launch-time checks and the setters' argument checks (slf_bind.h part (f)) ---------------------------------------------
struct Answer {
  int code;
  std::string message, detail;
};

// what the launch would hand to launch_box
std::string dump_box(bool collect, const int* dirs, int nd, unsigned long long base, long long col_stride, int ncols, long long row_stride,
                     int nrows, long long buf_k_stride, long long buf_row_stride, bool deliver_all) {
  return "collect=" + num(collect) + " dirs=" + list(dirs, nd) + " base=" + std::to_string(base) + " col_stride=" + std::to_string(col_stride) +
         " ncols=" + num(ncols) + " row_stride=" + std::to_string(row_stride) + " nrows=" + num(nrows) + " buf_strides=" +
         std::to_string(buf_k_stride) + "," + std::to_string(buf_row_stride) + " deliver_all=" + num(deliver_all);
}

// the kinds whose launch takes a propagation step and rows (this program's own list, not the table's column)
bool takes_rows(slf::KernelKind kk) {
  switch (kk) {
    case slf::KK_COLLIDE_AND_PROPAGATE: case slf::KK_COMPUTE_MACRO: case slf::KK_SC_MACRO: case slf::KK_SC_SWEEP0: case slf::KK_SC_SWEEP1:
    case slf::KK_SC_FUSED: case slf::KK_SCS_MACRO: case slf::KK_SCS_SWEEP: case slf::KK_FE_MACRO: case slf::KK_FE_FLUID: case slf::KK_FE_ORDER:
    case slf::KK_SC3_MACRO: case slf::KK_SC3_SWEEP0: case slf::KK_SC3_SWEEP1: case slf::KK_SC3_SWEEP2: case slf::KK_SC3_FUSED: return true;
    default: return false;
  }
}
bool whole_box_kind(slf::KernelKind kk) { return kk == slf::KK_COMPUTE_MACRO || kk == slf::KK_SCS_MACRO; }

// ---- the functions under test, each answering with (code, message, what the launch would use) ----
struct State {
  int needs_iteration;
  uint32_t iteration;
  bool has_field, pair_armed;
};

Answer launch_answer(const slf::ModuleConfig& c, const slf::KernelRow& row, const slf::BoundArgs& b, const State& st, const slf_region* region) {
  slf::LaunchShape sh = {};
  slf::FaceBox box = {};
  std::string err;
  const slf::LaunchState state = {st.needs_iteration, st.iteration, st.has_field, st.pair_armed};
  const int rc = slf::launch_check(c, row, b, state, region, &sh, &box, &err);
  if (rc) return {rc, err, ""};
  const slf::KernelKind kk = row.kind;
  if (st.pair_armed && (kk == slf::KK_COLLIDE_AND_PROPAGATE || kk == slf::KK_COMPUTE_MACRO)) return {0, "", "pair"};
  if (takes_rows(kk)) return {0, "", "prop=" + num(sh.prop) + " rows=" + num(sh.y0) + "," + num(sh.y1) + "," + num(sh.z0) + "," + num(sh.z1)};
  if (slf::is_box_kind(kk) || slf::is_face_kind(kk))
    return {0, "", dump_box(box.collect, box.dirs, box.nd, box.base, box.col_stride, box.ncols, box.row_stride, box.nrows, box.buf_k_stride,
                            box.buf_row_stride, box.macro)};
  return {0, "", ""};
}
Answer resident_answer(const slf::ModuleConfig& c, const slf::BoundArgs& b, int needs_iteration) {
  std::string err;
  const int rc = slf::resident_check(c, b, needs_iteration, &err);
  return {rc, err, ""};
}
Answer xface_buffers_answer(const slf::ModuleConfig* c, const void* const xf[4]) {
  std::string err;
  const int rc = slf::xface_buffers_check(c, xf, &err);
  return {rc, err, ""};
}
Answer xface_planes_answer(const slf::ModuleConfig* c, int which, const void* const xf[4]) {
  std::string err;
  const int rc = slf::xface_planes_check(c, which, xf, &err);
  return {rc, err, ""};
}
// ---- end of the functions under test ----

// the arguments `fmt` binds: pointer i is 0x1000 * (i + 1), integer i is 100 + i
int bind_call(const slf::ModuleConfig& c, const slf::KernelRow& row, const std::string& fmt, slf::BoundArgs* bound) {
  std::vector<unsigned long long> pv(fmt.size() + 1);
  std::vector<int32_t> iv(fmt.size() + 1);
  std::vector<const void*> argv(fmt.size() + 1);
  for (size_t i = 0; i < fmt.size(); i++) {
    pv[i] = 0x1000ull * (i + 1);
    iv[i] = 100 + (int)i;
    argv[i] = fmt[i] == 'i' ? (const void*)&iv[i] : (const void*)&pv[i];
  }
  std::string err;
  return slf::bind(c, row, fmt.c_str(), argv.data(), (int)fmt.size(), bound, &err);
}

void launch_sections(const std::vector<Config>& configs) {
  // the modules: a 2-D and a 3-D one of every family, both access patterns and both addressings among them (the collision
  // model is nothing a launch asks about), then those the launch rules single out
  std::vector<Config> mods;
  for (const char* name : {"bgk-d2q9-ab-direct", "bgk-d2q9-aa-direct", "bgk-d3q19-ab-direct", "bgk-d3q19-aa-direct", "bgk-d3q19-ab-indirect",
                           "sc2-d2q9-ab-direct", "sc2-d3q19-aa-direct", "sc2-d3q19-ab-indirect", "scs-d2q9-aa-direct", "scs-d3q19-ab-direct", "scs-d3q19-aa-indirect",
                           "fe-d2q9-aa-direct", "fe-d3q19-ab-direct", "sc3-d2q9-ab-direct", "sc3-d3q19-aa-direct"})
    for (const Config& cc : configs)
      if (cc.name == name && !cc.code) mods.push_back(cc);
  auto add = [&mods](const std::string& name, slf_module_desc d) {
    Config c{name, d, {}, 0};
    const char* err = "";
    c.code = slf::module_config(&c.desc, &c.cfg, &err);
    if (c.code) line("launch", "-", name, "module", c.code, err, "");
    else mods.push_back(c);
  };
  const int DIR = SLF_ADDR_DIRECT;
  slf_module_desc d = base_desc(SLF_D2Q9, SLF_AB, SLF_SIM_LBM, SLF_BGK, DIR);
  d.accel_field = 1; add("accf-d2q9-ab-direct", d);
  d = base_desc(SLF_D3Q19, SLF_AA, SLF_SIM_LBM, SLF_BGK, DIR);
  d.accel_field = 1; add("accf-d3q19-aa-direct", d);
  add("d3q15-ab-direct", base_desc(SLF_D3Q15, SLF_AB, SLF_SIM_LBM, SLF_BGK, DIR));
  struct Fam { const char* name; int simtype; };
  for (const Fam& f : {Fam{"bgk", SLF_SIM_LBM}, Fam{"sc3", SLF_SIM_SHAN_CHEN_TERNARY}}) {      // the two map rules
    d = base_desc(SLF_D3Q19, SLF_AB, f.simtype, SLF_BGK, DIR);
    d.fluid_only = 1; d.n_types = 0;
    add(std::string(f.name) + "-d3q19-ab-fluid-only", d);
  }

  std::vector<std::string> names;
  for (const slf::KernelRow& r : slf::KERNEL_TABLE) {
    bool seen = false;
    for (const std::string& n : names) seen = seen || n == r.name;
    if (!seen) names.push_back(r.name);
  }
  for (const Config& cc : mods) {
    const slf::ModuleConfig& c = cc.cfg;
    const slf::Geometry& g = c.geo;
    const bool d3 = g.dim == 3, aa = c.access_pattern == SLF_AA;
    const bool halo = cc.name == "bgk-d3q19-aa-direct" || cc.name == "bgk-d2q9-ab-direct";      // the modules that show the halo kinds
    for (const std::string& name : names) {
      const slf::KernelRow* row = nullptr;
      std::string err;
      if (slf::resolve(c, name.c_str(), &row, &err)) continue;
      const slf::KernelKind kk = row->kind;
      if (kk == slf::KK_RESIDENT) continue;      // its launch asks for the map alone: the `resident` section
      if (row->families == slf::F_ALL && !halo) continue;
      // the region at each edge: one sweep per family, in a module with direct addressing
      const bool edges = !g.indirect && c.sel.general && !c.phys.accel_field &&
                         (kk == slf::KK_COLLIDE_AND_PROPAGATE || kk == slf::KK_SC_SWEEP1 || kk == slf::KK_SCS_SWEEP || kk == slf::KK_FE_ORDER || kk == slf::KK_SC3_FUSED);
      const slf::KernelRow* sig = signature_of(name.c_str(), kk);
      slf::BoundArgs bound = {};
      if (bind_call(c, *row, calls_for(c, *sig)[0].second.fmt, &bound)) continue;      // (indirect addressing has no fused binary sweep)
      if (slf::is_face_kind(kk) || slf::is_box_kind(kk)) {      // a face the module has
        const bool macro = kk == slf::KK_COLLECT_MACRO_FACE || kk == slf::KK_DISTRIBUTE_MACRO_FACE;
        const long long f3[5] = {2, 1, 1, 4, macro ? 2 : 10}, f2[5] = {2, 1, 10, 0, 0}, m2[5] = {1, 4, 2, 0, 0};
        if (slf::is_face_kind(kk))
          for (int i = 0; i < 5; i++) bound.ints[i] = d3 ? f3[i] : (macro ? m2[i] : f2[i]);
      }
      struct Try {
        std::string name;
        slf::BoundArgs b;
        State st;
        bool has_region;
        slf_region region;
      };
      const State plain = {1, 0, true, false};
      const slf_region inner = {2, 3, 2, 3};
      std::vector<Try> tries;
      tries.push_back({"no-region", bound, plain, false, inner});
      if (whole_box_kind(kk) || (!takes_rows(kk) && halo)) tries.push_back({"region-out-of-range", bound, plain, true, {-5, 400, -7, 900}});
      if (edges) {
        tries.push_back({"inner-region", bound, plain, true, inner});
        tries.push_back({"y0-0", bound, plain, true, {0, 3, 1, 2}});
        tries.push_back({"y1-lat-ny", bound, plain, true, {1, g.lat_ny, 1, 2}});
        tries.push_back({"y0-above-y1", bound, plain, true, {3, 2, 1, 2}});
        tries.push_back({"y0-equals-y1", bound, plain, true, {2, 2, 1, 2}});
        tries.push_back({"all-rows", bound, plain, true, {1, g.lat_ny - 1, 1, d3 ? g.lat_nz - 1 : 1}});
        tries.push_back({"z-far-out", bound, plain, true, {1, 2, -40, 900}});         // (2-D: z is not read)
        if (d3) {
          tries.push_back({"z0-0", bound, plain, true, {1, 2, 0, 2}});
          tries.push_back({"z1-lat-nz", bound, plain, true, {1, 2, 1, g.lat_nz}});
          tries.push_back({"z0-above-z1", bound, plain, true, {1, 2, 3, 2}});
          tries.push_back({"z0-equals-z1", bound, plain, true, {1, 2, 2, 2}});
        }
      }
      if (aa) tries.push_back({"no-iteration", bound, {0, 7, true, false}, false, inner});
      if (aa && takes_rows(kk)) {
        tries.push_back({"iteration-odd", bound, {1, 7, true, false}, false, inner});
        tries.push_back({"iteration-even", bound, {1, 8, true, false}, !whole_box_kind(kk), inner});
      }
      if (aa && edges) tries.push_back({"no-iteration-region-out", bound, {0, 0, true, false}, true, {0, 900, 0, 900}});
      slf::BoundArgs nomap = bound, nonodes = bound, neither = bound;
      nomap.sweep.map = nomap.sc3.map = nullptr;
      nonodes.sweep.nodes = nullptr;
      neither.sweep.map = neither.sc3.map = neither.sweep.nodes = nullptr;
      tries.push_back({"null-map", nomap, plain, false, inner});
      if (edges) tries.push_back({"null-map-region-out", nomap, plain, true, {0, 900, 0, 900}});
      if (aa && edges) tries.push_back({"null-map-no-iteration", nomap, {0, 0, true, false}, false, inner});
      if (g.indirect) {
        tries.push_back({"null-nodes", nonodes, plain, false, inner});
        tries.push_back({"null-nodes-null-map", neither, plain, false, inner});
        tries.push_back({"null-nodes-region-out", nonodes, plain, true, {0, 900, 0, 900}});
      }
      if (c.phys.accel_field) {
        tries.push_back({"no-field", bound, {1, 0, false, false}, false, inner});
        tries.push_back({"no-field-null-map", nomap, {1, 0, false, false}, false, inner});
        tries.push_back({"no-field-region-out", bound, {1, 0, false, false}, true, {0, 900, 0, 900}});
      }
      if (cc.name == "bgk-d3q19-ab-direct" || cc.name == "bgk-d3q19-ab-fluid-only") {      // (only CollideAndPropagate kernels are ever armed)
        tries.push_back({"pair-armed", bound, {1, 0, true, true}, false, inner});
        tries.push_back({"pair-armed-region", bound, {1, 0, true, true}, true, inner});
        tries.push_back({"pair-armed-region-null-map-no-field", nomap, {0, 0, false, true}, true, {0, 900, 0, 900}});
        tries.push_back({"pair-armed-null-map-no-field", nomap, {0, 0, false, true}, false, inner});
      }
      if (slf::is_box_kind(kk)) {
        for (const char* fmt : {"PPiiiiii", "PPiiiiiiii"}) {
          slf::BoundArgs bx = {};
          if (bind_call(c, *row, fmt, &bx)) continue;
          const std::string form = std::string(fmt).size() == 8 ? "box-6-ints" : "box-8-ints";
          for (long long mask : {0ll, 0xFFFll, 0x1FFFll, 0xFFF00000ll, (long long)(int32_t)0x80000000u, -1ll}) {
            bx.ints[0] = mask;
            char hex[32];
            snprintf(hex, sizeof hex, "%llx", (unsigned long long)mask & 0xFFFFFFFFull);
            tries.push_back({form + "-mask-" + hex, bx, plain, false, inner});
          }
          bx.ints[0] = 0x1FFF; bx.ints[1] = -1;
          tries.push_back({form + "-13-dirs-negative-base", bx, plain, false, inner});
        }
        slf::BoundArgs ref = {};
        if (!bind_call(c, *row, d3 ? "PiiiiiP" : "PiiiP", &ref)) {
          const long long f3[5] = {3, 1, 1, 4, 10}, f2[5] = {3, 1, 10, 0, 0};
          for (int i = 0; i < 5; i++) ref.ints[i] = d3 ? f3[i] : f2[i];
          tries.push_back({"reference-form", ref, plain, false, inner});
          ref.ints[0] = 1;
          tries.push_back({"reference-form-x-face", ref, plain, false, inner});
          ref.ints[0] = 2; ref.ints[1] = 7;
          tries.push_back({"reference-form-outside", ref, plain, true, inner});
        }
      }
      if (slf::is_face_kind(kk)) {
        slf::BoundArgs bad = bound;
        bad.ints[d3 ? 1 : 0] = 7;
        tries.push_back({"face-outside", bad, plain, false, inner});
        bad = bound;
        bad.ints[d3 ? 4 : (kk == slf::KK_COLLECT_MACRO_FACE || kk == slf::KK_DISTRIBUTE_MACRO_FACE ? 1 : 2)] = 7;
        tries.push_back({"face-count-7", bad, plain, false, inner});
      }
      for (const Try& t : tries) {
        const Answer a = launch_answer(c, *row, t.b, t.st, t.has_region ? &t.region : nullptr);
        line("launch", name, cc.name, t.name, a.code, a.message, a.detail);
      }
    }
  }

  // CollideAndPropagateResident: the arguments at bind time (one line per return of the check) and the map at launch time
  for (const Config& cc : mods) {
    const slf::ModuleConfig& c = cc.cfg;
    const slf::KernelRow* row = nullptr;
    std::string err;
    if (slf::resolve(c, "CollideAndPropagateResident", &row, &err)) continue;
    slf::BoundArgs bound = {};
    if (bind_call(c, *row, "PPPPPiiiii", &bound)) continue;
    struct Try { std::string name; long long steps, tx, ty, halo; int needs_iteration; int change; };
    const Try tries[] = {
      {"fits", 2, 16, 8, 4, 1, 0}, {"no-iteration", 2, 16, 8, 4, 0, 0}, {"steps-0", 0, 16, 8, 4, 1, 0}, {"tile-x-0", 2, 0, 8, 4, 1, 0},
      {"tile-y-negative", 2, 16, -8, 4, 1, 0}, {"halo-0", 2, 16, 8, 0, 1, 0}, {"no-source", 2, 16, 8, 4, 1, 1}, {"no-destination", 2, 16, 8, 4, 1, 2},
      {"no-source-b", 2, 16, 8, 4, 1, 3}, {"no-destination-b", 2, 16, 8, 4, 1, 4}, {"same-buffer", 2, 16, 8, 4, 1, 5}, {"same-buffer-b", 2, 16, 8, 4, 1, 6},
      {"halo-1-steps-1", 1, 16, 8, 1, 1, 0}, {"halo-2-steps-1", 1, 16, 8, 2, 1, 0}, {"halo-2-steps-2", 2, 16, 8, 2, 1, 0}, {"halo-3-steps-2", 2, 16, 8, 3, 1, 0},
      {"halo-3-steps-4", 4, 16, 8, 3, 1, 0}, {"halo-4-steps-4", 4, 16, 8, 4, 1, 0}, {"halo-5-steps-4", 4, 16, 8, 5, 1, 0},
      {"window-2048", 1, 60, 28, 2, 1, 0}, {"window-2112", 1, 62, 28, 2, 1, 0}, {"window-46x44", 1, 42, 40, 2, 1, 0}, {"window-huge", 1, 1 << 30, 1 << 30, 2, 1, 0},
      {"no-iteration-steps-0-no-source", 0, 16, 8, 4, 0, 1}, {"steps-0-no-source", 0, 16, 8, 4, 1, 1}, {"no-source-halo-small", 4, 16, 8, 1, 1, 1},
      {"same-buffer-halo-small", 4, 16, 8, 1, 1, 5}, {"halo-small-window-large", 40, 60, 60, 2, 1, 0},
    };
    for (const Try& t : tries) {
      slf::BoundArgs b = bound;
      b.ints[1] = t.steps; b.ints[2] = t.tx; b.ints[3] = t.ty; b.ints[4] = t.halo;
      if (t.change == 1) b.sweep.dist_in = nullptr;
      if (t.change == 2) b.sweep.dist_out = nullptr;
      if (t.change == 3) b.sweep.dist_in2 = nullptr;
      if (t.change == 4) b.sweep.dist_out2 = nullptr;
      if (t.change == 5) b.sweep.dist_out = b.sweep.dist_in;
      if (t.change == 6) b.sweep.dist_out2 = b.sweep.dist_in2;
      const Answer a = resident_answer(c, b, t.needs_iteration);
      line("resident", "args", cc.name, t.name, a.code, a.message, a.detail);
    }
    slf::BoundArgs nomap = bound;
    nomap.sweep.map = nullptr;
    const slf_region out = {0, 900, 0, 900};
    for (int needs_iteration : {0, 1}) {
      const State st = {needs_iteration, 3, false, false};
      Answer a = launch_answer(c, *row, bound, st, &out);
      line("resident", "launch", cc.name, "iteration-flag-" + num(needs_iteration), a.code, a.message, a.detail);
      a = launch_answer(c, *row, nomap, st, nullptr);
      line("resident", "launch", cc.name, "null-map-iteration-flag-" + num(needs_iteration), a.code, a.message, a.detail);
    }
  }

  // the x-face setters: buffers (single fluid) and planes (Shan-Chen), per module and per combination of the four pointers
  for (int mi = -1; mi < (int)mods.size(); mi++) {
    if (mi >= 0 && mods[mi].cfg.geo.dim == 2 && mods[mi].name != "sc2-d2q9-ab-direct" && mods[mi].name != "bgk-d2q9-ab-direct") continue;
    if (mi >= 0 && (mods[mi].cfg.phys.accel_field || !mods[mi].cfg.sel.general)) continue;
    const slf::ModuleConfig* c = mi < 0 ? nullptr : &mods[mi].cfg;
    std::vector<std::pair<std::string, slf::ModuleConfig>> variants;
    if (c) {
      variants.push_back({mods[mi].name, *c});
      if (mods[mi].name == "bgk-d3q19-ab-direct" || mods[mi].name == "scs-d3q19-ab-direct") {      // one that takes buffers, one that takes planes
        slf::ModuleConfig v = *c;
        v.geo.wrap[0] = 1; variants.push_back({mods[mi].name + "+x-wrapped", v});
        v = *c; v.geo.lat_nx = 1027; variants.push_back({mods[mi].name + "+rows-1025", v});
        v = *c; v.geo.lat_nx = 1026; variants.push_back({mods[mi].name + "+rows-1024", v});
        v = *c; v.geo.lat_nx = 3; variants.push_back({mods[mi].name + "+rows-1", v});
        v = *c; v.geo.lat_nx = 4; variants.push_back({mods[mi].name + "+rows-2", v});
        v = *c; v.geo.variant &= ~8; variants.push_back({mods[mi].name + "+no-whole-rows", v});
        v = *c; v.geo.wrap[0] = 1; v.geo.lat_nx = 1027; variants.push_back({mods[mi].name + "+wrapped-1025", v});
      }
    } else {
      variants.push_back({"null-module", slf::ModuleConfig{}});
    }
    for (const auto& v : variants) {
      const slf::ModuleConfig* vc = c ? &v.second : nullptr;
      const bool base = c && v.first == mods[mi].name && !c->geo.indirect && c->geo.dim == 3 && !c->fe.enabled && !c->sc3.enabled;
      for (int bits : {0, 1, 4, 5, 10, 15}) {
        if (!base && bits != 5 && bits != 0) continue;      // every pointer set where they can be accepted, else nothing and one face
        const void* xf[4];
        std::string what;
        for (int i = 0; i < 4; i++) {
          xf[i] = ((bits >> i) & 1) ? (const void*)(0x1000ull * (i + 1)) : nullptr;
          what += ((bits >> i) & 1) ? "SsRr"[i] : '-';      // S / s: send low / high, R / r: receive low / high
        }
        Answer a = xface_buffers_answer(vc, xf);
        if (base || bits == 5) line("xface-buffers", "-", v.first, what, a.code, a.message, a.detail);
        for (int which = -1; which <= 3; which++) {
          if ((which < 0 || which > 2) && (bits != 5 || !(base || !c))) continue;      // no such set: with one face
          if (!base && (bits == 0) != (which == 2)) continue;                         // ... set 2 with nothing, sets 0 and 1 with one face
          a = xface_planes_answer(vc, which, xf);
          line("xface-planes", "set" + num(which), v.first, what, a.code, a.message, a.detail);
        }
      }
    }
  }
}

}  // namespace

int main() {
  for (const char* knob : {"SLF_BC_LEVEL", "SLF_VARIANT", "SLF_BLOCK_X"}) unsetenv(knob);
  std::vector<Config> configs = all_configs();
  for (Config& c : configs) {
    const char* err = "";
    c.code = slf::module_config(&c.desc, &c.cfg, &err);
    line("config", "-", c.name, "-", c.code, err, c.code ? "" : dump(c.cfg));
  }
  for (Config& c : cross_configs()) {
    const char* err = "";
    c.code = slf::module_config(&c.desc, &c.cfg, &err);
    line("cross", "-", c.name, "-", c.code, err,
         c.code ? "" : "variant=" + num(c.cfg.geo.variant) + " bc_level=" + num(c.cfg.geo.bc_level) + " block_x=" + num(c.cfg.block_x) +
                           " has_force=" + num(c.cfg.phys.has_force));
  }
  // the support table as sailfish_amd/serves.py must hold it: name, position, per_node_only, the masks in the order of slf::Column
  int position = 0;
  for (const slf::Serves& row : slf::SERVES) {
    std::string masks;
    for (int col = 0; col < slf::N_COLUMNS; col++) masks += (col ? " " : "") + std::to_string(row.serves[col]);
    line("serves", row.name, "-", "row" + num(position++), row.per_node_only, "", masks);
  }
  std::vector<std::string> names;
  for (const slf::KernelRow& r : slf::KERNEL_TABLE) {
    bool seen = false;
    for (const std::string& n : names) seen = seen || n == r.name;
    if (!seen) names.push_back(r.name);
  }
  names.push_back("");
  names.push_back("NoSuchKernel");
  for (const std::string& name_s : names) {
    const char* name = name_s.c_str();
    for (const Config& cc : configs) {
      if (cc.code) continue;
      const slf::ModuleConfig& c = cc.cfg;
      const slf::KernelRow* row = nullptr;
      std::string err;
      const int rc = slf::resolve(c, name, &row, &err);
      line("resolve", name_s, cc.name, "-", rc, err, rc ? "" : "kind=" + num(row->kind) + " local_velocity=" + num(row->local_velocity));
      if (rc) continue;
      const slf::KernelRow* sig = signature_of(name, row->kind);
      if (!sig) {
        line("bind", name_s, cc.name, "no-signature", -1, "", "");
        continue;
      }
      for (const auto& call : calls_for(c, *sig)) {
        const std::string& fmt = call.second.fmt;
        // argument i: a pointer 0x1000 * (i + 1) or the integer 100 + i
        std::vector<unsigned long long> pv(fmt.size() + 1);
        std::vector<int32_t> iv(fmt.size() + 1);
        std::vector<const void*> argv(fmt.size() + 1);
        for (size_t i = 0; i < fmt.size(); i++) {
          pv[i] = 0x1000ull * (i + 1);
          iv[i] = 100 + (int)i;
          argv[i] = fmt[i] == 'i' ? (const void*)&iv[i] : (const void*)&pv[i];
        }
        slf::BoundArgs bound = {};
        err.clear();
        const int brc = slf::bind(c, *row, fmt.c_str(), argv.data(), call.second.argc, &bound, &err);
        line("bind", name_s, cc.name, call.first, brc, err, brc ? "" : dump(bound));
      }
    }
  }
  const slf::ModuleConfig* c2 = nullptr;
  const slf::ModuleConfig* c3 = nullptr;
  for (const Config& cc : configs) {
    if (cc.name == "bgk-d2q9-aa-direct") c2 = &cc.cfg;
    if (cc.name == "bgk-d3q19-aa-direct") c3 = &cc.cfg;
  }
  face_boxes(*c2, *c3);
  launch_sections(configs);
  return 0;
}
