// The compile-time switches of the per-node code (node_update, slf_sweep.h) and of the per-node sweep (sweep_kernel,
// slf_kernels.hip) as one value, and the one statement of which of its values exist as instantiations of that sweep.
// Plain constexpr data and functions: host code (slf_bind.h, on a CPU) and the kernels' template arguments read the same
// lines.  Calls no HIP function.
#pragma once
#include "../../include/sailfish_hip.h"
#include "slf_kernels.h"
#include "slf_node.h"

namespace slf {

// model: 0 BGK, 1 MRT, 2 entropic (slf_node.h elbm_relax; the per-node sweep only).
// prop: the propagation step (Prop).  general: the node map is read.  indirect: indirect addressing.
// force: FORCE_RUNTIME, or 0 / 1 where a kernel family is instantiated per "module has a body force" (slf_row.hip).
// bcl: the module's Geometry::bc_level the instantiation is for (2 = everything; the outflow, do-nothing and full-slip nodes
// exist at level 2 only, so that the level-1 kernels of the usual wall / inlet / outlet conditions do not carry their code).
// roundoff: the --minimize_roundoff formulation (slf_node.h: macro_roundoff, bgk_relax_roundoff): BGK; fluid, full-way
// and half-way bounce-back nodes (the module is refused otherwise); the per-node sweep only.
// turb: the BGK collision with the options of the reference's relaxation preamble (--regularized, --subgrid; which of
// the two: SweepParams::turb_flags) -- slf_node.h bgk_relax_turb; the per-node sweep only, BGK.
// tms: the module has Tamm-Mott-Smith wall nodes (SweepParams::tms_mask != 0): half-way bounce-back types with the flag run
// tms_fix_missing before and tms_add_equilibrium_difference after the collision; the target state stays live across it.
// The per-node sweep and the slot sweep only; instantiations of their own, so that the others do not carry the registers.
// accf: the module has an acceleration field (slf_module_desc::accel_field): the collision takes the node's acceleration
// from `acc` (the caller formed cp.accel + field[gi]) instead of cp.accel.  The per-node sweep only; `acc` is not read otherwise.
// sw: a shallow-water module (slf_module_desc::equilibrium = SLF_EQ_SHALLOW_WATER): the BGK relaxation uses sw_equilibrium
// (slf_node.h) with p.cp.gravity -- and that is all: moments, bounce-back, the half-way store, the slip reflection and
// streaming are the code of every other module.  The per-node sweep only; the value-carrying node kinds are refused at
// module creation (slf_bind.h SERVES).
struct SweepVariant {
  int model = 0;
  int prop = PROP_AB;
  bool general = false, indirect = false;
  int force = FORCE_RUNTIME, bcl = 2;
  bool roundoff = false, turb = false, tms = false, accf = false, sw = false;
};

// What node_update is written for, whichever kernel calls it: NULL, or the rule the variant breaks.
constexpr const char* node_variant_conflict(SweepVariant v) {
  if (v.accf && (v.model == 2 || v.indirect || v.roundoff || v.turb || v.tms))
    return "no per-node code for accf (accel_field) with model = elbm, indirect addressing, roundoff, turb or tms";
  if (v.sw && (v.model != 0 || v.indirect || v.roundoff || v.turb || v.tms))
    return "no per-node code for sw (equilibrium = shallow water) with a model other than BGK, indirect addressing, roundoff, turb or tms";
  return nullptr;
}
constexpr bool node_variant_ok(SweepVariant v) { return node_variant_conflict(v) == nullptr; }

// Which variants the per-node sweep is instantiated for (launch_sweep2 instantiates exactly these; module_config refuses a
// module that would need another): NULL, or the rule the variant breaks.  lattice_id: L::id = SLF_D2Q9 | SLF_D3Q19.
constexpr const char* per_node_variant_conflict(int lattice_id, SweepVariant v) {
  if (v.force != FORCE_RUNTIME || v.bcl != 2) return "no per-node sweep with force != FORCE_RUNTIME or bcl != 2";
  if (v.indirect && !v.general) return "no per-node sweep with indirect addressing and without the node map (general): the map is always read";
  if (v.roundoff && v.turb) return "no per-node sweep with roundoff (minimize_roundoff) and turb (regularized / subgrid) together";
  if ((v.roundoff || v.turb) && v.model != 0) return "no per-node sweep with roundoff (minimize_roundoff) or turb (regularized / subgrid) and a model other than BGK";
  if (v.tms && !v.general) return "no per-node sweep with tms (NTWallTMS types) and without the node map (general): the walls are node types";
  if (v.sw && lattice_id != SLF_D2Q9) return "no per-node sweep with sw (equilibrium = shallow water) on a lattice other than D2Q9";
  return node_variant_conflict(v);
}
constexpr bool per_node_variant_exists(int lattice_id, SweepVariant v) { return per_node_variant_conflict(lattice_id, v) == nullptr; }

// Threads per workgroup of the per-node sweep, its launch bound.  turb: 256 VGPRs -- the non-equilibrium flux tensor on top
// of the collision does not fit the 128 of a 1024-thread workgroup (76-152 bytes of scratch per lane in the odd step).
// model = 2: f and fneq stay live across the Newton solve.  accf: under 128 VGPRs the D3Q19 odd-step instantiations spill
// (20-32 bytes of scratch per lane in single, 84-136 in double precision: profiles/accf).  sw alone: nine populations and
// one more equilibrium array, no scratch under 128 VGPRs (profiles/sw).
constexpr int sweep_max_threads(SweepVariant v) { return (v.turb || v.model == 2 || v.accf) ? 512 : 1024; }

// The variant of the per-node sweep that a module's run-time values select for the step `prop`.
// BGK only (checked at module creation): --minimize_roundoff; --regularized / --subgrid=les-smagorinsky.
constexpr SweepVariant per_node_variant_of(const KernelSelector& sel, const Geometry& g, const Physics& ph, Prop prop) {
  SweepVariant v;
  v.model = (sel.model != 0 && sel.model != 2) ? 1 : sel.model;
  v.prop = prop;
  v.general = sel.general || g.indirect;
  v.indirect = g.indirect != 0;
  v.roundoff = v.model == 0 && ph.incompressible == SLF_DENSITY_ROUNDOFF;
  v.turb = v.model == 0 && !v.roundoff && (ph.regularized || ph.subgrid);
  v.tms = ph.tms_mask != 0;
  v.accf = ph.accel_field != 0;
  v.sw = ph.equilibrium == SLF_EQ_SHALLOW_WATER;
  return v;
}

}  // namespace slf
