// D3Q15 and D3Q27 (slf_lattice.h) for gfx950: the BGK collide-and-stream sweep of a single fluid with full-way and half-way
// bounce-back walls and body forces, and the lattice-generic kernels of slf_plain.h instantiated for the two lattices.
//
//   lat_sweep_kernel  CollideAndPropagate                       (lb_single_fluid.mako:161-229)
//   init_kernel       SetInitialConditions                      } slf_plain.h
//   pbc_kernel        ApplyPeriodicBoundaryConditions[WithSwap] }
//   macro_kernel      ComputeMacroFields                        }
//
// The sweep has the shape of fe_sweep_kernel (slf_fe.hip): one workgroup per (y, z) row -- or per x-segment of one --
// that streams through row_push() in the two-copy pattern and the odd in-place step, and into the node's own opposite
// slots in the even in-place step.  Everything per node is a piece of slf_node.h / slf_sweep.h / slf_nn.h (sc_node, nn_kind,
// sc_load, sc_store) templated on the lattice; nothing here knows a direction by number.  The launch shape is nn_shape()
// with this unit's bound on threads per workgroup.
//
// Operation order per node (the arithmetic of the D3Q19 general path, node_update<..., GENERAL, BCL = 0> plus its half-way
// wall, with other tables; the numpy twin tests/_lat_twin.py restates it):
//   1. sc_load: the node's own slots (two-copy, even in-place step) or the opposite slots of its neighbours (odd step)
//   2. wet nodes (fluid, half-way wall):
//        rho = ((f_0 + f_1) + f_2) + ...;  j_d = sum over i in index order of +-f_i;  v_d = j_d / rho (compressible)
//        unless relaxation is off: bgk_relax_accel --
//          Guo:  v += a / 2;  f_i += omega (feq_i(rho, v) - f_i);  f_i += (rho pref) w_i (((e_i.a) - (v.a)) + 3 (e_i.v) (e_i.a))
//          EDM:  f_i += omega (feq_i(rho, v) - f_i);  f_i += feq_i(rho, v + a) - feq_i(rho, v);  v += a / 2
//          feq_i = w_i (rho + rho0 ((e_i.v) (3 + 4.5 (e_i.v)) - 1.5 v^2)),  rho0 = 1 (incompressible) | rho
//        the invalid-value check, then rho and v (the velocity the collision used, as in every other sweep) where
//        options bit 0 asks for them
//   3. full-way walls: f_i <-> f_opp(i)
//   4. half-way walls: half_bb_store -- f_i of every direction that points at a non-fluid node goes where the node's next
//      step reads population opp(i)
//   5. sc_store: the aligned row push, or the opposite slots
#include <string.h>
#include "slf_nn.h"
#include "slf_plain.h"

namespace slf {

// Threads per workgroup, i.e. registers per thread.  Single-precision D3Q15 fits the 128 VGPRs of a 1024-thread workgroup
// (90 VGPRs); D3Q27 does not -- 27 populations, the nine shifted values of a sign of e_x and the addresses spill 20-36 bytes
// at 128 -- and takes 768 threads (170 VGPRs).  Double precision doubles the populations: 512 threads (256 VGPRs).  Rows
// longer than the bound are cut into segments, which row_push() serves.
template <class L, class R>
constexpr int lat_max_threads() { return sizeof(R) == 8 ? 512 : (L::Q > 19 ? 768 : 1024); }

template <class L, class R, int PROP>
__global__ void __launch_bounds__((lat_max_threads<L, R>())) lat_sweep_kernel(const SweepParams<L, R> p) {
  constexpr bool ROW = PROP != PROP_AA_EVEN;
  const Geometry& g = p.g;
  const int nx = g.lat_nx - 2;
  bool live;
  const ScNode n = sc_node<L>(g, p.y0, p.z0, nx, live);
  NnKind nk;
  if (!nn_kind<ROW>(g, p.map, n.gi, live, nk)) return;
  const size_t ds = g.dist_size;
  const uint32_t lo = n.xi * (uint32_t)sizeof(R);

  R f[L::Q];
  sc_load<L, R, PROP>(f, p.din, ds, n);
  if (nk.wet) {
    R rho, v[3];
    macro_standard<L, R>(f, p.cp.incompressible != 0, rho, v);
    if (p.relaxation_enabled) bgk_relax<L, R>(f, rho, v, p.cp);
    check_invalid<R>(p.status, p.options, rho, n.gx, n.gy, n.gz);
    if (p.options & 1u) {
      *at_byte(uniform_base(p.rho + n.row), lo) = rho;
      *at_byte(uniform_base(p.vx + n.row), lo) = v[0];
      *at_byte(uniform_base(p.vy + n.row), lo) = v[1];
      *at_byte(uniform_base(p.vz + n.row), lo) = v[2];
    }
  }
  if (nk.kind == NK_FULL_BB) bounce_back<L, R>(f);
  if (nk.kind == NK_HALF_BB && nk.active) half_bb_store<L, R, PROP, false>(p, f, (int)(nk.code >> g.orient_shift), n.gi, n.gi, n.ox, n.oy, n.oz);
  sc_store<L, R, PROP, true, ROW>(g, f, p.dout, ds, n, nx, live, nk.active);
}

// ---------------------------------------------------------------------------
// The unit's own picker: D3Q15 | D3Q27 x float | double.  Any other lattice id is an error.
template <class F>
static hipError_t pick_lat(const KernelSelector& sel, F&& f) {
  if (sel.precision != 4 && sel.precision != 8) return hipErrorInvalidValue;
  if (sel.lattice == D3Q15::id) return pick_real(sel, [&](auto r) { return f(LR<D3Q15, decltype(r)>{}); });
  if (sel.lattice == D3Q27::id) return pick_real(sel, [&](auto r) { return f(LR<D3Q27, decltype(r)>{}); });
  return hipErrorInvalidValue;
}

hipError_t launch_lat_sweep(const Launch& lc, const SweepArgs& a) {
  const auto& [sel, prop, g, ph, y0, y1, z0, z1, block_x, s] = lc;
  if (sel.model != SLF_BGK || g.indirect) return hipErrorInvalidValue;      // (refused at module creation)
  return pick_lat(sel, [&](auto lr) {
    using L = typename decltype(lr)::L;
    using R = typename decltype(lr)::R;
    SweepArgs b = a;
    if (!sel.general) b.map = nullptr;
    b.nodes = nullptr;
    b.rows = nullptr;
    b.slots = nullptr;
    const SweepParams<L, R> p = make_params<L, R>(g, ph, b, y0, z0);
    const NNShape sh = nn_shape<L>(g, true, prop, y0, y1, z0, z1, block_x, lat_max_threads<L, R>());
    if (sh.empty) return hipSuccess;
    hipError_t e = hipErrorInvalidValue;
    pick_prop(prop, [&](auto P) {
      hipLaunchKernelGGL((lat_sweep_kernel<L, R, P>), sh.grid, sh.block, 0, s, p);
      e = hipGetLastError();
    });
    return e;
  });
}

hipError_t launch_lat_init(const KernelSelector& sel, const Geometry& g, const Physics& ph, void* dist, const void* rho,
                           const void* const v[3], hipStream_t s) {
  return pick_lat(sel, [&](auto lr) { return launch_init2(lr, g, ph, dist, rho, v, nullptr, s); });
}

hipError_t launch_lat_pbc(const KernelSelector& sel, const Geometry& g, void* dist, int axis, bool with_swap, hipStream_t s) {
  if (axis < 0 || axis >= g.dim) return hipErrorInvalidValue;
  return pick_lat(sel, [&](auto lr) { return launch_pbc2(lr, g, dist, axis, with_swap, s); });
}

hipError_t launch_lat_macro(const Launch& lc, const SweepArgs& a) {
  return pick_lat(lc.sel, [&](auto lr) {
    SweepArgs b = a;
    b.nodes = nullptr;
    return launch_macro2(lr, lc.prop, lc.sel.general, lc.g, lc.ph, b, lc.s);
  });
}

}  // namespace slf
