// Ternary Shan-Chen mixture (reference lb_ternary.py, templates/models/lb_ternary_fluid.mako, ternary_shan_chen.mako) for
// gfx950, BGK: three lattices with the densities rho, phi, theta, coupled by nine pseudopotential forces.
//
//   sc3_macro_kernel   ShanChenPrepareMacroFields          (ternary_shan_chen.mako:19-99)
//   sc3_sweep_kernel   ShanChenCollideAndPropagate{0,1,2}  (:101-154, shan_chen.mako:9-84); the lattice is a run-time value
//   sc3_fused_kernel   the three of them in one pass ("ShanChenCollideAndPropagateFused", ternary argument list)
//   sc3_init_kernel    SetInitialConditions                (lb_ternary_fluid.mako)
//
// Layout, streaming modes and launch shape as the free-energy sweeps (slf_fe.hip): whole-row workgroups with row_push() for
// the x-streaming steps in 3-D, the node's own slots in the even in-place step.  The node prologue (nn_kind), the stencil
// sum (sc_stencil), the common velocity (sc_add_momentum) and the launch shape (nn_shape) are slf_nn.h's, shared with the
// binary model.
//
// Operation order (the numpy twin tests/_scn_twin.py restates it):
//   pass in front, wet nodes:   rho_k = ((f_k,0 + f_k,1) + ...) of the populations as this step reads them
//                               v     = (1/tau_0) j_0, then v = v + (1/tau_1) j_1, then v = v + (1/tau_2) j_2
//                               total = ((1/tau_0) rho_0 + (1/tau_1) rho_1) + (1/tau_2) rho_2,  v = v / total
//   sweep of lattice K:         S_j   = sum_i psi(rho_j(x + e_i)) (+-w_i), i = 1 .. Q - 1, per component (sc_stencil, slf_nn.h)
//                               a     = 0; for j = 0, 1, 2 with G_Kj != 0:  a = a + S_j ((0 - psi(rho_K)) G_Kj)
//                               a     = a / rho_K [+ the body acceleration of lattice K]
//                               full-way bounce-back swap on wall nodes; bgk_relax_accel(f, rho_K, v, 1/tau_K, 3 (1 - 1/(2 tau_K)), a)
//   fused sweep:                S_0, S_1, S_2 and psi(rho_k) once per node, then lattices 0, 1, 2 one after the other -- the
//                               same operations on the same values, so the same bits
// Wave-uniform choices (node map or none, the potential through sc_with_potential, Guo or EDM, which couplings are zero, which
// lattice a sweep serves) are run-time values: one instantiation per lattice type, precision and streaming mode --
// 8 (pass in front) + 12 (sweep) + 12 (fused sweep) + 4 (initial conditions) = 36.
#include <string.h>
#include "slf_nn.h"

namespace slf {

template <class R>
struct Sc3Params {
  const uint32_t* __restrict__ map;   // NULL: every real node is a fluid node
  const R* d_in[3];    // pass in front, fused sweep: lattices 0, 1, 2 | sweep of one lattice: [0]
  R* d_out[3];
  R* field[3];         // rho, phi, theta
  R* vx;
  R* vy;
  R* vz;
  uint32_t options;
  int y0, z0;
  int xcd_shift;
  Geometry g;
  R omega[3];          // 1 / tau, 1 / tau_phi, 1 / tau_theta
  R guo_pref[3];
  R G[9];              // row-major: G[3 k + j] couples lattice k to field j
  R accel[3][3];       // [lattice][component]
  int has_body_force[3];
  int potential;
  int force_edm;
  // the sweep of one lattice: its own density field and constants (filled by the host from the arrays above)
  const R* own;
  R omega_k, guo_k;
  R Gk[3];
  R accel_k[3];
  int has_force_k;
};

// PROP: PROP_AB (the node's own slots: two-copy and the even in-place step) | PROP_AA_ODD
template <class L, class R, int PROP>
__global__ void __launch_bounds__(1024) sc3_macro_kernel(const Sc3Params<R> p) {
  const Geometry& g = p.g;
  bool live;
  const ScNode n = sc_node<L>(g, p.y0, p.z0, g.lat_nx - 2, live, p.xcd_shift);
  if (!live) return;
  const uint32_t gi = n.gi;
  if (p.map) {
    const int kind = node_kind(g.type_lut, g.type_mask, p.map[gi]);
    if (!kind_is_wet(kind)) return;
  }
  const size_t ds = g.dist_size;
  R rho[3];
  R v[3] = {(R)0, (R)0, (R)0};
  static_for<0, 3>([&](auto K) {
    R f[L::Q];
    sc_load<L, R, PROP>(f, p.d_in[K], ds, n);
    rho[K] = density<L, R>(f);
    sc_add_momentum<L, R, K == 0>(v, p.omega[K], f);
  });
  const R total = (p.omega[0] * rho[0] + p.omega[1] * rho[1]) + p.omega[2] * rho[2];
  p.field[0][gi] = rho[0];
  p.field[1][gi] = rho[1];
  p.field[2][gi] = rho[2];
  p.vx[gi] = v[0] / total;
  p.vy[gi] = v[1] / total;
  if constexpr (L::dim == 3) p.vz[gi] = v[2] / total;
}

// One lattice (p.d_in[0] -> p.d_out[0]; p.own, p.omega_k, p.guo_k, p.Gk, p.accel_k are its field and constants).
// ROW: one workgroup = one whole row, streaming through row_push(); every thread stays until the end (barrier inside).
template <class L, class R, int PROP>
__global__ void __launch_bounds__(1024) sc3_sweep_kernel(const Sc3Params<R> p) {
  constexpr bool ROW = L::dim == 3 && PROP != PROP_AA_EVEN;
  const Geometry& g = p.g;
  const int nx = g.lat_nx - 2;
  bool live;
  const ScNode n = sc_node<L>(g, p.y0, p.z0, nx, live, p.xcd_shift);
  const uint32_t gi = n.gi;
  NnKind nk;
  if (!nn_kind<ROW>(g, p.map, gi, live, nk)) return;
  const size_t ds = g.dist_size;

  R f[L::Q];
  sc_load<L, R, PROP>(f, p.d_in[0], ds, n);
  const R rho = p.own[gi];
  R a[3] = {(R)0, (R)0, (R)0};
  if (nk.wet) {
    sc_with_potential(p.potential, [&](auto POT) {
      const R psi_loc = sc_psi<R, POT>(rho);
      static_for<0, 3>([&](auto J) {
        const R cc = p.Gk[J];
        if (cc != (R)0) {
          R S[3] = {(R)0, (R)0, (R)0};
          sc_stencil<L, R, POT>((const R*)p.field[J], n, S);
          static_for<0, L::dim>([&](auto D) { a[D] = a[D] + S[D] * (((R)0 - psi_loc) * cc); });
        }
      });
    });
    static_for<0, L::dim>([&](auto D) { a[D] = a[D] / rho; });
    if (p.has_force_k) {
      static_for<0, L::dim>([&](auto D) { a[D] = a[D] + p.accel_k[D]; });
    }
  }
  R v[3];
  v[0] = p.vx[gi];
  v[1] = p.vy[gi];
  v[2] = (R)0;
  if constexpr (L::dim == 3) v[2] = p.vz[gi];
  if (nk.kind == NK_FULL_BB) bounce_back<L, R>(f);
  if (nk.wet) bgk_relax_accel<L, R>(f, rho, v, p.omega_k, p.guo_k, false, true, a, p.force_edm != 0);
  sc_store<L, R, PROP, true, ROW>(g, f, p.d_out[0], ds, n, nx, live, nk.active);
}

// The three lattices in one pass: the stencil sums S_0, S_1, S_2 of the fields some lattice is coupled to and the three
// psi(rho_k) are formed once per node (the three sweeps of the reference form each S_j up to three times), then lattice 0, 1
// and 2 are loaded, collided and streamed one after the other: one set of populations in registers at a time.
template <class L, class R, int PROP>
__global__ void __launch_bounds__(1024) sc3_fused_kernel(const Sc3Params<R> p) {
  constexpr bool ROW = L::dim == 3 && PROP != PROP_AA_EVEN;
  const Geometry& g = p.g;
  const int nx = g.lat_nx - 2;
  bool live;
  const ScNode n = sc_node<L>(g, p.y0, p.z0, nx, live, p.xcd_shift);
  const uint32_t gi = n.gi;
  NnKind nk;
  if (!nn_kind<ROW>(g, p.map, gi, live, nk)) return;
  const size_t ds = g.dist_size;

  R rho[3], psi_own[3];
  static_for<0, 3>([&](auto K) { rho[K] = p.field[K][gi]; });
  R vc[3] = {p.vx[gi], p.vy[gi], (R)0};
  if constexpr (L::dim == 3) vc[2] = p.vz[gi];
  R S[3][3] = {{(R)0, (R)0, (R)0}, {(R)0, (R)0, (R)0}, {(R)0, (R)0, (R)0}};
  static_for<0, 3>([&](auto K) { psi_own[K] = rho[K]; });
  if (nk.wet) {
    sc_with_potential(p.potential, [&](auto POT) {
      static_for<0, 3>([&](auto J) {
        if (p.G[J] != (R)0 || p.G[3 + J] != (R)0 || p.G[6 + J] != (R)0) sc_stencil<L, R, POT>((const R*)p.field[J], n, S[J]);
      });
      static_for<0, 3>([&](auto K) { psi_own[K] = sc_psi<R, POT>(rho[K]); });
    });
  }
  static_for<0, 3>([&](auto K) {
    // one lattice at a time: without the fence the scheduler starts the loads of the next lattice under the collision of
    // this one, and two sets of populations in registers cost resident waves
    __builtin_amdgcn_sched_barrier(0);
    R f[L::Q];
    sc_load<L, R, PROP>(f, p.d_in[K], ds, n);
    R a[3] = {(R)0, (R)0, (R)0};
    if (nk.wet) {
      static_for<0, 3>([&](auto J) {
        const R cc = p.G[3 * K + J];
        if (cc != (R)0) {
          static_for<0, L::dim>([&](auto D) { a[D] = a[D] + S[J][D] * (((R)0 - psi_own[K]) * cc); });
        }
      });
      static_for<0, L::dim>([&](auto D) { a[D] = a[D] / rho[K]; });
      if (p.has_body_force[K]) {
        static_for<0, L::dim>([&](auto D) { a[D] = a[D] + p.accel[K][D]; });
      }
    }
    R v[3] = {vc[0], vc[1], vc[2]};
    if (nk.kind == NK_FULL_BB) bounce_back<L, R>(f);
    if (nk.wet) bgk_relax_accel<L, R>(f, rho[K], v, p.omega[K], p.guo_pref[K], false, true, a, p.force_edm != 0);
    if constexpr (ROW && K > 0) __syncthreads();      // row_push's LDS words of the lattice before are still being read
    sc_store<L, R, PROP, true, ROW>(g, f, p.d_out[K], ds, n, nx, live, nk.active);
  });
}

// f_k = feq(rho_k, v) on every node of the arrays (no type test, as sc_init_kernel)
template <class L, class R>
__global__ void __launch_bounds__(256) sc3_init_kernel(R* d1, R* d2, R* d3, const R* __restrict__ irho, const R* __restrict__ iphi,
                                                      const R* __restrict__ itheta, const R* __restrict__ ivx,
                                                      const R* __restrict__ ivy, const R* __restrict__ ivz, Geometry g) {
  const int gx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int gy = (int)blockIdx.y;
  const int gz = (int)blockIdx.z;
  if (gx > g.lat_nx - 1) return;
  const uint32_t gi = (uint32_t)gx + (uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz;
  R v[3];
  v[0] = ivx[gi];
  v[1] = ivy[gi];
  v[2] = (R)0;
  if constexpr (L::dim == 3) v[2] = ivz[gi];
  const R u15 = usq15<L, R>(v);
  const R r0 = irho[gi], r1 = iphi[gi], r2 = itheta[gi];
  static_for<0, L::Q>([&](auto I) {
    (d1 + (size_t)g.dist_size * (size_t)I)[gi] = feq<L, R, I>(r0, r0, v, u15);
    (d2 + (size_t)g.dist_size * (size_t)I)[gi] = feq<L, R, I>(r1, r1, v, u15);
    (d3 + (size_t)g.dist_size * (size_t)I)[gi] = feq<L, R, I>(r2, r2, v, u15);
  });
}

// ---------------------------------------------------------------------------
template <class R>
static Sc3Params<R> make_sc3(const Geometry& g, const Physics& ph, const ShanChen3& sc, const Sc3Args& a, int y0, int z0) {
  Sc3Params<R> p;
  p.map = (const uint32_t*)a.map;
  for (int k = 0; k < 3; k++) {
    p.d_in[k] = (const R*)a.dist_in[k];
    p.d_out[k] = (R*)a.dist_out[k];
    p.field[k] = (R*)a.field[k];
  }
  p.vx = (R*)a.v[0];
  p.vy = (R*)a.v[1];
  p.vz = (R*)a.v[2];
  p.options = a.options;
  p.y0 = y0;
  p.z0 = z0;
  p.xcd_shift = 0;
  p.g = g;
  const double tau[3] = {ph.tau, sc.tau_phi, sc.tau_theta};
  // body forces act per lattice (reference add_body_force(force, grid=k), relaxation_common.mako:9-36)
  const double* acc[3] = {ph.accel, sc.accel1, sc.accel2};
  for (int k = 0; k < 3; k++) {
    p.omega[k] = (R)(1.0 / tau[k]);
    p.guo_pref[k] = (R)(3.0 * (1.0 - 0.5 / tau[k]));
    p.has_body_force[k] = 0;
    for (int d = 0; d < 3; d++) {
      p.accel[k][d] = (R)acc[k][d];
      if (p.accel[k][d] != (R)0) p.has_body_force[k] = 1;
    }
  }
  for (int i = 0; i < 9; i++) p.G[i] = (R)sc.G[i];
  p.potential = sc.potential;
  p.force_edm = ph.force_edm;
  p.own = nullptr;
  p.omega_k = p.guo_k = (R)0;
  for (int d = 0; d < 3; d++) p.Gk[d] = p.accel_k[d] = (R)0;
  p.has_force_k = 0;
  return p;
}

hipError_t launch_sc3_macro(const Launch& lc, const ShanChen3& sc, const Sc3Args& a) {
  const auto& [sel, prop, g, ph, y0, y1, z0, z1, block_x, s] = lc;
  return pick_lr(sel, [&](auto lr) {
    using L = typename decltype(lr)::L;
    using R = typename decltype(lr)::R;
    const Sc3Params<R> p = make_sc3<R>(g, ph, sc, a, y0, z0);
    const NNShape sh = nn_shape<L>(g, false, prop, y0, y1, z0, z1, nn_pass_block_x(g.lat_nx - 2));
    if (sh.empty) return hipSuccess;
    // two-copy and the even in-place step: the node's own slots
    if (prop == PROP_AA_ODD) hipLaunchKernelGGL((sc3_macro_kernel<L, R, PROP_AA_ODD>), sh.grid, sh.block, 0, s, p);
    else hipLaunchKernelGGL((sc3_macro_kernel<L, R, PROP_AB>), sh.grid, sh.block, 0, s, p);
    return hipGetLastError();
  });
}

// which: 0 .. 2 the sweep of that lattice (a.dist_in[0] -> a.dist_out[0]), 3 the fused sweep of all of them
static hipError_t sc3_sweep(const Launch& lc, const ShanChen3& sc, const Sc3Args& a, int which) {
  const auto& [sel, prop, g, ph, y0, y1, z0, z1, block_x, s] = lc;
  return pick_lr(sel, [&](auto lr) {
    using L = typename decltype(lr)::L;
    using R = typename decltype(lr)::R;
    Sc3Params<R> p = make_sc3<R>(g, ph, sc, a, y0, z0);
    if (which < 3) {
      const int k = which;
      p.own = p.field[k];
      p.omega_k = p.omega[k];
      p.guo_k = p.guo_pref[k];
      for (int j = 0; j < 3; j++) {
        p.Gk[j] = p.G[3 * k + j];
        p.accel_k[j] = p.accel[k][j];
      }
      p.has_force_k = p.has_body_force[k];
    }
    const NNShape sh = nn_shape<L>(g, true, prop, y0, y1, z0, z1, block_x);      // the x-streaming steps in 3-D: whole rows
    if (sh.empty) return hipSuccess;
    p.xcd_shift = sh.xcd_shift;      // the stencil's density rows: neighbouring rows on one XCD
    hipError_t e = hipErrorInvalidValue;
    pick_prop(prop, [&](auto P) {
      if (which < 3) hipLaunchKernelGGL((sc3_sweep_kernel<L, R, P>), sh.grid, sh.block, 0, s, p);
      else hipLaunchKernelGGL((sc3_fused_kernel<L, R, P>), sh.grid, sh.block, 0, s, p);
      e = hipGetLastError();
    });
    return e;
  });
}

hipError_t launch_sc3_sweep(const Launch& lc, const ShanChen3& sc, const Sc3Args& a, int lattice) {
  if (lattice < 0 || lattice > 2) return hipErrorInvalidValue;
  return sc3_sweep(lc, sc, a, lattice);
}

hipError_t launch_sc3_fused(const Launch& lc, const ShanChen3& sc, const Sc3Args& a) { return sc3_sweep(lc, sc, a, 3); }

hipError_t launch_sc3_init(const KernelSelector& sel, const Geometry& g, void* const dist[3], const void* const field[3],
                           const void* const v[3], hipStream_t s) {
  return pick_lr(sel, [&](auto lr) {
    using L = typename decltype(lr)::L;
    using R = typename decltype(lr)::R;
    const dim3 grid((g.lat_nx + 255) / 256, g.lat_ny, g.lat_nz);
    hipLaunchKernelGGL((sc3_init_kernel<L, R>), grid, dim3(256, 1, 1), 0, s, (R*)dist[0], (R*)dist[1], (R*)dist[2],
                       (const R*)field[0], (const R*)field[1], (const R*)field[2], (const R*)v[0], (const R*)v[1],
                       (const R*)v[2], g);
    return hipGetLastError();
  });
}

}  // namespace slf
