// Free-energy binary fluid (reference lb_binary.py:139-372, templates/models/lb_binary_fluid.mako) for gfx950, BGK.
//
//   fe_macro_kernel   FreeEnergyPrepareMacroFields             (lb_binary_fluid.mako:130-254)
//   fe_sweep_kernel<0> FreeEnergyCollideAndPropagateFluid      (:256-320)
//   fe_sweep_kernel<1> FreeEnergyCollideAndPropagateOrderParam (:322-369)
//   fe_init_kernel    SetInitialConditions                     (:64-127)
//
// Lattice 0 carries the density rho, lattice 1 the order parameter phi.  The pass in front stores phi of every node (wall
// nodes: the wetting condition); the fluid sweep reads the 18 (8) neighbour values of phi through the caches like the
// Shan-Chen force stencil (sc_neighbour, slf_nn.h), forms the Laplacian and the gradient with the stencils of Pooley &
// Furtado (PRE 77, 046702; finite_difference_optimized.mako:41-48), and leaves the velocity and the Laplacian in memory
// for the order-parameter sweep.  Equilibria: sym_equilibrium.py:15-71 (Pooley, Kusumaatmaja & Yeomans, PRE 78, 056709).
//
// Operation order (the numpy twin tests/_fe_twin.py restates it):
//   h_i   = (eu + 1.5 (eu eu)) - 0.5 (vx vx + vy vy [+ vz vz])                        eu = e_i . v as edotv()
//   pb    = rho / 3 + A (phi2 (0.75 phi2 - 0.5))                                       phi2 = phi phi
//   f_i   = wi_i ((pb - (kappa phi) lap) + rho h_i) + kappa (((wxx_i gx gx + wyy_i gy gy) [+ wzz_i gz gz]) [+ wab_i (ga gb)])
//   g_i   = wi_i (Gamma (A (phi phi2 - phi) - kappa lap) + phi h_i)
//   f_0   = rho - ((f_1 + f_2) + ...),  g_0 = phi - ((g_1 + g_2) + ...)
//   tau0  = tau_b + ((phi + 1) (tau_a - tau_b)) 0.5, tau_b below phi = -1, tau_a above phi = 1;  f += (1 / tau0) (feq - f)
// Wave-uniform choices (node map or none, wetting order, which rims have zero gradients) are run-time values: one
// instantiation per lattice, precision and streaming mode for each of the three kernels.  Node position and kind (sc_node,
// nn_kind), loads and stores (sc_load, sc_store) and the launch shape (nn_shape) are slf_nn.h's.
#include <string.h>
#include "slf_nn.h"

namespace slf {

template <int K>
using fe_ic = std::integral_constant<int, K>;

// weight tables of lb_binary.py:198-268, by direction (basis order of slf_lattice.h)
template <class L, class R>
struct FeWeights {
  static constexpr bool axis(int i) { return L::ex(i) * L::ex(i) + L::ey(i) * L::ey(i) + L::ez(i) * L::ez(i) == 1; }
  static constexpr R wi(int i) { return axis(i) ? (L::dim == 3 ? (R)(1.0 / 6.0) : (R)(1.0 / 3.0)) : (R)(1.0 / 12.0); }
  // wxx, wyy, wzz: d = 0, 1, 2
  static constexpr R waa(int i, int d) {
    const bool along = e_comp<L>(i, d) != 0;
    if (L::dim == 3) return axis(i) ? (along ? (R)(5.0 / 12.0) : (R)(-1.0 / 3.0)) : (along ? (R)(-1.0 / 24.0) : (R)(1.0 / 12.0));
    return axis(i) ? (along ? (R)(1.0 / 3.0) : (R)(-1.0 / 6.0)) : (R)(-1.0 / 24.0);
  }
  // wxy, wyz, wxz: e_a e_b / 4
  static constexpr R wab(int i, int a, int b) { return (R)(0.25 * (double)(e_comp<L>(i, a) * e_comp<L>(i, b))); }
};

template <class R>
struct FeParams {
  const uint32_t* __restrict__ map;   // NULL: every real node is a fluid node
  const R* d_in;     // sweep: lattice in      | macro: lattice 1
  R* d_out;          // sweep: lattice out
  R* rho;
  R* phi;
  R* vx;
  R* vy;
  R* vz;
  R* lap;
  uint32_t options;
  int y0, z0;
  int xcd_shift;
  Geometry g;
  R Gamma, kappa, A, tau_a, tau_b;
  R omega_phi;       // 1 / tau_phi
  R wall_shift;      // bc_wall_grad_order * bc_wall_grad_phase
  int wall_order;    // 1 | 2
  int rim[3];        // per axis: 1 = the low rim layer has zero gradient and Laplacian, 2 = the high one (mako_utils.mako:168-197)
};

template <class R>
__device__ __forceinline__ bool fe_on_zero_rim(const int (&rim)[3], const Geometry& g, int x, int y, int z) {
  bool r = (rim[0] == 1 && x == 1) || (rim[0] == 2 && x == g.lat_nx - 2) || (rim[1] == 1 && y == 1) || (rim[1] == 2 && y == g.lat_ny - 2);
  if (g.dim == 3) r = r || (rim[2] == 1 && z == 1) || (rim[2] == 2 && z == g.lat_nz - 2);
  return r;
}

// laplacian_and_grad (finite_difference_optimized.mako:20-48) in the reference's operation order; at(fe_ic<I>{}) is the
// field at the neighbour in direction I, c the field at the node
template <class L, class R, class F>
__device__ __forceinline__ void fe_stencil(F&& at, R c, R& lap, R (&grad)[3]) {
  if constexpr (L::dim == 3) {
    const R fe = at(fe_ic<1>{}), fw = at(fe_ic<2>{}), fn = at(fe_ic<3>{}), fs = at(fe_ic<4>{}), ft = at(fe_ic<5>{}), fb = at(fe_ic<6>{});
    const R fne = at(fe_ic<7>{}), fnw = at(fe_ic<8>{}), fse = at(fe_ic<9>{}), fsw = at(fe_ic<10>{});
    const R ftn = at(fe_ic<11>{}), fts = at(fe_ic<12>{}), fbn = at(fe_ic<13>{}), fbs = at(fe_ic<14>{});
    const R fte = at(fe_ic<15>{}), ftw = at(fe_ic<16>{}), fbe = at(fe_ic<17>{}), fbw = at(fe_ic<18>{});
    grad[0] = (((((((((R)0 -fnw) - fsw) - ftw) - fbw) + fse) + fne) + fte) + fbe) / (R)12 + (fe - fw) / (R)6;
    grad[1] = (((((((((R)0 -fse) - fsw) - fts) - fbs) + fne) + fnw) + ftn) + fbn) / (R)12 + (fn - fs) / (R)6;
    grad[2] = (((((((((R)0 -fbe) - fbw) - fbn) - fbs) + fte) + ftw) + ftn) + fts) / (R)12 + (ft - fb) / (R)6;
    lap = (((((((((((fnw + fne) + fse) + fsw) + fte) + ftw) + ftn) + fts) + fbe) + fbw) + fbn) + fbs) / (R)6 +
          (((((ft + fb) + fe) + fw) + fn) + fs) / (R)3 - (R)4 * c;
  } else {
    const R fe = at(fe_ic<1>{}), fn = at(fe_ic<2>{}), fw = at(fe_ic<3>{}), fs = at(fe_ic<4>{});
    const R fne = at(fe_ic<5>{}), fnw = at(fe_ic<6>{}), fsw = at(fe_ic<7>{}), fse = at(fe_ic<8>{});
    grad[0] = (((((R)0 - fnw) - fsw) + fse) + fne) / (R)12 + (fe - fw) / (R)3;
    grad[1] = (((((R)0 - fse) - fsw) + fne) + fnw) / (R)12 + (fn - fs) / (R)3;
    grad[2] = (R)0;
    lap = (((((fnw + fne) + fsw) + fse) + (R)4 * (((fe + fw) + fn) + fs)) - (R)20 * c) / (R)6;
  }
}

template <class L, class R>
__device__ __forceinline__ R fe_half_usq(const R (&v)[3]) {
  R s = v[0] * v[0] + v[1] * v[1];
  if constexpr (L::dim == 3) s = s + v[2] * v[2];
  return (R)0.5 * s;
}
template <class R>
__device__ __forceinline__ R fe_h(R eu, R husq) { return (eu + (R)1.5 * (eu * eu)) - husq; }

// free_energy_equilibrium_fluid (sym_equilibrium.py:15-48; lambda_ = 0 on D2Q9 / D3Q19)
template <class L, class R>
__device__ __forceinline__ void fe_feq_fluid(R (&fe)[L::Q], R rho, R phi, R lap, const R (&v)[3], const R (&grad)[3], R A, R kappa) {
  const R phi2 = phi * phi;
  const R pb = rho / (R)3 + A * (phi2 * ((R)0.75 * phi2 - (R)0.5));
  const R bulk = pb - (kappa * phi) * lap;
  const R husq = fe_half_usq<L, R>(v);
  R gg[3] = {grad[0] * grad[0], grad[1] * grad[1], (R)0};
  if constexpr (L::dim == 3) gg[2] = grad[2] * grad[2];
  R sum = (R)0;
  static_for<1, L::Q>([&](auto I) {
    using W = FeWeights<L, R>;
    const R eu = edotv<L, R, I>(v);
    R q = W::waa(I, 0) * gg[0] + W::waa(I, 1) * gg[1];
    if constexpr (L::dim == 3) q = q + W::waa(I, 2) * gg[2];
    if constexpr (L::ex(I) * L::ey(I) != 0) q = q + W::wab(I, 0, 1) * (grad[0] * grad[1]);
    if constexpr (L::ey(I) * L::ez(I) != 0) q = q + W::wab(I, 1, 2) * (grad[1] * grad[2]);
    if constexpr (L::ex(I) * L::ez(I) != 0) q = q + W::wab(I, 0, 2) * (grad[0] * grad[2]);
    fe[I] = W::wi(I) * (bulk + rho * fe_h(eu, husq)) + kappa * q;
    sum = sum + fe[I];
  });
  fe[0] = rho - sum;
}

// free_energy_equilibrium_order_param (sym_equilibrium.py:50-71)
template <class L, class R>
__device__ __forceinline__ void fe_feq_order(R (&fe)[L::Q], R phi, R lap, const R (&v)[3], R A, R kappa, R Gamma) {
  const R phi2 = phi * phi;
  const R gmu = Gamma * (A * (phi * phi2 - phi) - kappa * lap);
  const R husq = fe_half_usq<L, R>(v);
  R sum = (R)0;
  static_for<1, L::Q>([&](auto I) {
    const R eu = edotv<L, R, I>(v);
    fe[I] = FeWeights<L, R>::wi(I) * (gmu + phi * fe_h(eu, husq));
    sum = sum + fe[I];
  });
  fe[0] = phi - sum;
}

// relaxation_common.mako:156-163
template <class R>
__device__ __forceinline__ R fe_tau0(R phi, R tau_a, R tau_b) {
  R tau0 = tau_b + ((phi + (R)1) * (tau_a - tau_b)) * (R)0.5;
  if (phi < (R)-1) tau0 = tau_b;
  else if (phi > (R)1) tau0 = tau_a;
  return tau0;
}

// zeroth moment of the populations of node (x, y, z) as getDist reads them in this step: any node of the arrays, per lane
template <class L, class R, int PROP>
__device__ __forceinline__ R fe_density_at(const Geometry& g, const R* din, int x, int y, int z) {
  const AxisOff ox = axis_off(x, g.lat_nx, 1, g.wrap[0]);
  const AxisOff oy = axis_off(y, g.lat_ny, g.arr_nx, g.wrap[1]);
  const AxisOff oz = (L::dim == 3) ? axis_off(z, g.lat_nz, g.arr_nxy, g.wrap[2]) : AxisOff{0, 0};
  const uint32_t gi = (uint32_t)x + (uint32_t)g.arr_nx * (uint32_t)y + (uint32_t)g.arr_nxy * (uint32_t)z;
  const size_t ds = g.dist_size;
  R f[L::Q];
  static_for<0, L::Q>([&](auto I) {
    if constexpr (PROP == PROP_AA_ODD) f[I] = (din + ds * (size_t)L::opp(I))[(uint32_t)((int)gi + dir_offset<L, I>(ox, oy, oz, false))];
    else f[I] = (din + ds * (size_t)I)[gi];
  });
  return density<L, R>(f);
}

// PROP: PROP_AB (the node's own slots: two-copy and the even in-place step) | PROP_AA_ODD
template <class L, class R, int PROP>
__global__ void __launch_bounds__(1024) fe_macro_kernel(const FeParams<R> p) {
  const Geometry& g = p.g;
  bool live;
  const ScNode n = sc_node<L>(g, p.y0, p.z0, g.lat_nx - 2, live, p.xcd_shift);
  if (!live) return;
  NnKind nk;
  nn_kind<true>(g, p.map, n.gi, live, nk);       // every kind stays: wall nodes get their phi here
  if (nk.wet) {
    R f[L::Q];
    sc_load<L, R, PROP>(f, p.d_in, g.dist_size, n);
    p.phi[n.gi] = density<L, R>(f);
  } else if (nk.kind == NK_FULL_BB) {
    // wetting walls (Kusumaatmaja, option 2): phi of the fluid node `order` nodes along the wall's normal, minus
    // order * (the prescribed gradient); orientation 0: the wall's own populations.  A helper node outside the real
    // nodes was refused when the simulation was set up (lb_binary.py).
    const int o = (int)(nk.code >> g.orient_shift);
    int hx = n.gx, hy = n.gy, hz = n.gz;
    if (o >= 1 && o <= 2 * L::dim) {
      int ex = 0, ey = 0, ez = 0;       // the normal: a chain of selects (a table indexed at run time would live in LDS)
      static_for<1, 2 * L::dim + 1>([&](auto O) {
        if (o == O) { ex = L::ex(O); ey = L::ey(O); ez = L::ez(O); }
      });
      hx += p.wall_order * ex;
      hy += p.wall_order * ey;
      hz += p.wall_order * ez;
      if (g.wrap[0]) hx = 1 + (hx - 1 + (g.lat_nx - 2)) % (g.lat_nx - 2);
      if (g.wrap[1]) hy = 1 + (hy - 1 + (g.lat_ny - 2)) % (g.lat_ny - 2);
      if (L::dim == 3 && g.wrap[2]) hz = 1 + (hz - 1 + (g.lat_nz - 2)) % (g.lat_nz - 2);
    }
    const bool inside = hx >= 1 && hx <= g.lat_nx - 2 && hy >= 1 && hy <= g.lat_ny - 2 && (L::dim == 2 || (hz >= 1 && hz <= g.lat_nz - 2));
    if (inside) p.phi[n.gi] = fe_density_at<L, R, PROP>(g, p.d_in, hx, hy, hz) - p.wall_shift;
  }
}

// K = 0: the fluid lattice (local relaxation time; stores v and the Laplacian), K = 1: the order parameter.
// ROW: one workgroup = one whole row, streaming through row_push(); every thread stays until the end (barrier inside).
template <class L, class R, int K, int PROP>
__global__ void __launch_bounds__(1024) fe_sweep_kernel(const FeParams<R> p) {
  constexpr bool ROW = L::dim == 3 && PROP != PROP_AA_EVEN;
  const Geometry& g = p.g;
  const int nx = g.lat_nx - 2;
  bool live;
  const ScNode n = sc_node<L>(g, p.y0, p.z0, nx, live, p.xcd_shift);
  NnKind nk;
  if (!nn_kind<ROW>(g, p.map, n.gi, live, nk)) return;
  const size_t ds = g.dist_size;
  const uint32_t lo = n.xi * (uint32_t)sizeof(R);

  R f[L::Q];
  sc_load<L, R, PROP>(f, p.d_in, ds, n);
  if (nk.wet) {
    const R phi = *at_byte(uniform_base((const R*)p.phi + n.row), lo);
    R fe[L::Q];
    R omega;
    if constexpr (K == 0) {
      R lap = (R)0, grad[3] = {(R)0, (R)0, (R)0};
      if (!fe_on_zero_rim<R>(p.rim, g, n.gx, n.gy, n.gz)) {
        fe_stencil<L, R>([&](auto I) { return *sc_neighbour<L, I>((const R*)p.phi, n, true); }, phi, lap, grad);
      }
      R rho, v[3];
      macro_standard<L, R>(f, false, rho, v);
      *at_byte(uniform_base(p.vx + n.row), lo) = v[0];
      *at_byte(uniform_base(p.vy + n.row), lo) = v[1];
      if constexpr (L::dim == 3) *at_byte(uniform_base(p.vz + n.row), lo) = v[2];
      *at_byte(uniform_base(p.lap + n.row), lo) = lap;
      if (p.options & 1u) *at_byte(uniform_base(p.rho + n.row), lo) = rho;
      fe_feq_fluid<L, R>(fe, rho, phi, lap, v, grad, p.A, p.kappa);
      omega = (R)1 / fe_tau0(phi, p.tau_a, p.tau_b);
    } else {
      const R lap = *at_byte(uniform_base((const R*)p.lap + n.row), lo);
      R v[3];
      v[0] = *at_byte(uniform_base((const R*)p.vx + n.row), lo);
      v[1] = *at_byte(uniform_base((const R*)p.vy + n.row), lo);
      v[2] = (R)0;
      if constexpr (L::dim == 3) v[2] = *at_byte(uniform_base((const R*)p.vz + n.row), lo);
      fe_feq_order<L, R>(fe, phi, lap, v, p.A, p.kappa, p.Gamma);
      omega = p.omega_phi;
    }
    static_for<0, L::Q>([&](auto I) { f[I] = f[I] + omega * (fe[I] - f[I]); });
  }
  if (nk.kind == NK_FULL_BB) bounce_back<L, R>(f);
  sc_store<L, R, PROP, true, ROW>(g, f, p.d_out, ds, n, nx, live, nk.active);
}

// Both lattices at their equilibria of the host's rho, phi, v on every node of the arrays; Laplacian and gradient of the
// host's phi on the real wet nodes (its ghost layer must be filled), zero on dry nodes, the ghost layer and the zero-gradient rims.
template <class L, class R>
__global__ void __launch_bounds__(256) fe_init_kernel(R* d1, R* d2, const R* __restrict__ irho, const R* __restrict__ iphi,
                                                     const R* __restrict__ ivx, const R* __restrict__ ivy,
                                                     const R* __restrict__ ivz, const FeParams<R> p) {
  const Geometry& g = p.g;
  const int gx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int gy = (int)blockIdx.y;
  const int gz = (int)blockIdx.z;
  if (gx > g.lat_nx - 1) return;
  const uint32_t gi = (uint32_t)gx + (uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz;
  const bool real = gx >= 1 && gx <= g.lat_nx - 2 && gy >= 1 && gy <= g.lat_ny - 2 && (L::dim == 2 || (gz >= 1 && gz <= g.lat_nz - 2));
  const R rho = irho[gi], phi = iphi[gi];
  R v[3] = {ivx[gi], ivy[gi], (R)0};
  if constexpr (L::dim == 3) v[2] = ivz[gi];
  R lap = (R)0, grad[3] = {(R)0, (R)0, (R)0};
  // dry nodes (walls: their stencil may reach into a ghost layer nothing fills) start without gradient terms as well
  const bool wet = !p.map || kind_is_wet(node_kind(g.type_lut, g.type_mask, p.map[gi]));
  if (real && wet && !fe_on_zero_rim<R>(p.rim, g, gx, gy, gz)) {
    const AxisOff ox = axis_off(gx, g.lat_nx, 1, g.wrap[0]);
    const AxisOff oy = axis_off(gy, g.lat_ny, g.arr_nx, g.wrap[1]);
    const AxisOff oz = (L::dim == 3) ? axis_off(gz, g.lat_nz, g.arr_nxy, g.wrap[2]) : AxisOff{0, 0};
    fe_stencil<L, R>([&](auto I) { return iphi[(uint32_t)((int)gi + dir_offset<L, I>(ox, oy, oz, true))]; }, phi, lap, grad);
  }
  R fe[L::Q];
  fe_feq_fluid<L, R>(fe, rho, phi, lap, v, grad, p.A, p.kappa);
  static_for<0, L::Q>([&](auto I) { (d1 + (size_t)g.dist_size * (size_t)I)[gi] = fe[I]; });
  fe_feq_order<L, R>(fe, phi, lap, v, p.A, p.kappa, p.Gamma);
  static_for<0, L::Q>([&](auto I) { (d2 + (size_t)g.dist_size * (size_t)I)[gi] = fe[I]; });
}

// ---------------------------------------------------------------------------
template <class R>
static FeParams<R> make_fe(const Geometry& g, const FreeEnergy& fe, const SweepArgs& a, int y0, int z0) {
  FeParams<R> p;
  p.map = (const uint32_t*)a.map;
  p.d_in = (const R*)a.dist_in;
  p.d_out = (R*)a.dist_out;
  p.rho = (R*)a.rho;
  p.phi = (R*)a.phi;
  p.vx = (R*)a.v[0];
  p.vy = (R*)a.v[1];
  p.vz = (R*)a.v[2];
  p.lap = (R*)a.lap;
  p.options = a.options;
  p.y0 = y0;
  p.z0 = z0;
  p.xcd_shift = 0;
  p.g = g;
  p.Gamma = (R)fe.Gamma;
  p.kappa = (R)fe.kappa;
  p.A = (R)fe.A;
  p.tau_a = (R)fe.tau_a;
  p.tau_b = (R)fe.tau_b;
  p.omega_phi = (R)(1.0 / fe.tau_phi);
  p.wall_shift = (R)((double)fe.wall_order * fe.wall_phase);
  p.wall_order = fe.wall_order;
  for (int i = 0; i < 3; i++) p.rim[i] = fe.rim[i];
  return p;
}

// a.dist_out: lattice 1 (read), a.phi: written
hipError_t launch_fe_macro(const Launch& lc, const FreeEnergy& fe, const SweepArgs& a) {
  const auto& [sel, prop, g, ph, y0, y1, z0, z1, block_x, s] = lc;
  return pick_lr(sel, [&](auto lr) {
    using L = typename decltype(lr)::L;
    using R = typename decltype(lr)::R;
    FeParams<R> p = make_fe<R>(g, fe, a, y0, z0);
    p.d_in = (const R*)a.dist_out;
    p.d_out = nullptr;
    const NNShape sh = nn_shape<L>(g, false, prop, y0, y1, z0, z1, nn_pass_block_x(g.lat_nx - 2));
    if (sh.empty) return hipSuccess;
    if (prop == PROP_AA_ODD) hipLaunchKernelGGL((fe_macro_kernel<L, R, PROP_AA_ODD>), sh.grid, sh.block, 0, s, p);
    else hipLaunchKernelGGL((fe_macro_kernel<L, R, PROP_AB>), sh.grid, sh.block, 0, s, p);
    return hipGetLastError();
  });
}

// which = 0: fluid lattice, 1: order parameter
hipError_t launch_fe_sweep(const Launch& lc, const FreeEnergy& fe, const SweepArgs& a, int which) {
  const auto& [sel, prop, g, ph, y0, y1, z0, z1, block_x, s] = lc;
  return pick_lr(sel, [&](auto lr) {
    using L = typename decltype(lr)::L;
    using R = typename decltype(lr)::R;
    FeParams<R> p = make_fe<R>(g, fe, a, y0, z0);
    const NNShape sh = nn_shape<L>(g, true, prop, y0, y1, z0, z1, block_x);      // the x-streaming steps in 3-D: whole rows
    if (sh.empty) return hipSuccess;
    p.xcd_shift = sh.xcd_shift;      // the stencil's phi rows: neighbouring rows on one XCD
    hipError_t e = hipErrorInvalidValue;
    pick<int, 0, 1>(which == 0 ? 0 : 1, [&](auto K) { pick_prop(prop, [&](auto P) {
      hipLaunchKernelGGL((fe_sweep_kernel<L, R, K, P>), sh.grid, sh.block, 0, s, p);
      e = hipGetLastError();
    }); });
    return e;
  });
}

hipError_t launch_fe_init(const KernelSelector& sel, const Geometry& g, const FreeEnergy& fe, void* dist1, void* dist2,
                          const void* rho, const void* phi, const void* const v[3], const void* map, hipStream_t s) {
  return pick_lr(sel, [&](auto lr) {
    using L = typename decltype(lr)::L;
    using R = typename decltype(lr)::R;
    SweepArgs a = {};
    a.map = map;
    const FeParams<R> p = make_fe<R>(g, fe, a, 0, 0);
    const dim3 grid((g.lat_nx + 255) / 256, g.lat_ny, g.lat_nz);
    hipLaunchKernelGGL((fe_init_kernel<L, R>), grid, dim3(256, 1, 1), 0, s, (R*)dist1, (R*)dist2, (const R*)rho, (const R*)phi,
                       (const R*)v[0], (const R*)v[1], (const R*)v[2], p);
    return hipGetLastError();
  });
}

}  // namespace slf
