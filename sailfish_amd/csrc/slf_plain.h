// The kernels of a single-fluid module that are written once for every lattice and take it as a template argument: the
// initial conditions, the ghost-layer periodic boundary conditions and the pass that stores density and velocity.
// Instantiated for D2Q9 and D3Q19 by slf_kernels.hip and for D3Q15 and D3Q27 by slf_lat.hip.
#pragma once
#include "../../include/sailfish_hip.h"
#include "slf_dispatch.h"
#include "slf_kernels.h"
#include "slf_node.h"
#include "slf_sweep.h"

namespace slf {

// SetInitialConditions: f_i = feq_i(rho, v) on *every* node of the lattice box,
// no type test (ghost nodes carry the non-finite sentinels of the host fields).
// SW: a shallow-water module (slf_module_desc::equilibrium): f = sw_equilibrium(h = rho, v, gravity), slf_node.h.  The switch
// is a second kernel, not a template argument of init_kernel, whose name -- and with it the device code of slf_lat.hip,
// which instantiates this header for D3Q15 and D3Q27 -- stays what it was; launch_init2 names it for D2Q9 only.
template <class L, class R>
__global__ void __launch_bounds__(256) init_kernel_sw(R* dist, const R* __restrict__ irho, const R* __restrict__ ivx,
                                                      const R* __restrict__ ivy, Geometry g, R gravity) {
  const int gx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int gy = (int)blockIdx.y;
  if (gx > g.lat_nx - 1) return;
  const uint32_t gi = (uint32_t)gx + (uint32_t)g.arr_nx * (uint32_t)gy;
  const R v[3] = {ivx[gi], ivy[gi], (R)0};
  R fe[L::Q];
  sw_equilibrium<L, R>(fe, irho[gi], v, gravity);
  static_for<0, L::Q>([&](auto I) { (dist + (size_t)g.dist_size * (size_t)I)[gi] = fe[I]; });
}

template <class L, class R>
__global__ void __launch_bounds__(256) init_kernel(R* dist, const R* __restrict__ irho, const R* __restrict__ ivx,
                                                   const R* __restrict__ ivy, const R* __restrict__ ivz, Geometry g,
                                                   int incompressible, const uint32_t* __restrict__ nodes) {
  const int gx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int gy = (int)blockIdx.y;
  const int gz = (int)blockIdx.z;
  if (gx > g.lat_nx - 1) return;
  const uint32_t gi = (uint32_t)gx + (uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz;
  uint32_t si = gi;   // indirect addressing: slot of this node, if it is active
  if (nodes) {
    si = nodes[gi];
    if (si == INVALID_NODE) return;
  }
  // incompressible = the module's density model: SLF_DENSITY_ROUNDOFF stores f_i - w_i (lb_single_fluid.mako:113)
  const R rho = (incompressible == SLF_DENSITY_ROUNDOFF) ? irho[gi] - (R)1 : irho[gi];
  R v[3];
  v[0] = ivx[gi];
  v[1] = ivy[gi];
  v[2] = (R)0;
  if constexpr (L::dim == 3) v[2] = ivz[gi];
  const R rho0 = (incompressible == SLF_DENSITY_ROUNDOFF) ? rho + (R)1 : (incompressible ? (R)1 : rho);
  const R u15 = usq15<L, R>(v);
  static_for<0, L::Q>([&](auto I) { (dist + (size_t)g.dist_size * (size_t)I)[si] = feq<L, R, I>(rho, rho0, v, u15); });
}

__device__ __forceinline__ bool slf_isfinite(float x) { return __builtin_isfinite(x); }
__device__ __forceinline__ bool slf_isfinite(double x) { return __builtin_isfinite(x); }

// Which face nodes take part in the PBC copy of `axis`, judged along another axis b
// (coordinate c, population component e, mode of b: 0 not locally periodic, 1 ghost-layer
// PBC, 2 wrapped in-sweep; `earlier` = b is handled before `axis` in the x, y, z order).
//
// After a push step a ghost slot holds data only if it was pushed from a real node:
// e = +1 -> c >= 2, e = -1 -> c <= lat-3.  Along a PBC axis handled earlier the wrapped
// copies already sit on real nodes; along a later PBC axis the ghost rows still hold the
// edge populations (they are moved on by that axis' kernel).  Ghost rows of axes that are
// not locally periodic belong to walls or to other subdomains (halo exchange) and never
// take part; along an in-sweep wrapped axis there are no ghost rows at all.
__device__ __forceinline__ bool pbc_push_ok(int c, int e, int lat, int mode, bool earlier) {
  const bool real = c >= 1 && c <= lat - 2;
  if (mode == 2) return real;
  if (mode == 1 && earlier) return real;
  const bool pushed = (e > 0) ? c >= 2 : ((e < 0) ? c <= lat - 3 : real);
  if (mode == 1) return pushed;
  return real && pushed;
}

// Swap variant (ghost <- opposite real layer, for the pull of the next step): along a PBC
// axis handled earlier the already filled ghost columns take part when the pulling node
// (at c + e) is real; everything else contributes its real range only.
__device__ __forceinline__ bool pbc_pull_ok(int c, int e, int lat, int mode, bool earlier) {
  if (mode == 1 && earlier) return c + e >= 1 && c + e <= lat - 2;
  return c >= 1 && c <= lat - 2;
}

// Periodic boundary conditions inside one subdomain for one axis.
//
// !SWAP (after a push step; effect of kernel_utils.mako:295-336): populations
// that were pushed into the ghost layer of `axis` are moved to the real layer on
// the opposite side.  Applied in x, y, z order this moves edge/corner populations
// one axis at a time (see pbc_push_ok for which face nodes take part);
// non-finite values (never-written ghost slots) are skipped.
//
// SWAP (after the in-place even AA step; effect of kernel_utils.mako:343-384):
// real layer -> opposite ghost layer, opposite slots, so that the next (odd)
// step can pull through the periodic face.  Axes already processed (lower
// index) contribute their ghost columns, later axes only their real range.
template <class L, class R, bool SWAP>
__global__ void __launch_bounds__(256) pbc_kernel(R* dist, Geometry g, int axis) {
  const int lat[3] = {g.lat_nx, g.lat_ny, g.lat_nz};
  const int stride[3] = {1, g.arr_nx, g.arr_nxy};
  int b_ax, c_ax;  // the two other axes, b fastest
  if (axis == 0) { b_ax = 1; c_ax = 2; }
  else if (axis == 1) { b_ax = 0; c_ax = 2; }
  else { b_ax = 0; c_ax = 1; }
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int c = (L::dim == 3) ? (int)blockIdx.y : 0;
  if (b > lat[b_ax] - 1) return;
  if (L::dim == 2) c_ax = 2;  // lat_nz == 1, c == 0

  const int n = lat[axis];
  const size_t ds = g.dist_size;
  const uint32_t base = (uint32_t)b * (uint32_t)stride[b_ax] + (uint32_t)c * (uint32_t)stride[c_ax];

  static_for<1, L::Q>([&](auto I) {
    const int e[3] = {L::ex(I), L::ey(I), L::ez(I)};
    const int ea = e[axis];
    if (ea == 0) return;
    const int eb = e[b_ax];
    const int ec = (L::dim == 3) ? e[c_ax] : 0;
    if constexpr (!SWAP) {
      if (!pbc_push_ok(b, eb, lat[b_ax], g.axis_mode[b_ax], b_ax < axis)) return;
      if (L::dim == 3) {
        if (!pbc_push_ok(c, ec, lat[c_ax], g.axis_mode[c_ax], c_ax < axis)) return;
      }
      // ea = -1: landed in the low ghost (0) -> high real (n-2); ea = +1: high ghost (n-1) -> low real (1)
      const uint32_t src = base + (uint32_t)((ea < 0 ? 0 : n - 1) * stride[axis]);
      const uint32_t dst = base + (uint32_t)((ea < 0 ? n - 2 : 1) * stride[axis]);
      R* d = dist + ds * (size_t)I;
      const R val = d[src];
      if (slf_isfinite(val)) d[dst] = val;
    } else {
      if (!pbc_pull_ok(b, eb, lat[b_ax], g.axis_mode[b_ax], b_ax < axis)) return;
      if (L::dim == 3) {
        if (!pbc_pull_ok(c, ec, lat[c_ax], g.axis_mode[c_ax], c_ax < axis)) return;
      }
      // ea = +1: puller at 1 reads ghost 0 <- real n-2 ; ea = -1: puller at n-2 reads ghost n-1 <- real 1
      const uint32_t src = base + (uint32_t)((ea > 0 ? n - 2 : 1) * stride[axis]);
      const uint32_t dst = base + (uint32_t)((ea > 0 ? 0 : n - 1) * stride[axis]);
      R* d = dist + ds * (size_t)L::opp(I);
      const R val = d[src];
      if (slf_isfinite(val)) d[dst] = val;
    }
  });
}

// PrepareMacroFields-style pass: density/velocity of every wet node without
// collision or streaming (lb_single_fluid.mako:129-159, used for output of
// the current state, e.g. right after initialisation or a restore).
template <class L, class R, int PROP, bool GENERAL>
__global__ void __launch_bounds__(1024) macro_kernel(const SweepParams<L, R> p) {
  const Geometry& g = p.g;
  const int gy = p.y0 + (int)blockIdx.y;
  const int gz = (L::dim == 3) ? p.z0 + (int)blockIdx.z : 0;
  const int gx = 1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (gx > g.lat_nx - 2) return;
  const uint32_t gi = (uint32_t)gx + (uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz;
  int kind = NK_FLUID;
  if constexpr (GENERAL) {
    const uint32_t code = p.map[gi];
    kind = node_kind(g.type_lut, g.type_mask, code);
    if (!kind_is_wet(kind)) return;
  }
  const AxisOff ox = axis_off(gx, g.lat_nx, 1, g.wrap[0]);
  const AxisOff oy = axis_off(gy, g.lat_ny, g.arr_nx, g.wrap[1]);
  const AxisOff oz = (L::dim == 3) ? axis_off(gz, g.lat_nz, g.arr_nxy, g.wrap[2]) : AxisOff{0, 0};
  const size_t ds = g.dist_size;
  const uint32_t* nodes = p.nodes;
  uint32_t si = gi;
  if (nodes) {
    si = nodes[gi];
    if (si == INVALID_NODE) return;
  }
  R f[L::Q];
  static_for<0, L::Q>([&](auto I) {
    if constexpr (PROP == PROP_AA_ODD) {
      const int off = dir_offset<L, I>(ox, oy, oz, false);
      uint32_t sn = (uint32_t)((int)gi + off);
      if (nodes) sn = nodes[sn];
      f[I] = (sn != INVALID_NODE) ? (p.din + ds * (size_t)L::opp(I))[sn] : (R)0;
    } else {
      f[I] = (p.din + ds * (size_t)I)[si];
    }
  });
  R rho, v[3];
  if (p.cp.incompressible == SLF_DENSITY_ROUNDOFF) macro_roundoff<L, R>(f, rho, v);
  else macro_standard<L, R>(f, p.cp.incompressible != 0, rho, v);
  p.rho[gi] = rho;
  p.vx[gi] = v[0];
  p.vy[gi] = v[1];
  if constexpr (L::dim == 3) p.vz[gi] = v[2];
}

template <class L, class R>
static hipError_t launch_init2(LR<L, R>, const Geometry& g, const Physics& ph, void* dist, const void* rho,
                               const void* const v[3], const void* nodes, hipStream_t s) {
  dim3 block(256, 1, 1);
  dim3 grid((g.lat_nx + 255) / 256, g.lat_ny, g.lat_nz);
  if (ph.equilibrium == SLF_EQ_SHALLOW_WATER) {      // D2Q9, direct addressing (module_config); no other lattice has the kernel
    if constexpr (L::id == D2Q9::id) {
      hipLaunchKernelGGL((init_kernel_sw<L, R>), grid, block, 0, s, (R*)dist, (const R*)rho, (const R*)v[0], (const R*)v[1], g,
                         (R)ph.gravity);
      return hipGetLastError();
    }
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL((init_kernel<L, R>), grid, block, 0, s, (R*)dist, (const R*)rho, (const R*)v[0], (const R*)v[1],
                     (const R*)v[2], g, ph.incompressible, (const uint32_t*)nodes);
  return hipGetLastError();
}

template <class L, class R>
static hipError_t launch_pbc2(LR<L, R>, const Geometry& g, void* dist, int axis, bool with_swap, hipStream_t s) {
  const int lat[3] = {g.lat_nx, g.lat_ny, g.lat_nz};
  int b_ax = (axis == 0) ? 1 : 0;
  int c_ax = (axis == 2) ? 1 : 2;
  dim3 block(256, 1, 1);
  dim3 grid((lat[b_ax] + 255) / 256, L::dim == 3 ? lat[c_ax] : 1, 1);
  pick_bool(with_swap, [&](auto SWAP) { hipLaunchKernelGGL((pbc_kernel<L, R, SWAP>), grid, block, 0, s, (R*)dist, g, axis); });
  return hipGetLastError();
}

template <class L, class R>
static hipError_t launch_macro2(LR<L, R>, Prop prop, bool general, const Geometry& g, const Physics& ph,
                                const SweepArgs& a, hipStream_t s) {
  const SweepParams<L, R> p = make_params<L, R>(g, ph, a, 1, L::dim == 3 ? 1 : 0);
  const int bx = 256;
  dim3 block(bx, 1, 1);
  dim3 grid((g.lat_nx - 2 + bx - 1) / bx, g.lat_ny - 2, L::dim == 3 ? g.lat_nz - 2 : 1);
  // two-copy and the even in-place step: the node's own slots
  pick<int, PROP_AB, PROP_AA_ODD>(prop == PROP_AA_ODD ? PROP_AA_ODD : PROP_AB, [&](auto P) {
    pick_bool(general, [&](auto G) { hipLaunchKernelGGL((macro_kernel<L, R, P, G>), grid, block, 0, s, p); });
  });
  return hipGetLastError();
}

}  // namespace slf
