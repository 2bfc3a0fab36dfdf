// Immersed boundary markers on the acceleration field (C ABI slf_ibm_*; host surface lb_single.LBIBMFluidSim,
// sailfish_amd/ibm.py, subdomain_runner.IBMSubdomainRunner).
//
// A marker p has a position x_p[d] in GLOBAL lattice coordinates (a node sits at integer coordinates), a reference
// position ref_p[d] and a stiffness k_p; arrays are [d][n] for positions, [n] for the stiffness, in the module's precision
// R.  The reference's templates/ibm.mako is a sketch (one z layer under a two-layer weight, positions used as array
// indices, floating-point atomics, float only): this file follows the semantics of DESIGN.md §9h, not its bits.
//
// ONE OPERATION ORDER (compiled with -ffp-contract=off; tests/_ibm_twin.py restates it in numpy):
//   i0[d]  = (int)floor(x_p[d])                                    node array index a[d] = i0[d] - origin[d] + 1 (+ 0 / 1)
//   stencil: the 2^dim nodes i0[d] + {0, 1}, z outermost, x innermost
//   w[d]   = (R)1 - fabs(x_p[d] - (R)i[d])                         i[d] the node's global coordinate
//   w      = wx * wy                     (2-D)        (wx * wy) * wz                     (3-D)
//   spread:  c = ((-k_p) * (x_p[d] - ref_p[d])) * w;   q = llrint((double)c * 2^48);   acc[d][gi] += q   (int64 atomic)
//   gather:  field[d][gi] = (R)((double)acc[d][gi] * 2^-48)
//   clear:   acc[d][gi] = 0, field[d][gi] = 0
//   advect:  v_p[d] = 0;  for the stencil nodes in order: v_p[d] = v_p[d] + w * (wet(gi) ? v[d][gi] : 0);  x_p[d] += v_p[d]
// Integer addition is associative: the accumulator, and with it the field, does not depend on the order in which the
// lanes arrive -- no floating-point atomics.  Markers that share a node store identical values in gather
// and clear.  A stencil node that is not a real node of the subdomain (1 <= a[d] <= lat_n[d] - 2) is skipped by spread,
// gather and clear; a marker that has one does not move and its word in `outside` is 1 (0 otherwise).  A position that is
// not finite or beyond +-2^30 counts as outside with all its nodes.  One lane per marker; every index is checked against
// the real nodes before it is used, so no launch reads or writes outside the arrays whatever the positions hold.
#include "slf_dispatch.h"
#include "slf_kernels.h"
#include "slf_lattice.h"
#include "slf_node.h"

namespace slf {

namespace {

constexpr double IBM_SCALE = 281474976710656.0;           // 2^48
constexpr double IBM_INV_SCALE = 1.0 / 281474976710656.0;

struct IbmGeo {
  int lat[3], arr_nx, arr_nxy;
  int origin[3];
  size_t field_stride;         // arr_nx * arr_ny * arr_nz
};

// The stencil of one marker: base array index per axis, validity per axis and offset, the two weights per axis.
template <int DIM, class R>
struct IbmStencil {
  int a0[3];
  bool ok[3][2];
  R w[3][2];
  bool inside;                 // every stencil node is a real node

  __device__ __forceinline__ IbmStencil(const IbmGeo& g, const R* __restrict__ pos, int n, int p) {
    inside = true;
    static_for<0, 3>([&](auto D) {
      a0[D] = 1, ok[D][0] = true, ok[D][1] = false, w[D][0] = (R)1, w[D][1] = (R)0;      // (axes beyond DIM: one layer)
      if constexpr (decltype(D)::value < DIM) {
        const R x = pos[(size_t)D * (size_t)n + (size_t)p];
        const bool finite = x >= (R)-1073741824.0 && x <= (R)1073741824.0;      // false for NaN
        const R fl = floor(finite ? x : (R)0);
        const int i0 = (int)fl;
        a0[D] = i0 - g.origin[D] + 1;
        static_for<0, 2>([&](auto O) {
          const int a = a0[D] + O;
          ok[D][O] = finite && a >= 1 && a <= g.lat[D] - 2;
          w[D][O] = (R)1 - fabs(x - (R)(i0 + O));
          inside = inside && ok[D][O];
        });
      }
    });
  }

  // f(gi, w) for every stencil node that is a real node, z outermost, x innermost
  template <class F>
  __device__ __forceinline__ void each(const IbmGeo& g, F&& f) const {
    for (int oz = 0; oz < (DIM == 3 ? 2 : 1); oz++) {
      for (int oy = 0; oy < 2; oy++) {
        for (int ox = 0; ox < 2; ox++) {
          if (!(ok[0][ox] && ok[1][oy] && ok[2][oz])) continue;
          R wt = w[0][ox] * w[1][oy];
          if constexpr (DIM == 3) wt = wt * w[2][oz];
          const uint32_t gi = (uint32_t)(a0[0] + ox) + (uint32_t)g.arr_nx * (uint32_t)(a0[1] + oy) +
                              (uint32_t)g.arr_nxy * (uint32_t)(DIM == 3 ? a0[2] + oz : 0);
          f(gi, wt);
        }
      }
    }
  }
};

constexpr int IBM_BLOCK = 128;

template <int DIM, class R>
__global__ void __launch_bounds__(IBM_BLOCK) ibm_spread_kernel(const IbmGeo g, int n, const R* __restrict__ pos,
                                                               const R* __restrict__ ref, const R* __restrict__ stiff,
                                                               long long* __restrict__ acc) {
  const int p = blockIdx.x * IBM_BLOCK + threadIdx.x;
  if (p >= n) return;
  const IbmStencil<DIM, R> st(g, pos, n, p);
  const R nk = -stiff[p];
  R pull[DIM];
  static_for<0, DIM>([&](auto D) {
    const size_t o = (size_t)D * (size_t)n + (size_t)p;
    pull[D] = nk * (pos[o] - ref[o]);
  });
  st.each(g, [&](uint32_t gi, R wt) {
    static_for<0, DIM>([&](auto D) {
      const R c = pull[D] * wt;
      const long long q = llrint((double)c * IBM_SCALE);
      atomicAdd((unsigned long long*)(acc + g.field_stride * (size_t)D + gi), (unsigned long long)q);
    });
  });
}

template <int DIM, class R>
__global__ void __launch_bounds__(IBM_BLOCK) ibm_gather_kernel(const IbmGeo g, int n, const R* __restrict__ pos,
                                                               const long long* __restrict__ acc, R* __restrict__ field) {
  const int p = blockIdx.x * IBM_BLOCK + threadIdx.x;
  if (p >= n) return;
  const IbmStencil<DIM, R> st(g, pos, n, p);
  st.each(g, [&](uint32_t gi, R) {
    static_for<0, DIM>([&](auto D) {
      const size_t o = g.field_stride * (size_t)D + gi;
      field[o] = (R)((double)acc[o] * IBM_INV_SCALE);
    });
  });
}

template <int DIM, class R>
__global__ void __launch_bounds__(IBM_BLOCK) ibm_clear_advect_kernel(const IbmGeo g, int n, R* __restrict__ pos,
                                                                     long long* __restrict__ acc, R* __restrict__ field,
                                                                     const uint32_t* __restrict__ map,
                                                                     unsigned long long type_lut, uint32_t type_mask,
                                                                     const R* __restrict__ vx, const R* __restrict__ vy,
                                                                     const R* __restrict__ vz, uint32_t* __restrict__ outside) {
  const int p = blockIdx.x * IBM_BLOCK + threadIdx.x;
  if (p >= n) return;
  const IbmStencil<DIM, R> st(g, pos, n, p);
  const R* v[3] = {vx, vy, vz};
  R vp[DIM];
  static_for<0, DIM>([&](auto D) { vp[D] = (R)0; });
  st.each(g, [&](uint32_t gi, R wt) {
    const bool wet = map ? kind_is_wet(node_kind(type_lut, type_mask, map[gi])) : true;
    static_for<0, DIM>([&](auto D) {
      const size_t o = g.field_stride * (size_t)D + gi;
      acc[o] = 0;
      field[o] = (R)0;
      const R vn = wet ? v[D][gi] : (R)0;
      vp[D] = vp[D] + wt * vn;
    });
  });
  outside[p] = st.inside ? 0u : 1u;
  if (!st.inside) return;
  static_for<0, DIM>([&](auto D) {
    const size_t o = (size_t)D * (size_t)n + (size_t)p;
    pos[o] = pos[o] + vp[D];
  });
}

IbmGeo ibm_geo(const Geometry& g, const int32_t origin[3]) {
  IbmGeo o{};
  o.lat[0] = g.lat_nx, o.lat[1] = g.lat_ny, o.lat[2] = g.lat_nz;
  o.arr_nx = g.arr_nx, o.arr_nxy = g.arr_nxy;
  for (int d = 0; d < 3; d++) o.origin[d] = origin[d];
  o.field_stride = (size_t)g.arr_nxy * (size_t)g.arr_nz;
  return o;
}

// f(std::integral_constant<int, DIM>, R{}) for the module's lattice and precision
template <class F>
hipError_t pick_dim_real(const KernelSelector& sel, F&& f) {
  return pick_lr(sel, [&](auto lr) {
    using T = decltype(lr);
    f(std::integral_constant<int, T::L::dim>{}, typename T::R{});
    return hipGetLastError();
  });
}

}  // namespace

size_t ibm_accumulator_bytes(const Geometry& g) {
  return (size_t)g.dim * (size_t)g.arr_nxy * (size_t)g.arr_nz * sizeof(long long);
}

hipError_t launch_ibm_spread(const KernelSelector& sel, const Geometry& g, const int32_t origin[3], int n, const void* pos,
                             const void* ref, const void* stiff, void* acc, hipStream_t s) {
  const IbmGeo ig = ibm_geo(g, origin);
  const dim3 grid((n + IBM_BLOCK - 1) / IBM_BLOCK), block(IBM_BLOCK);
  return pick_dim_real(sel, [&](auto DIM, auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((ibm_spread_kernel<decltype(DIM)::value, R>), grid, block, 0, s, ig, n, (const R*)pos, (const R*)ref, (const R*)stiff,
                       (long long*)acc);
  });
}

hipError_t launch_ibm_gather(const KernelSelector& sel, const Geometry& g, const int32_t origin[3], int n, const void* pos,
                             const void* acc, void* field, hipStream_t s) {
  const IbmGeo ig = ibm_geo(g, origin);
  const dim3 grid((n + IBM_BLOCK - 1) / IBM_BLOCK), block(IBM_BLOCK);
  return pick_dim_real(sel, [&](auto DIM, auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((ibm_gather_kernel<decltype(DIM)::value, R>), grid, block, 0, s, ig, n, (const R*)pos, (const long long*)acc, (R*)field);
  });
}

hipError_t launch_ibm_clear_and_advect(const KernelSelector& sel, const Geometry& g, const int32_t origin[3], int n, void* pos,
                                       void* acc, void* field, const void* map, const void* const v[3], uint32_t* outside,
                                       hipStream_t s) {
  const IbmGeo ig = ibm_geo(g, origin);
  const dim3 grid((n + IBM_BLOCK - 1) / IBM_BLOCK), block(IBM_BLOCK);
  return pick_dim_real(sel, [&](auto DIM, auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((ibm_clear_advect_kernel<decltype(DIM)::value, R>), grid, block, 0, s, ig, n, (R*)pos, (long long*)acc, (R*)field,
                       (const uint32_t*)map, g.type_lut, g.type_mask, (const R*)v[0], (const R*)v[1], (const R*)v[2], outside);
  });
}

}  // namespace slf
