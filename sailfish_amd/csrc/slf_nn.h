// What the sweeps of the models with nearest-neighbour fields share (binary / single-component Shan-Chen: slf_sc.hip; the
// free-energy binary fluid: slf_fe.hip; the ternary Shan-Chen mixture: slf_sc3.hip): a node's row and lane position, the
// cached read of a field at a neighbouring node, the pseudopotential, and the loads and stores of one lattice's populations
// for the three streaming modes.
#pragma once
#include "slf_dispatch.h"
#include "slf_rowpush.h"

namespace slf {

// Cache hints for the populations: streamed once per kernel in 3-D (non-temporal); 2-D lattices live in the caches.
template <class L>
constexpr int sc_nt() { return L::dim == 3 ? 3 : 0; }

// A node's row and lane position, the way slf_row.hip addresses memory: everything that is the same for the whole
// workgroup (y, z, the row's first element, the y / z neighbour offsets) is pinned to SGPRs, so that every access is
// (uniform base) + (one shared 32-bit lane offset) -- see uniform_base(), slf_sweep.h.
struct ScNode {
  int gx, gy, gz;
  uint32_t row, xi, gi;
  AxisOff ox, oy, oz;
};
template <class L>
__device__ __forceinline__ ScNode sc_node(const Geometry& g, int y0, int z0, int nx, bool& live, int xcd_shift = 0) {
  ScNode n;
  // rows that share rho / phi rows through the L2 go to one XCD (xcd_row(), slf_sweep.h)
  const int by = xcd_row((int)blockIdx.y, xcd_shift);
  n.gy = sgpr(y0 + by);
  n.gz = (L::dim == 3) ? sgpr(z0 + (int)blockIdx.z) : 0;
  n.gx = 1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  live = n.gx <= nx;
  n.row = sgpr((uint32_t)g.arr_nx * (uint32_t)n.gy + (uint32_t)g.arr_nxy * (uint32_t)n.gz);
  n.xi = (uint32_t)(live ? n.gx : nx);      // idle lanes: an in-row address, never stored
  n.gi = n.row + n.xi;
  n.ox = axis_off(n.gx, g.lat_nx, 1, g.wrap[0]);
  n.oy = axis_off(n.gy, g.lat_ny, g.arr_nx, g.wrap[1]);
  n.oz = (L::dim == 3) ? axis_off(n.gz, g.lat_nz, g.arr_nxy, g.wrap[2]) : AxisOff{0, 0};
  n.oy.p = sgpr(n.oy.p); n.oy.m = sgpr(n.oy.m); n.oz.p = sgpr(n.oz.p); n.oz.m = sgpr(n.oz.m);
  return n;
}

// element (row + yz-offset of direction I, forward or backward) + (xi shifted along x) of a node-indexed array
template <class L, int I, class T>
__device__ __forceinline__ const SLF_GLOBAL T* sc_neighbour(const T* base, const ScNode& n, bool forward) {
  const AxisOff ox0 = {0, 0};
  const int off = dir_offset<L, I>(ox0, n.oy, n.oz, forward);          // y, z part: uniform
  constexpr int ex = L::ex(I);
  const int xs = (ex == 0) ? 0 : (((ex > 0) == forward) ? n.ox.p : n.ox.m);   // x part: per lane
  return at_byte(uniform_base(base + (uint32_t)((int)n.row + off)), (uint32_t)((int)n.xi + xs) * (uint32_t)sizeof(T));
}

template <class R, int POT>
__device__ __forceinline__ R sc_psi(R rho) {
  // sym.py:896-908: linear psi = rho; classic psi = 1 - exp(-rho)
  if constexpr (POT == 0) return rho;
  else if constexpr (sizeof(R) == 4) return 1.0f - expf(0.0f - rho);      // the reference's exp() on a float argument
  else return (R)1 - exp((R)0 - rho);
}

// The module's potential (a run-time constant of the launch) as a compile-time constant of `body`: ONE wave-uniform
// branch around a whole block of psi evaluations.  With the choice inside sc_psi() the compiler turned it into a select:
// every one of the 38 psi values of a node went through the 15-instruction expf sequence and was thrown away again when
// the potential is linear -- a third of the fused sweep's vector instructions (1577 per wave, the vector ALUs ~80 % busy:
// profiles/r05/sq_summary_shan_chen_before.txt).
template <class F>
__device__ __forceinline__ void sc_with_potential(int potential, F&& body) {
  if (potential == 0) body(std::integral_constant<int, 0>{});
  else body(std::integral_constant<int, 1>{});
}

// INDIRECT (reference subdomain_runner.py:829-878, kernel_common.mako:140-167; serves NNSubdomainRunner too): the
// distribution arrays hold the active nodes only; the node's own slot and the slots of its neighbours come from the
// dense table `nodes`, the fields rho / phi / v and the node map stay dense.
template <class L, class R, int PROP, bool INDIRECT = false>
__device__ __forceinline__ void sc_load(R (&f)[L::Q], const R* din, size_t ds, const ScNode& n,
                                        const uint32_t* nodes = nullptr, uint32_t si = 0) {
  if constexpr (INDIRECT) {
    static_for<0, L::Q>([&](auto I) {
      if constexpr (PROP == PROP_AA_ODD) {
        const uint32_t sn = nodes[(uint32_t)((int)n.gi + dir_offset<L, I>(n.ox, n.oy, n.oz, false))];
        f[I] = (sn != INVALID_NODE) ? (din + ds * (size_t)L::opp(I))[sn] : (R)0;
      } else {
        f[I] = (din + ds * (size_t)I)[si];
      }
    });
    return;
  }
  static_for<0, L::Q>([&](auto I) {
    if constexpr (PROP == PROP_AA_ODD) {
      constexpr int nt = (L::ex(I) != 0) ? (sc_nt<L>() & ~1) : sc_nt<L>();     // shifted pulls share their lines
      f[I] = ldg<nt>(sc_neighbour<L, I>(din + ds * (size_t)L::opp(I), n, false));
    } else {
      f[I] = ldg<sc_nt<L>()>(at_byte(uniform_base(din + ds * (size_t)I + n.row), n.xi * (uint32_t)sizeof(R)));
    }
  });
}

// the streaming part of a sweep: whole-row push (3-D x-streaming steps), own slots (even AA step), or per-node push
template <class L, class R, int PROP, bool GENERAL, bool ROW, bool INDIRECT = false>
__device__ __forceinline__ void sc_store(const Geometry& g, R (&f)[L::Q], R* dout, size_t ds, const ScNode& n, int nx,
                                         bool live, bool active, const uint32_t* nodes = nullptr, uint32_t si = 0) {
  if constexpr (INDIRECT) {
    static_for<0, L::Q>([&](auto I) {
      if constexpr (PROP == PROP_AA_EVEN) {
        (dout + ds * (size_t)L::opp(I))[si] = f[I];
      } else {
        const uint32_t t = nodes[(uint32_t)((int)n.gi + dir_offset<L, I>(n.ox, n.oy, n.oz, true))];
        if (t != INVALID_NODE) (dout + ds * (size_t)I)[t] = f[I];
      }
    });
  } else if constexpr (ROW && PROP != PROP_AA_EVEN) {
    row_push<L, R, GENERAL, sc_nt<L>()>(g, f, dout, ds, n.row, n.xi, n.gx, nx, live, active, n.oy, n.oz);
  } else {
    static_for<0, L::Q>([&](auto I) {
      if constexpr (PROP == PROP_AA_EVEN) {
        stg<sc_nt<L>()>(at_byte(uniform_base(dout + ds * (size_t)L::opp(I) + n.row), n.xi * (uint32_t)sizeof(R)), f[I]);
      } else {
        const int off = dir_offset<L, I>(n.ox, n.oy, n.oz, true);
        (dout + ds * (size_t)I)[(uint32_t)((int)n.gi + off)] = f[I];
      }
    });
  }
}

}  // namespace slf
