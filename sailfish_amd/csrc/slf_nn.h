// What the sweeps that read a neighbouring field or stream through row_push() share (binary / single-component Shan-Chen:
// slf_sc.hip; the ternary Shan-Chen mixture: slf_sc3.hip; the free-energy binary fluid: slf_fe.hip; D3Q15 / D3Q27:
// slf_lat.hip).  Per node, in the order a sweep uses them:
//   sc_node                          row and lane position
//   nn_kind                          the node's code and kind, whether it is swept at all and whether it collides
//   sc_load, sc_store                one lattice's populations in the three streaming modes
//   sc_neighbour                     cached read of a field at a neighbouring node
//   sc_psi, sc_with_potential        the pseudopotential
//   sc_stencil                       the stencil sum S_d of one field, of which every Shan-Chen force is made
//   sc_add_momentum                  one lattice's share of the common velocity
// and on the host nn_pass_block_x / nn_shape, the launch shape of every launcher of the four units.
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

// What a sweep does with a node once its position is known.  Without a node map every real node is a fluid node.  MAP: -1
// the pointer decides at run time (wave-uniform), else a kernel's compile-time GENERAL: 1 = there is a map, 0 = none.  (Not
// GENERAL ? p.map : nullptr with a test of the pointer: the branch that leaves in the GENERAL kernels cost the D3Q19 f32
// sc_sweep_kernels two VGPRs and a resident wave.)  ROW: one workgroup = one whole row streaming through row_push(); every
// thread stays until the end (barrier inside), excluded nodes and idle lanes are merely inactive.  Otherwise they leave:
// false = nothing to do for this lane.
struct NnKind {
  uint32_t code;      // the node map's entry (orientation: code >> g.orient_shift)
  int kind;
  bool active, wet;   // swept at all | collides
};
template <bool ROW, int MAP = -1>
__device__ __forceinline__ bool nn_kind(const Geometry& g, const uint32_t* map, uint32_t gi, bool live, NnKind& k) {
  if constexpr (!ROW) {
    if (!live) return false;
  }
  k.code = 0;
  k.kind = NK_FLUID;
  k.active = live;
  if (MAP > 0 || (MAP < 0 && map)) {
    k.code = map[gi];
    k.kind = node_kind(g.type_lut, g.type_mask, k.code);
    if constexpr (!ROW) {
      if (kind_is_excluded(k.kind)) return false;
    } else {
      k.active = live && !kind_is_excluded(k.kind);
    }
  }
  k.wet = kind_is_wet(k.kind) && k.active;
  return true;
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

// What an edge lane knows about its connected x face (sc_edge(), slf_sc.hip): which face, its receive plane, and where
// the stencil values of field 0 that sit across the face lie in it; those of field J lie J * fstride further on.
template <class L, class R>
struct ScEdge {
  bool lo, hi;
  const R* plane;
  int off[count_x_dirs<L>()];
  int fstride;
};

// S[d] += sum_i psi(field(x + e_i)) (+-w_i) over the directions with e_i,d != 0, i = 1 .. Q - 1: the neighbour values come
// through the caches (every value is used by Q - 1 nodes).  XF: n is the node sc_edge() made, whose own loads stay inside
// the row, and the values across the face come from the receive plane.  The one place this sum is written; the numpy
// twin tests/_scn_twin.py restates its order.
template <class L, class R, int POT, bool XF = false>
__device__ __forceinline__ void sc_stencil(const R* field, const ScNode& n, R (&S)[3], const ScEdge<L, R>* e = nullptr,
                                           int J = 0) {
  [[maybe_unused]] R ev[count_x_dirs<L>()];
  if constexpr (XF) {
    static_for<0, count_x_dirs<L>()>([&](auto K) { ev[K] = (R)0; });
    if (e->lo || e->hi) {
      static_for<0, count_x_dirs<L>()>([&](auto K) { ev[K] = e->plane[e->off[K] + J * e->fstride]; });
    }
  }
  static_for<1, L::Q>([&](auto I) {
    R nb = *sc_neighbour<L, I>(field, n, true);
    if constexpr (XF && L::ex(I) > 0) nb = e->hi ? ev[x_dir_rank<L, I>()] : nb;
    if constexpr (XF && L::ex(I) < 0) nb = e->lo ? ev[x_dir_rank<L, I>()] : nb;
    const R psi = sc_psi<R, POT>(nb);
    static_for<0, L::dim>([&](auto D) {
      constexpr int ec = e_comp<L>(I, D);
      if constexpr (ec > 0) S[D] = S[D] + psi * Weights<L, R>::w(I);
      if constexpr (ec < 0) S[D] = S[D] + psi * ((R)0 - Weights<L, R>::w(I));
    });
  });
}

// One lattice's share of the common velocity  sum_k j_k / tau_k  over  sum_k rho_k / tau_k  (binary_shan_chen.mako:69-83,
// ternary_shan_chen.mako:75-95): v = (1/tau_0) j_0, then v = v + (1/tau_k) j_k; the caller divides by the total.
template <class L, class R, bool FIRST>
__device__ __forceinline__ void sc_add_momentum(R (&v)[3], R omega, const R (&f)[L::Q]) {
  const R j0 = omega * momentum<L, R, 0>(f);
  const R j1 = omega * momentum<L, R, 1>(f);
  v[0] = FIRST ? j0 : v[0] + j0;
  v[1] = FIRST ? j1 : v[1] + j1;
  if constexpr (L::dim == 3) {
    const R j2 = omega * momentum<L, R, 2>(f);
    v[2] = FIRST ? j2 : v[2] + j2;
  }
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

// ---- host: the launch shape ----
// Block width of the pass kernels (densities, velocity): the whole row in one workgroup where it fits
static inline int nn_pass_block_x(int nx) {
  const int bx = ((nx + 63) / 64) * 64;
  return bx > 1024 ? 256 : bx;
}

// row: whole-row workgroups (or equal x-segments) + aligned stores for the x-streaming steps in 3-D (as slf_row.hip), where
// the caller's kernels have that form (row_ok); block_x is then the row's, not the caller's.  max_threads: the kernel's
// launch bound where it is below row_block_x()'s 1024 -- rows beyond it are cut into equal segments of whole waves that fit.
struct NNShape {
  dim3 grid, block;
  bool row, empty;
  int xcd_shift;      // rows that share field rows through the L2: neighbouring rows on one XCD (xcd_row(), slf_sweep.h)
};
template <class L>
static NNShape nn_shape(const Geometry& g, bool row_ok, Prop prop, int y0, int y1, int z0, int z1, int block_x,
                        int max_threads = 0) {
  const int nx = g.lat_nx - 2;
  NNShape sh;
  sh.row = row_ok && L::dim == 3 && prop != PROP_AA_EVEN;
  if (sh.row) block_x = row_block_x(nx);
  if (max_threads && block_x > max_threads) {
    const int waves = (nx + 63) / 64, per = max_threads / 64;
    const int nseg = (waves + per - 1) / per;
    block_x = sh.row ? ((waves + nseg - 1) / nseg) * 64 : max_threads;
  }
  sh.block = dim3(block_x, 1, 1);
  sh.grid = dim3((nx + block_x - 1) / block_x, y1 - y0, L::dim == 3 ? z1 - z0 : 1);
  sh.empty = sh.grid.y == 0 || sh.grid.z == 0;
  sh.xcd_shift = xcd_shift_for(sh.grid.y, sh.grid.x);
  return sh;
}

}  // namespace slf
