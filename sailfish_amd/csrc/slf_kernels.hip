// gfx950 (MI355X, CDNA4) kernels of the Sailfish hot path.
//
//   sweep_kernel      fused collide-and-stream  = reference CollideAndPropagate
//                     (sailfish/templates/models/lb_single_fluid.mako:161-229)
//   init_kernel       SetInitialConditions      (lb_single_fluid.mako:101-127)                 } slf_plain.h, shared
//   pbc_kernel        ApplyPeriodicBoundaryConditions[WithSwap] (kernel_utils.mako:19-384)     } with slf_lat.hip
//   macro_pbc_kernel  ApplyMacroPeriodicBoundaryConditions      (kernel_utils.mako:410-474)
//   sparse_kernel     Collect/DistributeSparseData              (kernel_utils.mako:796-836)
//
// Design: bandwidth-bound stencil, no MFMA.  SoA layout
// dist[q][z][y][x] with x padded (reference subdomain_runner.py:367-373), one
// thread per node along x so that every population access of a wave is one
// contiguous 256-byte row segment; a workgroup owns a contiguous x-chunk of one
// (y, z) row, so y/z neighbour offsets (and the periodic wrap of those axes) are
// wave-uniform scalars and only the +-1 x shift is per lane.  Streaming is
// "push" for AB and the odd AA step, in-place opposite-slot for the even AA step
// (reference propagation.mako:170-174, 384-421; geo_helpers.mako:248-276).
#include "../../include/sailfish_hip.h"
#include "slf_dispatch.h"
#include "slf_kernels.h"
#include "slf_node.h"
#include "slf_plain.h"
#include "slf_sweep.h"

namespace slf {

// V: the variant (SweepVariant, slf_variant.h).  Which ones are instantiated: per_node_variant_exists(); launched iff the
// module's run-time values name them (per_node_variant_of(), launch_sweep2); the launch bound: sweep_max_threads().
// V.accf: the node's acceleration is cp.accel + field[d][gi], one coalesced load per dimension next to the population
// loads, live across the collision.
template <class L, class R, SweepVariant V>
__global__ void __launch_bounds__(sweep_max_threads(V)) sweep_kernel(const SweepParams<L, R> p) {
  const Geometry& g = p.g;
  const int gy = p.y0 + (int)blockIdx.y;
  const int gz = (L::dim == 3) ? p.z0 + (int)blockIdx.z : 0;
  // thread 0 of a row owns the first *real* node (x = 1): with the distribution arrays allocated so that
  // x = 1 sits on a 128-byte boundary (backend alloc_buf(align_offset=...)), every wave's row segment
  // is line aligned
  const int gx = 1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (gx > g.lat_nx - 2) return;

  const uint32_t gi = (uint32_t)gx + (uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz;

  // indirect addressing (reference kernel_common.mako:140-167): the distribution arrays hold active
  // nodes only; si = slot of this node, neighbours are translated through the same dense table
  uint32_t si = gi;
  if constexpr (V.indirect) {
    si = p.nodes[gi];
    if (si == INVALID_NODE) return;
  }
  int kind = NK_FLUID;
  uint32_t code = 0;
  if constexpr (V.general) {
    code = p.map[gi];
    kind = node_kind(g.type_lut, g.type_mask, code);
    if (kind_is_excluded(kind)) return;
  }

  const AxisOff ox = axis_off(gx, g.lat_nx, 1, g.wrap[0]);
  const AxisOff oy = axis_off(gy, g.lat_ny, g.arr_nx, g.wrap[1]);
  const AxisOff oz = (L::dim == 3) ? axis_off(gz, g.lat_nz, g.arr_nxy, g.wrap[2]) : AxisOff{0, 0};
  const size_t ds = g.dist_size;

  // the acceleration field: issued in front of the population loads, so that all of them are in flight together
  R acc[3] = {(R)0, (R)0, (R)0};
  if constexpr (V.accf) {
    const size_t fs = (size_t)g.arr_nxy * (size_t)g.arr_nz;
    static_for<0, L::dim>([&](auto D) { acc[D] = (p.accf + fs * (size_t)D)[gi]; });
  }

  // ---- load (reference getDist, geo_helpers.mako:258-276)
  R f[L::Q];
  static_for<0, L::Q>([&](auto I) {
    if constexpr (V.prop == PROP_AA_ODD) {
      const int off = dir_offset<L, I>(ox, oy, oz, false);
      uint32_t sn = (uint32_t)((int)gi + off);
      if constexpr (V.indirect) sn = p.nodes[sn];
      f[I] = (!V.indirect || sn != INVALID_NODE) ? (p.din + ds * (size_t)L::opp(I))[sn] : (R)0;
    } else {
      f[I] = (p.din + ds * (size_t)I)[si];
    }
  });

  R rho, v[3];
  bool wet = true;
  if constexpr (V.accf) static_for<0, L::dim>([&](auto D) { acc[D] = p.cp.accel[D] + acc[D]; });
  node_update<L, R, V>(p, f, code, kind, gi, ox, oy, oz, rho, v, wet, si, V.accf ? &acc : nullptr);

  if (wet) check_invalid<R>(p.status, p.options, rho, gx, gy, gz);
  // ---- macroscopic output (save_macro_fields, kernel_common.mako:213-240)
  if ((p.options & 1u) && wet) {
    p.rho[gi] = rho;
    p.vx[gi] = v[0];
    p.vy[gi] = v[1];
    if constexpr (L::dim == 3) p.vz[gi] = v[2];
  }

  // ---- streaming (propagate, propagation.mako:384-421)
  static_for<0, L::Q>([&](auto I) {
    if constexpr (V.prop == PROP_AA_EVEN) {
      (p.dout + ds * (size_t)L::opp(I))[si] = f[I];
    } else {
      const int off = dir_offset<L, I>(ox, oy, oz, true);
      uint32_t t = (uint32_t)((int)gi + off);
      if constexpr (V.indirect) t = p.nodes[t];
      if (!V.indirect || t != INVALID_NODE) (p.dout + ds * (size_t)I)[t] = f[I];
    }
  });
}

// Ghost fill of a scalar field for one periodic axis (kernel_utils.mako:410-474).
template <class R>
__global__ void __launch_bounds__(256) macro_pbc_kernel(R* field, Geometry g, int axis) {
  const int lat[3] = {g.lat_nx, g.lat_ny, g.lat_nz};
  const int stride[3] = {1, g.arr_nx, g.arr_nxy};
  int b_ax, c_ax;
  if (axis == 0) { b_ax = 1; c_ax = 2; }
  else if (axis == 1) { b_ax = 0; c_ax = 2; }
  else { b_ax = 0; c_ax = 1; }
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int c = (int)blockIdx.y;
  if (b > lat[b_ax] - 1 || c > lat[c_ax] - 1) return;
  const int n = lat[axis];
  const uint32_t base = (uint32_t)b * (uint32_t)stride[b_ax] + (uint32_t)c * (uint32_t)stride[c_ax];
  const R hi = field[base + (uint32_t)((n - 2) * stride[axis])];
  if (slf_isfinite(hi)) field[base] = hi;
  const R lo = field[base + (uint32_t)stride[axis]];
  if (slf_isfinite(lo)) field[base + (uint32_t)((n - 1) * stride[axis])] = lo;
}

// Index-list gather / scatter of populations (halo pack / unpack).
template <class R, bool COLLECT>
__global__ void __launch_bounds__(256) sparse_kernel(const unsigned long long* __restrict__ idx, R* dist, R* buffer,
                                                     int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const unsigned long long gi = idx[i];
  if (gi == ~0ull) return;
  if constexpr (COLLECT) {
    buffer[i] = dist[gi];
  } else {
    // never-written ghost slots (pushed from excluded nodes) stay non-finite sentinels and are not
    // delivered -- the same policy as the periodic-boundary kernels (reference kernel_utils.mako:196,229)
    const R val = buffer[i];
    if (slf_isfinite(val)) dist[gi] = val;
  }
}

// Face pack / unpack without index lists (reference Collect/DistributeContinuousData, kernel_utils.mako:526-543,
// 629-645, 692-708, 777-793): the populations `dirs` (bit mask over q, ascending) of an ncols x nrows box of nodes
// base + c * col_stride + r * row_stride  <->  dense buffer [k][r][c].  z and y faces have col_stride = 1: every
// wave moves whole contiguous row segments; x faces (col_stride = arr_nx) are a strided gather / scatter, still
// without the 8 bytes of index per 4 bytes of payload of the sparse kernels.
template <class R, bool COLLECT>
__global__ void __launch_bounds__(256) box_kernel(R* dist, R* buffer, size_t dq, unsigned long long dirlist, unsigned long long base,
                                                  long long col_stride, int ncols, long long row_stride, int nrows,
                                                  long long buf_k_stride, long long buf_row_stride, int deliver_all) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int r = (int)blockIdx.y;
  if (c >= ncols) return;
  const int q = (int)((dirlist >> (5u * blockIdx.z)) & 31ull);  // the blockIdx.z-th direction of the list (5 bits each)
  R* node = dist + dq * (size_t)q + base + (size_t)((long long)c * col_stride + (long long)r * row_stride);
  R* slot = buffer + (size_t)blockIdx.z * (size_t)buf_k_stride + (size_t)r * (size_t)buf_row_stride + (size_t)c;
  if constexpr (COLLECT) {
    *slot = *node;
  } else {
    const R val = *slot;
    if (deliver_all || slf_isfinite(val)) *node = val;   // populations: sentinels are not delivered (as sparse_kernel / the PBC kernels)
  }
}

// dirs: the directions whose layers travel, in buffer order (at most 12, 5 bits each in the kernel argument).
hipError_t launch_box(const KernelSelector& sel, const Geometry& g, bool collect, void* dist, void* buffer,
                      const int* dirs, int nd, unsigned long long base, long long col_stride, int ncols, long long row_stride,
                      int nrows, long long buf_k_stride, long long buf_row_stride, bool deliver_all, hipStream_t s) {
  if (buf_k_stride <= 0) buf_k_stride = (long long)nrows * ncols;     // dense [k][r][c]
  if (buf_row_stride <= 0) buf_row_stride = ncols;
  if (nd <= 0 || ncols <= 0 || nrows <= 0) return hipSuccess;
  if (nd > 12) return hipErrorInvalidValue;
  unsigned long long dirlist = 0;
  for (int i = 0; i < nd; i++) dirlist |= (unsigned long long)(dirs[i] & 31) << (5 * i);
  dim3 block(256, 1, 1);
  dim3 grid((ncols + 255) / 256, nrows, nd);
  const size_t dq = g.dist_size;
  const int all = deliver_all ? 1 : 0;
  return pick_real(sel, [&](auto r) {
    using R = decltype(r);
    pick_bool(collect, [&](auto COLLECT) {
      hipLaunchKernelGGL((box_kernel<R, COLLECT>), grid, block, 0, s, (R*)dist, (R*)buffer, dq, dirlist, base, col_stride,
                         ncols, row_stride, nrows, buf_k_stride, buf_row_stride, all);
    });
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------

template <class L, class R>
static hipError_t launch_sweep2(LR<L, R>, const Launch& lc, const SweepArgs& a) {
  const auto& [sel, prop, g, ph, y0, y1, z0, z1, module_block_x, s] = lc;
  const SweepParams<L, R> p = make_params<L, R>(g, ph, a, y0, z0);
  const SweepVariant v = per_node_variant_of(sel, g, ph, prop);
  const int block_x = module_block_x > sweep_max_threads(v) ? sweep_max_threads(v) : module_block_x;      // the instantiation's launch bound
  dim3 block(block_x, 1, 1);
  dim3 grid((g.lat_nx - 2 + block_x - 1) / block_x, y1 - y0, L::dim == 3 ? z1 - z0 : 1);
  if (grid.y == 0 || grid.z == 0) return hipSuccess;
  if (ph.accel_field && !a.accf) return hipErrorInvalidValue;      // (slf_kernel_launch refuses first, with a message)
  if (!v.roundoff && !v.turb && v.model != 2 && g.indirect && p.slot_gi) {       // one thread per slot (slot_sweep_kernel)
    SweepParams<L, R> q = p;
    q.y1 = y1;
    q.z1 = (L::dim == 3) ? z1 : 1;
    return launch_slot_sweep<L, R>(v.model, prop, g.bc_level, q, s);      // slf_slots.hip
  }
  hipError_t e = hipErrorInvalidValue;      // stays if the run-time values name a variant that does not exist
  pick<int, 0, 1, 2>(v.model, [&](auto MODEL) { pick_prop(prop, [&](auto P) {
    pick_bool(v.general, [&](auto G) { pick_bool(v.indirect, [&](auto IND) {
      pick_bool(v.roundoff, [&](auto ROUNDOFF) { pick_bool(v.turb, [&](auto TURB) { pick_bool(v.tms, [&](auto TMS) {
      pick_bool(v.accf, [&](auto ACCF) { pick_bool(v.sw, [&](auto SW) {
        constexpr SweepVariant V{.model = MODEL, .prop = P, .general = G, .indirect = IND, .roundoff = ROUNDOFF, .turb = TURB,
                                 .tms = TMS, .accf = ACCF, .sw = SW};
        if constexpr (!per_node_variant_exists(L::id, V)) return;
        else {
          hipLaunchKernelGGL((sweep_kernel<L, R, V>), grid, block, 0, s, p);
          e = hipGetLastError();
        }
      }); });
      }); }); });
    }); });
  }); });
  return e;
}

hipError_t launch_sweep(const Launch& lc, const SweepArgs& a) {
  if (!lc.g.indirect) {   // the tuned kernels address the dense layout
    hipError_t fe = hipSuccess;
    if (launch_sweep_fast(lc.sel, lc.prop, lc.g, lc.ph, a, lc.y0, lc.y1, lc.z0, lc.z1, lc.block_x, lc.s, &fe)) return fe;
    if (launch_sweep_row(lc.sel, lc.prop, lc.g, lc.ph, a, lc.y0, lc.y1, lc.z0, lc.z1, lc.s, &fe)) return fe;
  }
  return pick_lr(lc.sel, [&](auto lr) { return launch_sweep2(lr, lc, a); });
}

hipError_t launch_init(const KernelSelector& sel, const Geometry& g, const Physics& ph, void* dist, const void* rho,
                       const void* const v[3], const void* nodes, hipStream_t s) {
  return pick_lr(sel, [&](auto lr) { return launch_init2(lr, g, ph, dist, rho, v, nodes, s); });
}

hipError_t launch_pbc(const KernelSelector& sel, const Geometry& g, void* dist, int axis, bool with_swap,
                      hipStream_t s) {
  if (axis < 0 || axis >= g.dim) return hipErrorInvalidValue;
  return pick_lr(sel, [&](auto lr) { return launch_pbc2(lr, g, dist, axis, with_swap, s); });
}

hipError_t launch_macro_pbc(const KernelSelector& sel, const Geometry& g, void* field, int axis, hipStream_t s) {
  if (axis < 0 || axis >= g.dim) return hipErrorInvalidValue;
  const int lat[3] = {g.lat_nx, g.lat_ny, g.lat_nz};
  int b_ax = (axis == 0) ? 1 : 0;
  int c_ax = (axis == 2) ? 1 : 2;
  dim3 block(256, 1, 1);
  dim3 grid((lat[b_ax] + 255) / 256, lat[c_ax], 1);
  return pick_real(sel, [&](auto r) {
    hipLaunchKernelGGL((macro_pbc_kernel<decltype(r)>), grid, block, 0, s, (decltype(r)*)field, g, axis);
    return hipGetLastError();
  });
}

hipError_t launch_sparse(const KernelSelector& sel, bool collect, const unsigned long long* idx, void* dist,
                         void* buffer, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  dim3 block(256, 1, 1);
  dim3 grid((n + 255) / 256, 1, 1);
  return pick_real(sel, [&](auto r) {
    using R = decltype(r);
    pick_bool(collect, [&](auto COLLECT) {
      hipLaunchKernelGGL((sparse_kernel<R, COLLECT>), grid, block, 0, s, idx, (R*)dist, (R*)buffer, n);
    });
    return hipGetLastError();
  });
}

hipError_t launch_macro(const Launch& lc, const SweepArgs& a) {
  return pick_lr(lc.sel, [&](auto lr) { return launch_macro2(lr, lc.prop, lc.sel.general, lc.g, lc.ph, a, lc.s); });
}

}  // namespace slf
