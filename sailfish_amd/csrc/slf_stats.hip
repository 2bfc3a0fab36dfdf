// Flow statistics on the device (C ABI slf_stats_*; host surface sailfish_amd/stats.py).
//
//   ke_enstrophy_kernel   v^2 and |curl v|^2 per node with both sums fused in = the reference's
//                         ComputeSquareVelocityAndVorticity (sailfish/templates/data_processing.mako:35-109) followed by
//                         its two GPUArray sums (stats.py:38-53)
//   profiles_kernel       the 22 sums per position along one axis the reference forms with five Reduce...64 passes per
//                         sample (templates/reynolds_statistics.mako, stats.py:193-220): f, f^2, f^3, f^4 of ux, uy, uz,
//                         rho and the six correlations, ux, uy, uz and rho read once
//
// Both read the module's field layout real[(nz+2)][(ny+2)][arr_nx] whose ghost layer holds +inf: no ghost value ever
// enters a result.  Sums are double, formed without floating-point atomics in an order that the launch shape fixes:
// lane -> wave (shuffle tree) -> workgroup (LDS, wave order) -> one partial per workgroup in a workspace -> a finalize
// launch that adds the partials in a fixed order.  Two calls on the same fields give the same bits.
//
// As in the sweeps (slf_kernels.hip) lanes run along x and thread 0 of a row owns x = 1, which the backend puts on a
// 128-byte line: every load of a wave is one aligned row segment, and the y / z neighbour offsets and the choice
// between central and one-sided differences along y and z are wave-uniform.
#include <algorithm>

#include "slf_dispatch.h"
#include "slf_kernels.h"
#include "slf_node.h"
#include "slf_reduce.h"

namespace slf {

namespace {

constexpr int KE_MAX_BLOCK = 1024;
constexpr int KE_FIN_BLOCK = 1024;
constexpr int KE_ROWS = 8;            // rows of one plane a workgroup of the energy pass takes
constexpr int PROF_BLOCK = 256;
constexpr int NSTAT = STATS_PROFILE_COUNT;

// (wave_sum / block_sum: slf_reduce.h)

// d f / d axis at a node of layer g (1 .. lat - 2) of that axis: central where both neighbours are real nodes of the
// subdomain, one-sided on its first / last real layer (data_processing.mako:61-102; numpy.gradient's first-order edges)
template <class R>
__device__ __forceinline__ R diff(const R* __restrict__ f, uint32_t gi, R own, int g, int lat, uint32_t stride) {
  if (g > 1 && g < lat - 2) return (f[gi + stride] - f[gi - stride]) * (R)0.5;
  if (g == lat - 2) return own - f[gi - stride];
  return f[gi + stride] - own;
}

// grid (x blocks, groups of KE_ROWS rows, lat_nz): a workgroup takes an x-stretch of KE_ROWS consecutive rows of one plane
// of the lattice box, ghost rows included (they only clear their part of the two output fields); a lane adds up its
// nodes in double, the workgroup reduces once.  partial[2 * workgroup + {0, 1}] = the workgroup's two sums.
template <class R>
__global__ void __launch_bounds__(KE_MAX_BLOCK) ke_enstrophy_kernel(const Geometry g, const uint32_t* __restrict__ map,
                                                                    const R* __restrict__ vx, const R* __restrict__ vy,
                                                                    const R* __restrict__ vz, R* __restrict__ v_sq,
                                                                    R* __restrict__ vort_sq, double* __restrict__ partial) {
  __shared__ double red[2 * (KE_MAX_BLOCK / 64)];
  const int gz = (int)blockIdx.z;
  const int gx = 1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const bool live = gx <= g.lat_nx - 2;
  const uint32_t blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int y0 = (int)blockIdx.y * KE_ROWS, y1 = min(y0 + KE_ROWS, g.lat_ny);

  double acc[2] = {0.0, 0.0};
  for (int gy = y0; gy < y1; gy++) {
    const uint32_t gi = (uint32_t)gx + (uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz;
    const bool ghost_row = gy == 0 || gy == g.lat_ny - 1 || gz == 0 || gz == g.lat_nz - 1;
    R usq = (R)0, wsq = (R)0;
    if (live && !ghost_row) {
      bool active = true;
      if (map) {
        const int kind = node_kind(g.type_lut, g.type_mask, map[gi]);
        active = !kind_is_excluded(kind);
      }
      if (active) {
        const R lvx = vx[gi], lvy = vy[gi], lvz = vz[gi];
        usq = (lvx * lvx + lvy * lvy) + lvz * lvz;
        const R duz_dy = diff(vz, gi, lvz, gy, g.lat_ny, (uint32_t)g.arr_nx);
        const R dux_dy = diff(vx, gi, lvx, gy, g.lat_ny, (uint32_t)g.arr_nx);
        const R duy_dz = diff(vy, gi, lvy, gz, g.lat_nz, (uint32_t)g.arr_nxy);
        const R dux_dz = diff(vx, gi, lvx, gz, g.lat_nz, (uint32_t)g.arr_nxy);
        const R duz_dx = diff(vz, gi, lvz, gx, g.lat_nx, 1u);
        const R duy_dx = diff(vy, gi, lvy, gx, g.lat_nx, 1u);
        const R wx = duz_dy - duy_dz;
        const R wy = dux_dz - duz_dx;
        const R wz = duy_dx - dux_dy;
        wsq = (wx * wx + wy * wy) + wz * wz;
      }
    }
    if (v_sq && live) {
      // the fields are 0 wherever they are not a node's value: excluded nodes and the whole ghost layer (the two ghost
      // columns of a row are cleared by the lanes next to them)
      v_sq[gi] = usq;
      vort_sq[gi] = wsq;
      if (gx == 1) v_sq[gi - 1] = (R)0, vort_sq[gi - 1] = (R)0;
      if (gx == g.lat_nx - 2) v_sq[gi + 1] = (R)0, vort_sq[gi + 1] = (R)0;
    }
    // the sums take the ROUNDED per-node values: the same bits whether or not the fields are stored
    acc[0] = acc[0] + (double)usq;
    acc[1] = acc[1] + (double)wsq;
  }
  block_sum<2>(acc, red);
  if (threadIdx.x == 0) partial[2 * blk] = acc[0], partial[2 * blk + 1] = acc[1];
}

// One workgroup: thread t adds the partials t, t + blockDim, ... in that order, then the workgroup sum.
__global__ void __launch_bounds__(KE_FIN_BLOCK) ke_enstrophy_finalize(const double* __restrict__ partial, uint32_t n,
                                                                      double* __restrict__ out2) {
  __shared__ double red[2 * (KE_FIN_BLOCK / 64)];
  double acc[2] = {0.0, 0.0};
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    acc[0] = acc[0] + partial[2 * i];
    acc[1] = acc[1] + partial[2 * i + 1];
  }
  block_sum<2>(acc, red);
  if (threadIdx.x == 0) out2[0] = acc[0], out2[1] = acc[1];
}

// The 22 terms of one node, formed as the reference's _compute_stats does (data_processing.mako:112-126): the field
// value converted to double, powers multiplied left to right, a correlation one product.
__device__ __forceinline__ void add_terms(double (&acc)[NSTAT], const double (&f)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double p2 = f[i] * f[i], p3 = p2 * f[i], p4 = p3 * f[i];
    acc[4 * i] = acc[4 * i] + f[i];
    acc[4 * i + 1] = acc[4 * i + 1] + p2;
    acc[4 * i + 2] = acc[4 * i + 2] + p3;
    acc[4 * i + 3] = acc[4 * i + 3] + p4;
  }
  acc[16] = acc[16] + f[0] * f[1];
  acc[17] = acc[17] + f[0] * f[2];
  acc[18] = acc[18] + f[1] * f[2];
  acc[19] = acc[19] + f[0] * f[3];
  acc[20] = acc[20] + f[1] * f[3];
  acc[21] = acc[21] + f[2] * f[3];
}

template <class R>
__device__ __forceinline__ void add_node(double (&acc)[NSTAT], const R* __restrict__ vx, const R* __restrict__ vy,
                                         const R* __restrict__ vz, const R* __restrict__ rho, uint32_t gi) {
  const double f[4] = {(double)vx[gi], (double)vy[gi], (double)vz[gi], (double)rho[gi]};
  add_terms(acc, f);
}

// AXIS 0 (profile along x): grid (64-wide x blocks, chunks); a lane owns one x, the four waves of a workgroup take the
// rows r = y + ny z of its chunk in turn (wave w: r0 + w, r0 + w + 4, ...), wave 0 adds the four; ws[chunk][22][nx].
// AXIS 1 / 2 (along y / z): grid (positions, chunks); a workgroup owns the rows of one position p whose other coordinate
// (z resp. y) lies in its chunk, lanes stride over x; ws[p][chunk][22].  A workgroup takes a chunk of rows, not one
// row, so that the 22 cross-lane reductions are paid once per chunk.
template <class R, int AXIS>
__global__ void __launch_bounds__(PROF_BLOCK) profiles_kernel(const Geometry g, const R* __restrict__ vx,
                                                              const R* __restrict__ vy, const R* __restrict__ vz,
                                                              const R* __restrict__ rho, double* __restrict__ ws,
                                                              int per_chunk) {
  const int nx = g.lat_nx - 2, ny = g.lat_ny - 2, nz = g.lat_nz - 2;
  const int chunk = (int)blockIdx.y;
  double acc[NSTAT];
#pragma unroll
  for (int k = 0; k < NSTAT; k++) acc[k] = 0.0;

  if constexpr (AXIS == 0) {
    constexpr int WAVES = PROF_BLOCK / 64;
    __shared__ double red[(WAVES - 1) * NSTAT * 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = (int)blockIdx.x * 64 + lane;
    const int r0 = chunk * per_chunk, r1 = min(r0 + per_chunk, ny * nz);
    if (x < nx) {
      for (int r = r0 + wave; r < r1; r += WAVES) {
        const int y = r % ny, z = r / ny;
        add_node<R>(acc, vx, vy, vz, rho,
                    (uint32_t)(x + 1) + (uint32_t)g.arr_nx * (uint32_t)(y + 1) + (uint32_t)g.arr_nxy * (uint32_t)(z + 1));
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int k = 0; k < NSTAT; k++) red[((wave - 1) * NSTAT + k) * 64 + lane] = acc[k];
    }
    __syncthreads();
    if (wave == 0 && x < nx) {
#pragma unroll
      for (int k = 0; k < NSTAT; k++) {
        double s = acc[k];
        for (int w = 0; w < WAVES - 1; w++) s = s + red[(w * NSTAT + k) * 64 + lane];
        ws[((size_t)chunk * NSTAT + k) * nx + x] = s;
      }
    }
  } else {
    __shared__ double red[NSTAT * (PROF_BLOCK / 64)];
    const int p = (int)blockIdx.x;
    const int nother = AXIS == 1 ? nz : ny;
    const int o0 = chunk * per_chunk, o1 = min(o0 + per_chunk, nother);
    for (int o = o0; o < o1; o++) {
      const int y = AXIS == 1 ? p : o, z = AXIS == 1 ? o : p;
      const uint32_t row = (uint32_t)g.arr_nx * (uint32_t)(y + 1) + (uint32_t)g.arr_nxy * (uint32_t)(z + 1);
      for (int x = (int)threadIdx.x; x < nx; x += (int)blockDim.x) add_node<R>(acc, vx, vy, vz, rho, row + (uint32_t)(x + 1));
    }
    block_sum<NSTAT>(acc, red);
    if (threadIdx.x == 0) {
      double* dst = ws + ((size_t)p * gridDim.y + chunk) * NSTAT;
#pragma unroll
      for (int k = 0; k < NSTAT; k++) dst[k] = acc[k];
    }
  }
}

// One thread per (statistic k, position p): adds the chunks in index order, out[k * out_stride + offset + p].
// ws element (p, c, k) at p * sp + c * sc + k * sk.
__global__ void __launch_bounds__(256) profiles_finalize(const double* __restrict__ ws, int n, int nchunks, size_t sp,
                                                         size_t sc, size_t sk, double* __restrict__ out, size_t out_stride,
                                                         size_t offset) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x), k = (int)blockIdx.y;
  if (p >= n) return;
  const double* src = ws + (size_t)p * sp + (size_t)k * sk;
  double s = src[0];
  for (int c = 1; c < nchunks; c++) s = s + src[(size_t)c * sc];
  out[(size_t)k * out_stride + offset + (size_t)p] = s;
}

int ke_block(const Geometry& g) { return std::min(KE_MAX_BLOCK, (g.lat_nx - 2 + 63) / 64 * 64); }

}  // namespace

StatsShape stats_ke_shape(const Geometry& g) {
  StatsShape s{};
  s.block = ke_block(g);
  s.grid_x = (g.lat_nx - 2 + s.block - 1) / s.block;
  s.chunks = (g.lat_ny + KE_ROWS - 1) / KE_ROWS;
  s.per_chunk = KE_ROWS;
  s.workspace_doubles = (size_t)2 * s.grid_x * s.chunks * g.lat_nz;
  return s;
}

// Some 2048 workgroups (32 waves per CU) where the lattice has that many rows, never fewer rows per chunk than one:
// a function of the lattice size alone, so the order of addition is too.
StatsShape stats_profiles_shape(const Geometry& g, int axis) {
  const int nx = g.lat_nx - 2, ny = g.lat_ny - 2, nz = g.lat_nz - 2;
  StatsShape s{};
  s.block = PROF_BLOCK;
  const int first = axis == 0 ? (nx + 63) / 64 : (axis == 1 ? ny : nz);
  const long long units = axis == 0 ? (long long)ny * nz : (axis == 1 ? nz : ny);   // rows resp. planes to share out
  const long long want = std::max(1LL, std::min(units, (long long)(2048 + first - 1) / first));
  s.per_chunk = (int)((units + want - 1) / want);
  s.chunks = (int)((units + s.per_chunk - 1) / s.per_chunk);
  s.grid_x = first;
  const int n = axis == 0 ? nx : (axis == 1 ? ny : nz);
  s.workspace_doubles = (size_t)n * s.chunks * NSTAT;
  return s;
}

hipError_t launch_stats_ke_enstrophy(const KernelSelector& sel, const Geometry& g, const void* map, const void* const v[3],
                                     void* v_sq, void* vort_sq, double* workspace, double* out2, hipStream_t s) {
  const StatsShape sh = stats_ke_shape(g);
  const dim3 grid(sh.grid_x, sh.chunks, g.lat_nz), block(sh.block, 1, 1);
  return pick_real(sel, [&](auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((ke_enstrophy_kernel<R>), grid, block, 0, s, g, (const uint32_t*)map, (const R*)v[0], (const R*)v[1],
                       (const R*)v[2], (R*)v_sq, (R*)vort_sq, workspace);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ke_enstrophy_finalize, dim3(1), dim3(KE_FIN_BLOCK), 0, s, (const double*)workspace,
                       (uint32_t)(sh.workspace_doubles / 2), out2);
    return hipGetLastError();
  });
}

hipError_t launch_stats_profiles(const KernelSelector& sel, const Geometry& g, int axis, const void* const v[3],
                                 const void* rho, double* workspace, double* out, size_t out_stride, size_t offset,
                                 hipStream_t s) {
  const StatsShape sh = stats_profiles_shape(g, axis);
  const int nx = g.lat_nx - 2, n = axis == 0 ? nx : (axis == 1 ? g.lat_ny - 2 : g.lat_nz - 2);
  const dim3 grid(sh.grid_x, sh.chunks, 1), block(sh.block, 1, 1);
  hipError_t e = pick_real(sel, [&](auto r) {
    using R = decltype(r);
    pick<int, 0, 1, 2>(axis, [&](auto AXIS) {
      hipLaunchKernelGGL((profiles_kernel<R, AXIS>), grid, block, 0, s, g, (const R*)v[0], (const R*)v[1], (const R*)v[2],
                         (const R*)rho, workspace, sh.per_chunk);
    });
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  // axis x: ws[chunk][22][nx]; axes y, z: ws[p][chunk][22]
  const size_t sp = axis == 0 ? 1 : (size_t)sh.chunks * NSTAT;
  const size_t sc = axis == 0 ? (size_t)NSTAT * nx : NSTAT;
  const size_t sk = axis == 0 ? (size_t)nx : 1;
  hipLaunchKernelGGL(profiles_finalize, dim3((n + 255) / 256, NSTAT, 1), dim3(256), 0, s, (const double*)workspace, n,
                     sh.chunks, sp, sc, sk, out, out_stride, offset);
  return hipGetLastError();
}

}  // namespace slf
