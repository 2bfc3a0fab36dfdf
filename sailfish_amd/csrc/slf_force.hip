// Momentum-exchange force on bodies (C ABI slf_force_*; host surface lb_base.ForceObject, SubdomainRunner.update_force_objects).
//
// A link is a solid node s, a direction i and the fluid node f = s + e_i.  After propagation the momentum the link hands to
// the body is (dist[opp(i)][s] + dist[i][f]) e_opp(i) (Ladd's momentum exchange; the reference's ForceObject: kernel
// ComputeForceObjects, templates/kernel_force_objects.mako, copies the bracket of every link to the host, which multiplies
// by e_opp(i) and sums).  Here the bracket is formed in the module's precision as there, widened to double, multiplied by
// the three components of e_opp(i) (-1, 0, 1: exact) and summed on the device: all objects of a subdomain in one call,
// object o owning the links seg[o] .. seg[o + 1] - 1, three doubles per object.
//
// The caller hands in the two word indices of every link (into the distribution array of lattice 0: two-copy or in-place
// pattern, dense or indirect addressing are all the same to the kernel) and its direction as one byte.  Sums are formed
// without floating-point atomics in an order that the link tables alone fix: lane (links t, t + 1024, ... of a chunk of
// FORCE_CHUNK links) -> wave -> workgroup (slf_reduce.h) -> one partial per chunk -> chunks in index order.  The chunks of
// an object are cut from its own first link, so its sum does not depend on the other objects of the call.
#include <algorithm>

#include "slf_dispatch.h"
#include "slf_kernels.h"
#include "slf_lattice.h"
#include "slf_reduce.h"

namespace slf {

namespace {

constexpr int FORCE_BLOCK = 1024;

// grid (chunks of the longest object, objects); dst[3 * (object * chunks + chunk) + component].  With one chunk per object
// dst is the result itself and nothing follows.
template <class L, class R>
__global__ void __launch_bounds__(FORCE_BLOCK) force_objects_kernel(const R* __restrict__ dist, const uint32_t* __restrict__ idx,
                                                                    const uint32_t* __restrict__ idx2,
                                                                    const uint8_t* __restrict__ dir,
                                                                    const uint32_t* __restrict__ seg, double* __restrict__ dst) {
  __shared__ double red[3 * (FORCE_BLOCK / 64)];
  const uint32_t o = blockIdx.y, c = blockIdx.x;
  const uint32_t first = seg[o], end = seg[o + 1];
  const uint32_t nchunks = (end - first + FORCE_CHUNK - 1) / FORCE_CHUNK;
  if (c > 0 && c >= nchunks) return;          // (the whole workgroup; chunk 0 of an object without links stores zeros)
  const uint32_t lo = first + c * FORCE_CHUNK, hi = min(lo + (uint32_t)FORCE_CHUNK, end);

  double acc[3] = {0.0, 0.0, 0.0};
  for (uint32_t l = lo + threadIdx.x; l < hi; l += FORCE_BLOCK) {
    const R m = dist[idx[l]] + dist[idx2[l]];
    const int d = dir[l];
    int cx = 0, cy = 0, cz = 0;
    static_for<1, L::Q>([&](auto I) {
      if (d == I) cx = L::ex(L::opp(I)), cy = L::ey(L::opp(I)), cz = L::ez(L::opp(I));
    });
    const double md = (double)m;
    acc[0] = acc[0] + md * (double)cx;
    acc[1] = acc[1] + md * (double)cy;
    acc[2] = acc[2] + md * (double)cz;
  }
  block_sum<3>(acc, red);
  if (threadIdx.x == 0) {
    double* p = dst + 3 * ((size_t)o * gridDim.x + c);
    p[0] = acc[0], p[1] = acc[1], p[2] = acc[2];
  }
}

// One thread per (object, component): adds the chunks of the object in index order.
__global__ void __launch_bounds__(256) force_finalize(const double* __restrict__ partial, const uint32_t* __restrict__ seg,
                                                      uint32_t grid_x, int n_objects, double* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, o = t / 3, k = t % 3;
  if (o >= (uint32_t)n_objects) return;
  const uint32_t nchunks = (seg[o + 1] - seg[o] + FORCE_CHUNK - 1) / FORCE_CHUNK;
  const double* src = partial + 3 * (size_t)o * grid_x + k;
  double s = src[0];
  for (uint32_t c = 1; c < nchunks; c++) s = s + src[3 * (size_t)c];
  out[3 * (size_t)o + k] = s;
}

}  // namespace

ForceShape force_shape(int n_objects, uint32_t max_links) {
  ForceShape sh{};
  sh.block = FORCE_BLOCK;
  sh.grid_x = (int)std::max<uint32_t>(1u, (max_links + FORCE_CHUNK - 1) / FORCE_CHUNK);
  sh.workspace_doubles = sh.grid_x > 1 ? (size_t)3 * sh.grid_x * (size_t)n_objects : 0;
  return sh;
}

hipError_t launch_force_objects(const KernelSelector& sel, const void* dist, const uint32_t* idx, const uint32_t* idx2,
                                const uint8_t* dir, const uint32_t* seg, int n_objects, uint32_t max_links,
                                double* workspace, double* out, hipStream_t s) {
  const ForceShape sh = force_shape(n_objects, max_links);
  const dim3 grid(sh.grid_x, n_objects, 1), block(sh.block, 1, 1);
  double* dst = sh.grid_x > 1 ? workspace : out;
  hipError_t e = pick_lr(sel, [&](auto lr) {
    using T = decltype(lr);
    hipLaunchKernelGGL((force_objects_kernel<typename T::L, typename T::R>), grid, block, 0, s, (const typename T::R*)dist, idx,
                       idx2, dir, seg, dst);
    return hipGetLastError();
  });
  if (e != hipSuccess || sh.grid_x == 1) return e;
  hipLaunchKernelGGL(force_finalize, dim3((3 * n_objects + 255) / 256), dim3(256), 0, s, (const double*)workspace, seg,
                     (uint32_t)sh.grid_x, n_objects, out);
  return hipGetLastError();
}

}  // namespace slf
