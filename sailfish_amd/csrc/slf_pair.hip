// Two time steps per pass over memory for the two-copy (AB) sweep of the periodic D3Q19 / f32 / BGK box.
//
// fast_row_kernel (slf_fast.hip) streams the populations once per step at the rate of a plain copy: the only traffic
// left to remove is the round trip of the intermediate populations through HBM between step t and step t + 1.
// pair_row_kernel reads the populations of step t from the source copy, keeps what step t produces in registers, and
// writes the populations of step t + 2 to the other copy.
//
// One workgroup owns a strip of TY rows (y0 .. y0 + TY - 1) of zc planes (z0 .. z0 + zc - 1) and has one thread per x
// (blockDim.x = nx, a multiple of 64: the row is a ring of whole waves).  It marches along z; at plane k it
//   phase A  loads and collides the TY + 2 rows y0 - 1 .. y0 + TY of plane k (step t).  A post-collision value f_i of
//            row r belongs to row r + e_y, plane k + e_z of the intermediate state: it is filed there if that row is
//            one of the strip's own (the x shift is left for phase B);
//   phase B  (from the third plane on) plane k - 1 of the intermediate state is complete: for every own row the x shift
//            (one DPP move per direction, the wave-edge words through LDS), the collision of step t + 1 and the push to
//            the destination copy, exactly as fast_row_kernel's AB branch does it;
//   rotates  the three register planes.
// A thread holds, per own row, the 19 values of plane k - 1, the 14 (e_z >= 0) of plane k that have arrived and the 5
// (e_z = +1) of plane k + 1.  The halo rows and planes are collided again by the neighbouring strips / chunks: reads
// (TY + 2) / TY x (zc + 2) / zc, writes 1.  Pushed (node, direction) pairs are written exactly once, so strips and
// chunks never store to the same word.
//
// The arithmetic is slf_node.h's, called as fast_row_kernel calls it; with -ffp-contract=off the result is bit-identical
// to two single steps.  Not served: macro field output (options bit 0), body forces, node maps, x-face buffers.
//
// Phase A has two load paths (template argument PF, SLF_PAIR_PREFETCH).  PF 0 loads a row into registers and waits for it
// before it collides.  PF 1 keeps the NEXT row of the march in flight while the current one collides: the loads write LDS
// directly (no register destination, so the 19 values in flight cost no VGPRs), see the comment at stage_row below.
//
// Which strip a workgroup takes, and in which order phase A walks its rows, is chosen for the L2 (speed only: every strip
// is taken exactly once whatever the placement, and the rows of phase A are collided independently and filed by
// assignment, so neither changes a result).  A halo row of a strip is an own row of its neighbour; the two reads of it
// meet in an L2 only if both strips run on one XCD, close in time:
//   strips   workgroups are dealt to the eight XCDs round-robin by flat index.  The grid is (1, strips, chunks): with a
//            strip count divisible by 8 the flat index modulo 8 is blockIdx.y % 8 for every z chunk, which is what
//            xcd_row() (slf_sweep.h) relies on to hand every XCD 1 << shift CONSECUTIVE strips of a block of 8 << shift
//            (SLF_PAIR_XCD_LOG2 limits the shift; 0: strips as they come, neighbours always on different XCDs);
//   march    SLF_PAIR_MARCH=1: odd strips walk the rows downwards (y0 + TY .. y0 - 1), even strips upwards, so that both
//            neighbours touch the two rows they share at the same end of the march (upwards everywhere: four rows apart).
//
// Strip height.  TY 2 is the default, TY 4 is kept (SLF_PAIR_ROWS=4).  Two-row strips load and collide two rows of phase A
// per own row where four-row strips need 1.5, but with the placement above the second read of a shared row is an L2 hit,
// and 119 VGPRs give four waves per SIMD and two workgroups per CU where 197 give two and one.  Two two-row strips joined
// in one workgroup of sixteen waves, handing each other the post-collision values of their seam rows through LDS instead
// of colliding them twice (TY 4's row count at TY 2's registers), were built, were bit-identical and ran 18 % slower than
// separate two-row strips: one barrier couples all sixteen waves of a CU three times per plane.  Not kept
// (profiles/NOTES.md).
#include "slf_dispatch.h"
#include "slf_rowpush.h"

namespace slf {

namespace {

constexpr int PAIR_NT = 3;       // non-temporal loads and stores, as in slf_fast.hip
// The cache hint of phase A's loads alone (the stores stay PAIR_NT): 1 = non-temporal, 0 = plain.  Plain: a row that two
// strips share has to stay in the L2 between their reads, and with the hint it does not (profiles/NOTES.md: with
// neighbouring strips on one XCD the hint costs 10 % of the rate).
#ifndef SLF_PAIR_LOAD_NT
#define SLF_PAIR_LOAD_NT 0
#endif
constexpr int PAIR_LOAD_NT = SLF_PAIR_LOAD_NT ? PAIR_NT : 0;
#if SLF_PAIR_LOAD_NT
#define SLF_PAIR_LOAD_HINT " nt"
#else
#define SLF_PAIR_LOAD_HINT ""
#endif
constexpr int PAIR_NW = 8;       // waves of a row: nx <= 512

__device__ __forceinline__ int wrap1(int c, int n) {      // c in 0 .. n + 1 -> 1 .. n
  if (c < 1) c += n;
  if (c > n) c -= n;
  return c;
}

// PF > 0: the stage of phase A's asynchronous loads (dynamic LDS: 19 x 64 words per wave of the row)
extern __shared__ float s_stage[];
#define SLF_LDS __attribute__((address_space(3)))

// The workgroup barrier of phase B.  RAW: `s_waitcnt lgkmcnt(0)` + `s_barrier` and nothing else -- __syncthreads() carries
// a fence that, with an LDS-DMA outstanding, waits vmcnt(0) and so would drain the prefetch of the next plane's first row.
// The LDS words the barrier orders (s_in_*, s_out_*) are written and read by ds_ instructions only: lgkmcnt(0) retires the
// writes of this wave, the memory clobbers keep the compiler from moving LDS accesses across.
template <bool RAW>
__device__ __forceinline__ void pair_barrier() {
  if constexpr (RAW) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  } else {
    __syncthreads();
  }
}

template <int MODEL, int TY, int PF>
__global__ void __launch_bounds__(512, TY == 2 ? 4 : 2) pair_row_kernel(const SweepParams<D3Q19, float> p, const int zc,
                                                                         const int xcd_shift, const int march) {
  using L = D3Q19;
  static_assert(MODEL == 0, "BGK only");
  static_assert(TY % 2 == 0, "the push slots alternate by row");
  static_assert(PF == 0 || PF == 1, "ring depth");
  constexpr int NXD = count_x_dirs<L>();
  // raw intermediate values at the wave edges, per register plane: written as phase A produces them
  __shared__ float s_in_p[3][TY][PAIR_NW][NXD], s_in_m[3][TY][PAIR_NW][NXD];
  __shared__ float s_out_p[2][PAIR_NW][NXD], s_out_m[2][PAIR_NW][NXD];      // pushed values at the wave edges, by row parity
  const Geometry& g = p.g;
  const int ny = g.lat_ny - 2, nz = g.lat_nz - 2;
  const int lane = (int)threadIdx.x & 63;
  const int w = sgpr((int)threadIdx.x >> 6);
  const int nwave = sgpr((int)blockDim.x >> 6);
  // the row is a ring of waves (nwave = 1: a wave is its own neighbour)
  const int slot_p = sgpr(w == 0 ? nwave - 1 : w - 1);
  const int slot_m = sgpr(w == nwave - 1 ? 0 : w + 1);
  const int x = (int)threadIdx.x + 1;
  const uint32_t xb = (uint32_t)x * 4u;
  const int strip = sgpr(xcd_row((int)blockIdx.y, xcd_shift));
  const int y0 = sgpr(1 + strip * TY);
  const bool down = sgpr((int)(march != 0 && (strip & 1) != 0)) != 0;      // this strip walks phase A's rows downwards
  const int z0 = sgpr(1 + (int)blockIdx.z * zc);
  int zn = nz - (z0 - 1);                 // planes of this chunk: the last one may be shorter
  if (zn > zc) zn = zc;
  zn = sgpr(zn);
  const size_t ds = g.dist_size;
  const AxisOff ox0 = {0, 0};
  const bool inc = p.cp.incompressible != 0;

  // intermediate state before the x shift: P0 plane k - 1, P1 plane k (e_z >= 0), P2 plane k + 1 (e_z > 0)
  float P0[TY][L::Q], P1[TY][L::Q], P2[TY][L::Q];
  static_for<0, TY>([&](auto J) {
    static_for<0, L::Q>([&](auto I) { P0[J][I] = P1[J][I] = P2[J][I] = 0.0f; });
  });

  // PF: the 19 values of a row go straight to LDS (global_load_lds_dword: no VGPR destination), each wave the 64 x of its
  // own segment into words of its own.  The image is lane-linear (wave-uniform base in M0 + lane x 4) and the wave reads
  // it back at its own lane, so no other wave touches the words and staging needs no barrier.  What orders the accesses
  // is written by hand, the compiler emits none of it:
  //   s_waitcnt vmcnt(0)    before the first read of a staged row: the DMAs have landed (a missing wait reads stale words);
  //   s_waitcnt lgkmcnt(0)  after the 19 reads, before the refill: the reads have returned, the words may be overwritten.
  // The refill is the NEXT row of the march (after the last row of a plane: the first row of the next plane), so its
  // latency runs under this wave's collision of the current row resp. under the whole of phase B.
  // One statement issues the 19 DMAs of a row: source = wave-uniform base of the direction (an SGPR pair, here VCC, stepped
  // by the distance between two directions) + the lane's x in a VGPR shared by all 19, with the cache hint of the loads of
  // the synchronous form (SLF_PAIR_LOAD_NT); destination = M0 (the compiler's register: saved and put back) + lane x 4, stepped by 256 B.
  float* const stage_w = s_stage + sgpr(w * (L::Q * 64));
  const uint32_t stage_m0 = sgpr((uint32_t)(uintptr_t)(SLF_LDS float*)stage_w);
  const uint64_t dir_bytes = (uint64_t)ds * sizeof(float);
  const uint32_t dlo = sgpr((uint32_t)dir_bytes), dhi = sgpr((uint32_t)(dir_bytes >> 32));
  auto stage_row = [&](int gy, int gz) {
    const uint32_t row = sgpr((uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz);
    const uint64_t src = (uint64_t)(p.din + row);
    const uint32_t slo = sgpr((uint32_t)src), shi = sgpr((uint32_t)(src >> 32));
    uint32_t keep;
    static_assert(L::Q == 19, "the statement below: 1 + 18 loads");
    asm volatile(
        "s_mov_b32 %[keep], m0\n\t"
        "s_mov_b32 vcc_lo, %[slo]\n\t"
        "s_mov_b32 vcc_hi, %[shi]\n\t"
        "s_mov_b32 m0, %[lds]\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %[xb], vcc" SLF_PAIR_LOAD_HINT "\n\t"
        ".rept 18\n\t"
        "s_add_u32 m0, m0, 0x100\n\t"
        "s_add_u32 vcc_lo, vcc_lo, %[dlo]\n\t"
        "s_addc_u32 vcc_hi, vcc_hi, %[dhi]\n\t"
        "global_load_lds_dword %[xb], vcc" SLF_PAIR_LOAD_HINT "\n\t"
        ".endr\n\t"
        "s_mov_b32 m0, %[keep]"
        : [keep] "=&s"(keep)
        : [slo] "s"(slo), [shi] "s"(shi), [lds] "s"(stage_m0), [dlo] "s"(dlo), [dhi] "s"(dhi), [xb] "v"(xb)
        : "vcc", "scc", "memory");
  };
  if constexpr (PF > 0) stage_row(sgpr(wrap1(down ? y0 + TY : y0 - 1, ny)), sgpr(wrap1(z0 - 1, nz)));

  int c0 = 0, c1 = 1, c2 = 2;     // LDS slots of the planes k - 1, k, k + 1
  for (int s = 0; s < zn + 2; s++) {
    const int gz = sgpr(wrap1(z0 - 1 + s, nz));
    const bool own_plane = s >= 1 && s <= zn;
    // ---- phase A: step t of rows y0 - 1 .. y0 + TY of plane k = z0 - 1 + s, upwards or (DOWN) downwards.  The row index
    // stays a compile-time constant either way (a run-time index would send the register planes to scratch), so the
    // march exists twice, behind one wave-uniform branch.
    auto phase_a = [&](auto DOWN) {
      static_for<0, TY + 2>([&](auto M) {
        constexpr bool dn = decltype(DOWN)::value;
        constexpr int rr = dn ? TY - (int)M : (int)M - 1;        // this row of the march; the next one is rr + step
        constexpr int step = dn ? -1 : 1, first = dn ? TY : -1;
        const int gy = sgpr(wrap1(y0 + rr, ny));
        float f[L::Q];
        if constexpr (PF > 0) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          static_for<0, L::Q>([&](auto I) { f[I] = stage_w[(int)I * 64 + lane]; });
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if constexpr ((int)M < TY + 1) stage_row(sgpr(wrap1(y0 + rr + step, ny)), gz);
          else if (s + 1 < zn + 2) stage_row(sgpr(wrap1(y0 + first, ny)), sgpr(wrap1(z0 + s, nz)));
        } else {
          const uint32_t row = sgpr((uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gz);
          static_for<0, L::Q>([&](auto I) {
            f[I] = ldg<PAIR_LOAD_NT>(at_byte(uniform_base(p.din + ds * (size_t)I + row), xb));
          });
        }
        float rho, v[3];
        macro_standard<L, float>(f, inc, rho, v);
        if constexpr (rr >= 0 && rr < TY) {
          if (own_plane) check_invalid<float>(p.status, p.options, rho, x, gy, gz);
        }
        if (p.relaxation_enabled) bgk_relax<L, float, false>(f, rho, v, p.cp);
        static_for<0, L::Q>([&](auto I) {
          constexpr int j = rr + L::ey(I);
          if constexpr (j >= 0 && j < TY) {
            if constexpr (L::ez(I) > 0) P2[j][I] = f[I];
            else if constexpr (L::ez(I) == 0) P1[j][I] = f[I];
            else P0[j][I] = f[I];
          }
        });
        // ... and the words that will cross a wave edge in phase B
        if (lane == 63) {
          static_for<1, L::Q>([&](auto I) {
            constexpr int j = rr + L::ey(I);
            if constexpr (L::ex(I) > 0 && j >= 0 && j < TY)
              s_in_p[L::ez(I) > 0 ? c2 : (L::ez(I) == 0 ? c1 : c0)][j][w][x_dir_rank<L, I>()] = f[I];
          });
        }
        if (lane == 0) {
          static_for<1, L::Q>([&](auto I) {
            constexpr int j = rr + L::ey(I);
            if constexpr (L::ex(I) < 0 && j >= 0 && j < TY)
              s_in_m[L::ez(I) > 0 ? c2 : (L::ez(I) == 0 ? c1 : c0)][j][w][x_dir_rank<L, I>()] = f[I];
          });
        }
      });
    };
    if (down) phase_a(std::true_type{});
    else phase_a(std::false_type{});
    // ---- phase B: plane k - 1 of the intermediate state is complete; step t + 1 of the own rows
    if (s >= 2) {
      const int gzb = sgpr(z0 + s - 2);
      AxisOff oz = axis_off(gzb, g.lat_nz, g.arr_nxy, 1);
      oz.p = sgpr(oz.p); oz.m = sgpr(oz.m);
      pair_barrier<(PF > 0)>();
      static_for<0, TY>([&](auto J) {
        constexpr int buf = (int)J & 1;
        float f[L::Q];
        {
          int kp = 0, km = 0;
          static_for<0, L::Q>([&](auto I) {
            if constexpr (L::ex(I) > 0) f[I] = lane_shift1<float, true>(s_in_p[c0][J][slot_p][kp++], P0[J][I]);
            else if constexpr (L::ex(I) < 0) f[I] = lane_shift1<float, false>(s_in_m[c0][J][slot_m][km++], P0[J][I]);
            else f[I] = P0[J][I];
          });
        }
        const int gy = sgpr(y0 + (int)J);
        float rho, v[3];
        macro_standard<L, float>(f, inc, rho, v);
        check_invalid<float>(p.status, p.options, rho, x, gy, gzb);
        if (p.relaxation_enabled) bgk_relax<L, float, false>(f, rho, v, p.cp);
        // push: the value of node x travels to x + e_x and is stored by the thread that owns the target x
        if (lane == 63) {
          int k = 0;
          static_for<1, L::Q>([&](auto I) { if constexpr (L::ex(I) > 0) s_out_p[buf][w][k++] = f[I]; });
        }
        if (lane == 0) {
          int k = 0;
          static_for<1, L::Q>([&](auto I) { if constexpr (L::ex(I) < 0) s_out_m[buf][w][k++] = f[I]; });
        }
        pair_barrier<(PF > 0)>();
        const uint32_t row = sgpr((uint32_t)g.arr_nx * (uint32_t)gy + (uint32_t)g.arr_nxy * (uint32_t)gzb);
        AxisOff oy = axis_off(gy, g.lat_ny, g.arr_nx, 1);
        oy.p = sgpr(oy.p); oy.m = sgpr(oy.m);
        int kp = 0, km = 0;
        static_for<0, L::Q>([&](auto I) {
          const int off = dir_offset<L, I>(ox0, oy, oz, true);
          const auto base = uniform_base(p.dout + ds * (size_t)I + (uint32_t)((int)row + off));
          float t = f[I];
          if constexpr (L::ex(I) > 0) t = lane_shift1<float, true>(s_out_p[buf][slot_p][kp++], f[I]);
          if constexpr (L::ex(I) < 0) t = lane_shift1<float, false>(s_out_m[buf][slot_m][km++], f[I]);
          stg<PAIR_NT>(at_byte(base, xb), t);
        });
      });
    }
    // ---- rotate the register planes and their LDS slots
    { const int t = c0; c0 = c1; c1 = c2; c2 = t; }
    static_for<0, TY>([&](auto J) {
      static_for<0, L::Q>([&](auto I) {
        if constexpr (L::ez(I) >= 0) P0[J][I] = P1[J][I];
        if constexpr (L::ez(I) > 0) P1[J][I] = P2[J][I];
      });
    });
  }
}

}  // namespace

// Two-row strips, whatever the box (they only need an even ny).  By the bytes four-row strips read less (1.5 x 66/64 arrays
// against 2 x 66/64), but with neighbouring strips on one XCD most of a strip's halo rows come from the L2, two-row strips
// gain twice as much from that, and their four waves per SIMD (119 VGPRs against 197) hide more of what is left:
// measured at 512^3 and 256^3, profiles/NOTES.md.  SLF_PAIR_ROWS=4 still selects four-row strips.
int pair_default_rows(const Geometry&) { return 2; }
int pair_default_zchunk(const Geometry&) { return 64; }
int pair_default_prefetch() { return 1; }
int pair_default_xcd_log2() { return 5; }
int pair_default_march() { return 1; }

// the shift of xcd_row() for this many strips: the largest s <= limit whose block of 8 << s strips divides the count
int pair_xcd_shift(int strips, int limit) {
  int s = limit < 0 ? 0 : (limit > 8 ? 8 : limit);
  while (s > 0 && (strips % (8 << s)) != 0) s--;
  return s;
}

const char* pair_refusal(const KernelSelector& sel, bool two_copy, const Geometry& g, const Physics& ph, const SweepArgs& a,
                         const PairKnobs& k) {
  const auto [rows, zc, prefetch, xcd_log2, march] = k;
  if (sel.lattice != 1 || sel.precision != 4 || sel.model != 0) return "pair sweep: D3Q19, single precision, BGK modules only";
  if (!two_copy) return "pair sweep: the two-copy (AB) access pattern only";
  if (sel.general || a.map) return "pair sweep: modules without a node map only";
  if (g.indirect || a.nodes) return "pair sweep: direct addressing only";
  if (ph.has_force) return "pair sweep: body forces are not served";
  if (!(g.variant & 1) || (g.variant & 256)) return "pair sweep: the tuned kernels are switched off for this module";
  if (!g.wrap[0] || !g.wrap[1] || !g.wrap[2]) return "pair sweep: every axis must be wrapped inside the sweep";
  if (a.xsend[0] || a.xsend[1] || a.xrecv[0] || a.xrecv[1]) return "pair sweep: not with x-face buffers";
  const int nx = g.lat_nx - 2, ny = g.lat_ny - 2;
  if (nx % 64 != 0 || nx < 64 || nx > 64 * PAIR_NW) return "pair sweep: rows of 64 .. 512 nodes, a multiple of 64";
  if (rows != 2 && rows != 4) return "pair sweep: 2 or 4 rows per strip";
  if (ny % rows != 0) return "pair sweep: ny must be a multiple of the rows per strip";
  if (zc < 1) return "pair sweep: planes per chunk must be positive";
  if (prefetch != 0 && prefetch != 1) return "pair sweep: SLF_PAIR_PREFETCH is 0 (synchronous loads) or 1 (one row staged in LDS)";
  if (xcd_log2 < 0 || xcd_log2 > 8)
    return "pair sweep: SLF_PAIR_XCD_LOG2 is an integer in 0 .. 8 (consecutive strips per XCD = 1 << this at most; 0: off)";
  if (march != 0 && march != 1) return "pair sweep: SLF_PAIR_MARCH is 0 (every strip walks its rows upwards) or 1 (odd strips downwards)";
  if (!a.dist_in || !a.dist_out) return "pair sweep: source or destination array is NULL";
  if (a.dist_in == a.dist_out) return "pair sweep: source and destination must be different arrays";
  if (a.options & 1u) return "pair sweep: macro field output is not served (options bit 0)";
  return nullptr;
}

bool launch_sweep_pair(const KernelSelector& sel, bool two_copy, const Geometry& g, const Physics& ph, const SweepArgs& a,
                       const PairKnobs& k, hipStream_t s, hipError_t* err) {
  if (pair_refusal(sel, two_copy, g, ph, a, k)) return false;
  const SweepParams<D3Q19, float> p = make_params<D3Q19, float>(g, ph, a, 1, 1);
  const int nx = g.lat_nx - 2, ny = g.lat_ny - 2, nz = g.lat_nz - 2;
  const int rows = k.rows, prefetch = k.prefetch, xcd_log2 = k.xcd_log2, march = k.march, zc = k.zc > nz ? nz : k.zc;
  dim3 block(nx, 1, 1);
  dim3 grid(1, ny / rows, (nz + zc - 1) / zc);
  // grid.x = 1: the flat index of a workgroup modulo 8 is blockIdx.y % 8 in every chunk where 8 divides the strip count,
  // and pair_xcd_shift() gives 0 (strips as they come) where it does not
  const int shift = pair_xcd_shift((int)grid.y, xcd_log2);
  // the stage of the asynchronous loads: 19 x 64 words per wave of the row (38 912 B at nx = 512: two workgroups of
  // two-row strips resp. one of four-row strips per CU, as the registers allow; narrower rows take less)
  const size_t lds = prefetch ? (size_t)(nx / 64) * D3Q19::Q * 64 * sizeof(float) : 0;
  const bool done = pick<int, 2, 4>(rows, [&](auto TY) {
    pick<int, 0, 1>(prefetch, [&](auto PF) {
      hipLaunchKernelGGL((pair_row_kernel<0, TY, PF>), grid, block, lds, s, p, zc, shift, march);
    });
  });
  if (done) *err = hipGetLastError();
  return done;
}

}  // namespace slf
