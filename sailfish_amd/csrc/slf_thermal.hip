// The temperature lattice of a thermal flow (C ABI slf_thermal_*; host surface lb_thermal.LBThermalFluidSim,
// sailfish_amd/thermal.py, subdomain_runner.ThermalSubdomainRunner).  The reference has no thermal model:
// this file follows the semantics of DESIGN.md §9j.
//
// D2Q5 beside D2Q9 and D3Q7 beside D3Q19.  Directions: 0 rest, 1 +x, 2 -x, 3 +y, 4 -y, 5 +z, 6 -z; opp(i) = i + 1 for odd i,
// i - 1 for even i > 0.  Weights w0 = 1/3, w = 1/6, k = 3 (D2Q5); w0 = 1/4, w = 1/8, k = 4 (D3Q7).  Two arrays g[copy][i][node]
// with the layout and padding of rho (direction arrays arr_nx * arr_ny * arr_nz elements apart); a node's slot holds its own
// post-collision values, so streaming is a pull.  The flow module is an ordinary accel_field module: the step reads the
// velocity its sweep has just stored and rewrites the field the next sweep reads.
//
// ONE OPERATION ORDER (compiled with -ffp-contract=off; tests/_thermal_twin.py restates it in numpy), at every wet node x:
//   pull     n = x - e_i, wrapped on the axes flagged periodic;
//            n a real node and wet:      g_i = src[i][n]
//            n a real node and not wet:  Tw = wall_temperature[n];  g_i = isfinite(Tw) ? (2 w_i) * Tw - src[opp i][x]
//                                                                                      : src[opp i][x]
//            n outside the real nodes:   g_i = src[opp i][x]                          (wall_temperature is not read)
//   T        = (((((g0 + g1) + g2) + g3) + g4) + g5) + g6                             (5 terms in 2-D)
//   fixed    MAP only: Tw = wall_temperature[x]; if isfinite(Tw): T = Tw, g_i = geq_i for every i
//   collide  eu_i = +-u[d] (0 for i = 0);  geq_i = (w_i * T) * (1 + k * eu_i);  dst[i][x] = g_i + omega_T * (geq_i - g_i)
//   store    T_field[x] = T;  field[d][x] = b[d] * (T - T_ref)
// Nodes that are not wet are never written.  One lane per node along x, one wave per 64-node row segment; lanes past the
// last real column and rows past the last real row leave.  Every index is formed from coordinates checked against the
// real nodes 1 .. lat - 2 of the module's (checked) extents, so no launch reads or writes outside the arrays.
#include "slf_dispatch.h"
#include "slf_kernels.h"
#include "slf_lattice.h"
#include "slf_node.h"

namespace slf {

namespace {

constexpr int THERMAL_BX = 64, THERMAL_BY = 4;        // a wave along x, four rows to a workgroup

struct ThermalGeo {
  int lat[3], arr_nx, arr_nxy;
  int periodic[3];
  size_t stride;               // arr_nx * arr_ny * arr_nz: between the direction arrays of g and the components of the field
  unsigned long long type_lut;
  uint32_t type_mask;
};

template <class R>
struct ThermalParams {
  R omega, t_ref, b[3];
};

template <int DIM, class R>
struct ThermalLattice {
  static constexpr int Q = 2 * DIM + 1;
  static constexpr R k = DIM == 2 ? (R)3 : (R)4;
  static constexpr R w(int i) { return DIM == 2 ? (i == 0 ? (R)(1.0 / 3.0) : (R)(1.0 / 6.0)) : (i == 0 ? (R)0.25 : (R)0.125); }
  static constexpr R w2(int i) { return (R)2 * w(i); }
  static constexpr int axis(int i) { return (i - 1) / 2; }
  static constexpr int sign(int i) { return (i & 1) ? 1 : -1; }
  static constexpr int opp(int i) { return i == 0 ? 0 : ((i & 1) ? i + 1 : i - 1); }
};

SLF_D bool thermal_finite(float x) { return __builtin_isfinite(x); }
SLF_D bool thermal_finite(double x) { return __builtin_isfinite(x); }

// geq_i = (w_i * T) * (1 + k * eu_i)
template <int DIM, class R, int I>
SLF_D R thermal_geq(R T, const R (&u)[3]) {
  using TL = ThermalLattice<DIM, R>;
  R eu = (R)0;
  if constexpr (I > 0) eu = TL::sign(I) > 0 ? u[TL::axis(I)] : (R)0 - u[TL::axis(I)];
  return (TL::w(I) * T) * ((R)1 + TL::k * eu);
}

// The coordinates (array indices) of the lane's node; false: not a real node of the subdomain.
template <int DIM>
SLF_D bool thermal_node(const ThermalGeo& g, int (&c)[3], size_t& gi) {
  c[0] = (int)(blockIdx.x * THERMAL_BX + threadIdx.x) + 1;
  c[1] = (int)(blockIdx.y * THERMAL_BY + threadIdx.y) + 1;
  c[2] = DIM == 3 ? (int)blockIdx.z + 1 : 0;
  if (c[0] > g.lat[0] - 2 || c[1] > g.lat[1] - 2) return false;
  if (DIM == 3 && c[2] > g.lat[2] - 2) return false;
  gi = (size_t)c[0] + (size_t)g.arr_nx * (size_t)c[1] + (size_t)g.arr_nxy * (size_t)c[2];
  return true;
}

template <int DIM, class R, bool MAP>
__global__ void __launch_bounds__(THERMAL_BX * THERMAL_BY)
thermal_step_kernel(const ThermalGeo g, const ThermalParams<R> p, const uint32_t* __restrict__ map, const R* __restrict__ src,
                    R* __restrict__ dst, const R* __restrict__ vx, const R* __restrict__ vy, const R* __restrict__ vz,
                    const R* __restrict__ wall_t, R* __restrict__ t_field, R* __restrict__ field) {
  using TL = ThermalLattice<DIM, R>;
  int c[3];
  size_t gi;
  if (!thermal_node<DIM>(g, c, gi)) return;
  if constexpr (MAP) {
    if (!kind_is_wet(node_kind(g.type_lut, g.type_mask, map[gi]))) return;
  }
  const size_t axis_stride[3] = {1, (size_t)g.arr_nx, (size_t)g.arr_nxy};
  R gp[TL::Q];
  gp[0] = src[gi];
  static_for<1, TL::Q>([&](auto I) {
    constexpr int d = TL::axis(I), o = TL::opp(I);
    int cn = c[d] - TL::sign(I);                       // n = x - e_i along axis d
    bool real = true;
    if (cn < 1) {
      cn = g.lat[d] - 2;
      real = g.periodic[d] != 0;
    } else if (cn > g.lat[d] - 2) {
      cn = 1;
      real = g.periodic[d] != 0;
    }
    // (cn is a real coordinate either way, so the index below is inside the arrays; it is used only where `real`)
    const size_t ni = gi - (size_t)c[d] * axis_stride[d] + (size_t)cn * axis_stride[d];
    R val;
    if (!real) {
      val = src[(size_t)o * g.stride + gi];
    } else {
      bool nwet = true;
      if constexpr (MAP) nwet = kind_is_wet(node_kind(g.type_lut, g.type_mask, map[ni]));
      if (nwet) {
        val = src[(size_t)I * g.stride + ni];
      } else {
        const R tw = wall_t[ni];
        const R own = src[(size_t)o * g.stride + gi];
        val = thermal_finite(tw) ? TL::w2(I) * tw - own : own;
      }
    }
    gp[I] = val;
  });
  R T = gp[0];
  static_for<1, TL::Q>([&](auto I) { T = T + gp[I]; });
  R u[3] = {vx[gi], vy[gi], (R)0};
  if constexpr (DIM == 3) u[2] = vz[gi];
  if constexpr (MAP) {
    const R tw = wall_t[gi];
    if (thermal_finite(tw)) {
      T = tw;
      static_for<0, TL::Q>([&](auto I) { gp[I] = thermal_geq<DIM, R, I>(T, u); });
    }
  }
  static_for<0, TL::Q>([&](auto I) {
    const R ge = thermal_geq<DIM, R, I>(T, u);
    dst[(size_t)I * g.stride + gi] = gp[I] + p.omega * (ge - gp[I]);
  });
  t_field[gi] = T;
  const R dt = T - p.t_ref;
  static_for<0, DIM>([&](auto D) { field[(size_t)D * g.stride + gi] = p.b[D] * dt; });
}

// (the map pointer is tested at run time: a launch per run does not pay for a second set of instantiations)
template <int DIM, class R>
__global__ void __launch_bounds__(THERMAL_BX * THERMAL_BY)
thermal_init_kernel(const ThermalGeo g, const ThermalParams<R> p, const uint32_t* __restrict__ map, const R* __restrict__ t_field,
                    const R* __restrict__ vx, const R* __restrict__ vy, const R* __restrict__ vz, R* __restrict__ dst,
                    R* __restrict__ field) {
  using TL = ThermalLattice<DIM, R>;
  int c[3];
  size_t gi;
  if (!thermal_node<DIM>(g, c, gi)) return;
  if (map && !kind_is_wet(node_kind(g.type_lut, g.type_mask, map[gi]))) return;
  const R T = t_field[gi];
  R u[3] = {vx[gi], vy[gi], (R)0};
  if constexpr (DIM == 3) u[2] = vz[gi];
  static_for<0, TL::Q>([&](auto I) { dst[(size_t)I * g.stride + gi] = thermal_geq<DIM, R, I>(T, u); });
  const R dt = T - p.t_ref;
  static_for<0, DIM>([&](auto D) { field[(size_t)D * g.stride + gi] = p.b[D] * dt; });
}

ThermalGeo thermal_geo(const Geometry& g, const int periodic[3]) {
  ThermalGeo o{};
  o.lat[0] = g.lat_nx, o.lat[1] = g.lat_ny, o.lat[2] = g.lat_nz;
  o.arr_nx = g.arr_nx, o.arr_nxy = g.arr_nxy;
  for (int d = 0; d < 3; d++) o.periodic[d] = d < g.dim && periodic[d] != 0;
  o.stride = (size_t)g.arr_nxy * (size_t)g.arr_nz;
  o.type_lut = g.type_lut, o.type_mask = g.type_mask;
  return o;
}

template <class R>
ThermalParams<R> thermal_params(const ThermalConstants& k) {
  ThermalParams<R> p;
  p.omega = (R)k.omega, p.t_ref = (R)k.t_ref;
  for (int d = 0; d < 3; d++) p.b[d] = (R)k.b[d];
  return p;
}

dim3 thermal_grid(const Geometry& g) {
  return dim3((g.lat_nx - 2 + THERMAL_BX - 1) / THERMAL_BX, (g.lat_ny - 2 + THERMAL_BY - 1) / THERMAL_BY,
              g.dim == 3 ? g.lat_nz - 2 : 1);
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

hipError_t launch_thermal_init(const KernelSelector& sel, const Geometry& g, const ThermalConstants& k, const void* map,
                               const void* t_field, const void* const v[3], void* g0, void* field, hipStream_t s) {
  const ThermalGeo tg = thermal_geo(g, k.periodic);
  const dim3 grid = thermal_grid(g), block(THERMAL_BX, THERMAL_BY);
  return pick_dim_real(sel, [&](auto DIM, auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((thermal_init_kernel<decltype(DIM)::value, R>), grid, block, 0, s, tg, thermal_params<R>(k),
                       (const uint32_t*)map, (const R*)t_field, (const R*)v[0], (const R*)v[1], (const R*)v[2], (R*)g0, (R*)field);
  });
}

hipError_t launch_thermal_step(const KernelSelector& sel, const Geometry& g, const ThermalConstants& k, const void* map,
                               const void* src, void* dst, const void* const v[3], const void* wall_t, void* t_field,
                               void* field, hipStream_t s) {
  const ThermalGeo tg = thermal_geo(g, k.periodic);
  const dim3 grid = thermal_grid(g), block(THERMAL_BX, THERMAL_BY);
  return pick_dim_real(sel, [&](auto DIM, auto r) {
    using R = decltype(r);
    pick_bool(map != nullptr, [&](auto MAP) {
      hipLaunchKernelGGL((thermal_step_kernel<decltype(DIM)::value, R, decltype(MAP)::value>), grid, block, 0, s, tg,
                         thermal_params<R>(k), (const uint32_t*)map, (const R*)src, (R*)dst, (const R*)v[0], (const R*)v[1],
                         (const R*)v[2], (const R*)wall_t, (R*)t_field, (R*)field);
    });
  });
}

}  // namespace slf
