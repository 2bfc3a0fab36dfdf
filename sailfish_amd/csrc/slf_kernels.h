// Host-visible launch interface of the gfx950 kernels (C++ linkage, used only by
// slf_api.hip).  See slf_kernels.hip for the kernels themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slf {

enum Prop : int { PROP_AB = 0, PROP_AA_EVEN = 1, PROP_AA_ODD = 2 };

// Geometry + decode information shared by all kernels of a module.
struct Geometry {
  int dim;
  int lat_nx, lat_ny, lat_nz;  // incl. ghosts (lat_nz == 1 in 2-D)
  int arr_nx, arr_ny, arr_nz;
  int arr_nxy;                 // arr_nx * arr_ny
  uint32_t dist_size;          // stride between direction arrays (>= arr_nx * arr_ny * arr_nz)
  int wrap[3];                 // in-kernel periodic wrap per axis
  int axis_mode[3];            // 0: not locally periodic, 1: ghost-layer PBC kernels, 2: wrapped in-sweep
  // node code decoding
  uint32_t type_mask;
  uint32_t param_shift;        // = bits of the type field
  uint32_t param_mask;
  uint32_t orient_shift;
  unsigned long long type_lut; // 4 bits per dense type id -> NodeKind
  int use_link_tags;
  int variant;                 // tuned-kernel selection bits (SLF_VARIANT), see slf_fast.hip
  int indirect;                // distributions hold active nodes only, addressed through SweepArgs::nodes
  // What the module's node-type table contains (decided once, at module creation): 0 = nothing beyond fluid, ghost,
  // unused, propagation-only and full-way bounce-back nodes; 1 = boundary-condition nodes; 2 = also the outflow
  // nodes that read neighbouring nodes (two-copy pattern), the do-nothing nodes of the in-place pattern and the full-slip
  // nodes.  The f32 whole-row kernels are instantiated per level: the
  // code of conditions a simulation does not use costs registers (52 instead of 78-80 VGPRs at level 0) and, for
  // the outflow nodes, spills in the hot path of the two-copy kernel.
  int bc_level;
  // bit 0 / 1: nothing ever reads the ghost column x = 0 / x = nx + 1 (the face is neither periodic through the
  // ghost-layer kernels nor connected to another subdomain): the whole-row kernels do not store into it -- five
  // partial-line writes per row and face that HBM turns into read-modify-writes (slf_module_set_x_ghost_unused)
  int x_ghost_unused;
};

// Decoding a node code: the NodeKind (slf_node.h) of a dense type id and of a node code.  The LUT and the mask are passed
// as values (call sites: g.type_lut, g.type_mask).
__host__ __device__ __forceinline__ int type_kind(unsigned long long type_lut, uint32_t dense_type) {
  return (int)((type_lut >> (4u * dense_type)) & 0xFull);
}
__host__ __device__ __forceinline__ int node_kind(unsigned long long type_lut, uint32_t type_mask, uint32_t code) {
  return type_kind(type_lut, code & type_mask);
}

struct Physics {
  double tau, visc;
  double accel[3];
  double mrt_rates[27];
  int incompressible;
  int has_force;
  int relaxation_enabled;
  int force_edm;   // body / Shan-Chen forces by the exact difference method instead of Guo's
  // --regularized / --subgrid=les-smagorinsky (slf_module_desc; relaxation_common.mako:166-237): per-node kernels only
  int regularized, subgrid;
  double smagorinsky_const;
  // --model=elbm (slf_module_desc; templates/entropic.mako): per-node kernels only
  int entropic_equilibrium;
  double entropy_tolerance, alpha_tolerance;
  // NTWallTMS (Tamm-Mott-Smith wall): bit t set = dense type id t is a TMS wall; 0: the module has none.  Inside the kernels
  // such a type is a half-way bounce-back type (its entry in Geometry::type_lut) with this flag (SweepParams::tms_mask),
  // read only by the boundary-condition code of the instantiations launched for modules that have one
  // (node_update with V.tms, slf_sweep.h).  Kept out of Geometry, which every kernel of the library takes by value.
  uint32_t tms_mask;
  // slf_module_desc::accel_field: the module reads an acceleration per node (SweepArgs::accf); the ACCF instantiations of
  // the per-node kernels run, has_force is set
  int accel_field;
  // slf_module_desc::equilibrium / gravity: SLF_EQ_SHALLOW_WATER -- the SW instantiations of the per-node kernels and of
  // init_kernel run (D2Q9, BGK); gravity is read by those only
  int equilibrium;
  double gravity;
};

struct ShanChen {
  int enabled;      // 0 off, 1 binary mixture, 2 single component
  double tau_phi;
  double G[4];      // G11 G12 G21 G22
  int potential;    // 0 linear, 1 classic
  double accel1[3]; // body-force acceleration on lattice 1 (Physics::accel acts on lattice 0)
};

// Free-energy binary fluid (slf_fe.hip; reference lb_binary.py:139-372)
struct FreeEnergy {
  int enabled;
  double Gamma, kappa, A;      // mobility, interface and bulk free-energy parameters
  double tau_a, tau_b;         // relaxation times of the two components (tau0 interpolates with phi)
  double tau_phi;              // relaxation time of the order-parameter lattice
  double wall_phase;           // --bc_wall_grad_phase
  int wall_order;              // --bc_wall_grad_order: 1 | 2
  int rim[3];                  // per axis: 1 / 2 = zero gradient and Laplacian on the low / high rim layer
};

// Ternary Shan-Chen mixture (slf_sc3.hip; reference lb_ternary.py); lattice 0 relaxes with Physics::tau
struct ShanChen3 {
  int enabled;
  double tau_phi, tau_theta;   // relaxation times of lattices 1 and 2
  double G[9];                 // row-major: G[3 k + j] couples lattice k to the density field of lattice j
  int potential;               // 0 linear, 1 classic
  double accel1[3], accel2[3]; // body-force accelerations on lattices 1 and 2 (Physics::accel acts on lattice 0)
};

// launch arguments of the ternary kernels
struct Sc3Args {
  const void* map;             // NULL: fluid-only module
  void* dist_in[3];            // pass in front, fused sweep: lattices 0, 1, 2 | sweep of one lattice: [0]
  void* dist_out[3];
  void* field[3];              // rho, phi, theta
  void* v[3];
  uint32_t options;
};

struct RowClasses;
struct SlotTable;

struct SweepArgs {
  const void* nodes;   // indirect addressing: dense index -> slot table (uint32), else NULL
  const void* map;
  void* dist_in;
  void* dist_out;
  void* dist_in2;   // second lattice (fused binary Shan-Chen sweep), else unused
  void* dist_out2;
  void* rho;
  void* phi;        // second density field (binary Shan-Chen), else unused
  void* v[3];
  const void* node_params;
  void* status;        // device uint32[4]: invalid-value flag + position
  uint32_t options;
  // binary Shan-Chen: the fused sweep forms densities and velocity of its own node itself (kernels
  // ShanChenPrepareDensities / ShanChenCollideAndPropagateFusedV); the pass in front stores rho, phi and -- only when
  // options bit 0 asks for output -- the velocity
  bool sc_local_velocity;
  // x-face buffers (slf_module_set_xface_buffers): [0] low face (x = 1 side), [1] high face; NULL = not used
  void* xsend[2];
  const void* xrecv[2];
  // indirect addressing: which node owns which slot (SlotTable), NULL = not built: one thread per DENSE node
  const SlotTable* slots;
  // row classes of the node map `map` (slf_module_classify_rows), NULL = not classified; see RowClasses
  const RowClasses* rows;
  // binary Shan-Chen over connected x faces (slf_module_set_xface_planes): xsend / xrecv above serve lattice 0, these
  // lattice 1 and the densities rho, phi ([z][field][y] planes); NULL = not used
  void* xsend2[2];
  const void* xrecv2[2];
  void* msend[2];
  const void* mrecv[2];
  void* alpha;         // entropic modules: the alpha field (dense, like rho) or NULL
  void* lap;           // free-energy modules: the Laplacian of phi (dense, like rho), else unused
  const void* accf;    // accel_field modules: the acceleration field [d][arr_nz][arr_ny][arr_nx] (slf_module_set_accel_field)
};

// What slf_module_classify_rows() found in a node map, per 64-node x-segment (= one wavefront of a whole-row
// workgroup) and per (y, z) row.  Segment class 0: every node of the segment is a plain fluid node -- the wave
// does not read the map at all (4 of the 156 bytes per update) and runs the straight-line fluid body; 1: other
// nodes that need no boundary-condition code (ghost, unused, propagation-only, full-way bounce-back); 2: nodes
// with boundary conditions.  Rows whose worst segment is class 2 are listed in bc_rows and swept by the kernel
// instantiated for the module's Geometry::bc_level; all other rows by the level-0 instantiation with its 8
// resident waves per SIMD -- a lid-driven cavity has boundary-condition nodes in 0.2 % of its rows.
// Indirect addressing, the other way round: slot -> node.  Built once per `nodes` table (slf_api.hip), so that the sweep
// can be launched over the SLOTS -- every lane of every wave an active node, and consecutive lanes consecutive slots of
// every array -- instead of over the dense box, where a packed bed leaves 70 % of the lanes idle.
struct SlotTable {
  const void* nodes;          // the dense node -> slot table this was built from
  const uint32_t* slot_gi;    // dense index of the node that owns slot s; INVALID_NODE: nobody does
  const uint32_t* slot_yz;    // its y | z << 16
  uint32_t n_slots;           // highest used slot + 1
};

struct RowClasses {
  const void* map;             // the device node map the tables were built from
  const uint32_t* seg_class;   // bytes [arr_nz * arr_ny][nseg], addressed as dwords (scalar loads)
  const uint8_t* row_class;    // [arr_nz * arr_ny]
  const uint32_t* bc_rows;     // y | z << 16 of the class-2 rows
  int nseg;                    // segments per row = ceil(nx / 64)
  int n_rows, n_bc_rows;       // real rows, class-2 rows
  long long n_fluid_segments, n_segments;
};

// One module = one (lattice, model, precision, access pattern) specialisation.
struct KernelSelector {
  int lattice, model, precision;
  bool general;  // reads the node map / handles BC nodes
};

// Where and how a region launcher runs: the module's selector, geometry and physics, the propagation step of this launch and
// the rows [y0, y1) x [z0, z1) it covers (slf_bind.h launch_check), the module's workgroup width and the stream.
struct Launch {
  const KernelSelector& sel; Prop prop; const Geometry& g; const Physics& ph;
  int y0, y1, z0, z1; int block_x; hipStream_t s;
};

hipError_t launch_sweep(const Launch& lc, const SweepArgs& a);

hipError_t launch_init(const KernelSelector& sel, const Geometry& g, const Physics& ph, void* dist,
                       const void* rho, const void* const v[3], const void* nodes, hipStream_t s);

hipError_t launch_pbc(const KernelSelector& sel, const Geometry& g, void* dist, int axis, bool with_swap,
                      hipStream_t s);

hipError_t launch_macro_pbc(const KernelSelector& sel, const Geometry& g, void* field, int axis, hipStream_t s);

hipError_t launch_sparse(const KernelSelector& sel, bool collect, const unsigned long long* idx, void* dist, void* buffer,
                         int n, hipStream_t s);

hipError_t launch_box(const KernelSelector& sel, const Geometry& g, bool collect, void* dist, void* buffer,
                      const int* dirs, int nd, unsigned long long base, long long col_stride, int ncols, long long row_stride,
                      int nrows, long long buf_k_stride, long long buf_row_stride, bool deliver_all, hipStream_t s);

hipError_t launch_macro(const Launch& lc, const SweepArgs& a);      // every real node, whatever the rows of lc

// Builds the tables of RowClasses for `map` (device buffers seg_class, row_class, bc_rows and the counters
// {class-2 rows, class-0 segments} are the caller's); the counts are read back by the caller.
hipError_t launch_build_slot_table(const Geometry& g, const void* nodes, uint32_t* slot_gi, uint32_t* slot_yz,
                                   uint32_t* max_slot, hipStream_t s);
hipError_t launch_classify_rows(const Geometry& g, const void* map, uint32_t* seg_class, uint8_t* row_class,
                                uint32_t* bc_rows, uint32_t* counters, int nseg, hipStream_t s);

// ---- binary Shan-Chen (slf_sc.hip) ----
// macro pass: a.dist_in = lattice 0, a.dist_out = lattice 1 (both read), writes rho, phi, v
hipError_t launch_sc_macro(const Launch& lc, const ShanChen& sc, const SweepArgs& a);
// collide-and-stream of lattice `grid_idx`: reads rho, phi, v
hipError_t launch_sc_sweep(const Launch& lc, const ShanChen& sc, const SweepArgs& a, int grid_idx);
// both lattices in one pass: a.dist_in / dist_out = lattice 0, a.dist_in2 / dist_out2 = lattice 1
hipError_t launch_sc_fused(const Launch& lc, const ShanChen& sc, const SweepArgs& a);
// single-component Shan-Chen: density pass (a.dist_in -> a.rho) and the sweep with the force
hipError_t launch_scs_macro(const Launch& lc, const ShanChen& sc, const SweepArgs& a);      // every real node
hipError_t launch_scs_sweep(const Launch& lc, const ShanChen& sc, const SweepArgs& a);
hipError_t launch_sc_init(const KernelSelector& sel, const Geometry& g, const Physics& ph, void* dist1, void* dist2,
                          const void* rho, const void* phi, const void* const v[3], const void* nodes, hipStream_t s);

// ---- free-energy binary fluid (slf_fe.hip) ----
// macro pass: a.dist_out = lattice 1 (read), writes a.phi (wetting walls: phi of the helper node minus the constant)
hipError_t launch_fe_macro(const Launch& lc, const FreeEnergy& fe, const SweepArgs& a);
// collide-and-stream of the fluid lattice (which = 0: reads phi, writes v and a.lap) or of the order parameter (1: reads them)
hipError_t launch_fe_sweep(const Launch& lc, const FreeEnergy& fe, const SweepArgs& a, int which);
hipError_t launch_fe_init(const KernelSelector& sel, const Geometry& g, const FreeEnergy& fe, void* dist1, void* dist2,
                          const void* rho, const void* phi, const void* const v[3], const void* map, hipStream_t s);

// ---- ternary Shan-Chen mixture (slf_sc3.hip) ----
// pass in front: a.dist_in[0..2] (read) -> a.field[0..2], a.v
hipError_t launch_sc3_macro(const Launch& lc, const ShanChen3& sc, const Sc3Args& a);
// collide-and-stream of lattice `lattice` (a.dist_in[0] -> a.dist_out[0]): reads the three fields and v
hipError_t launch_sc3_sweep(const Launch& lc, const ShanChen3& sc, const Sc3Args& a, int lattice);
// the three lattices in one pass: a.dist_in[k] -> a.dist_out[k]
hipError_t launch_sc3_fused(const Launch& lc, const ShanChen3& sc, const Sc3Args& a);
hipError_t launch_sc3_init(const KernelSelector& sel, const Geometry& g, void* const dist[3], const void* const field[3],
                           const void* const v[3], hipStream_t s);

// ---- D3Q15 and D3Q27 (slf_lat.hip): BGK single-fluid modules, direct addressing ----
// the counterparts of launch_sweep / launch_init / launch_pbc / launch_macro; any other lattice: hipErrorInvalidValue
hipError_t launch_lat_sweep(const Launch& lc, const SweepArgs& a);
hipError_t launch_lat_init(const KernelSelector& sel, const Geometry& g, const Physics& ph, void* dist, const void* rho,
                           const void* const v[3], hipStream_t s);
hipError_t launch_lat_pbc(const KernelSelector& sel, const Geometry& g, void* dist, int axis, bool with_swap, hipStream_t s);
hipError_t launch_lat_macro(const Launch& lc, const SweepArgs& a);

// ---- several steps inside one launch (slf_resident.hip): 2-D lattices ----
// src / dst: the raw distribution arrays ([0] = the array of the in-place pattern / copy A of the two-copy pattern, [1] =
// copy B) and where the tiles go after `steps` steps from iteration it0; tiles of tile_x x tile_y nodes, halo of `halo`
hipError_t launch_resident(const KernelSelector& sel, bool aa, const Geometry& g, const Physics& ph, const SweepArgs& a,
                           const void* const src[2], void* const dst[2], int it0, int steps, int tile_x, int tile_y, int halo,
                           hipStream_t s);
// How far what is wrong has spread from the window's ring after `steps` steps from iteration it0 (the head of
// slf_resident.hip): the halo the tile needs.
inline int resident_halo(bool aa, int it0, int steps) {
  if (!aa) return steps + 1;
  int odd = 0;
  for (int s = 0; s < steps; s++) odd += (it0 + s) & 1;
  return odd ? 2 * odd : 1;
}
// in place: the array and the staging block of the odd steps; two-copy: copy A and copy B
inline size_t resident_lds_bytes(int q, int precision, bool /*aa*/, int win_x, int win_y) {
  const size_t nw = (size_t)win_x * (size_t)win_y;
  return nw * (size_t)q * (size_t)precision * 2 + nw * 8;
}

// ---- two steps per launch of the two-copy sweep (slf_pair.hip): periodic D3Q19 / f32 / BGK boxes ----
// a.dist_in: the populations of step t, a.dist_out: where those of step t + 2 go.  PairKnobs: strips of `rows` rows (2 or 4;
// 0: no pair sweep is armed), chunks of `zc` planes; prefetch: 0 = phase A loads into registers and waits, 1 = the next row is
// in flight to LDS while the current one collides; xcd_log2: neighbouring strips go to one XCD, at most 1 << this each (0:
// strips as they come); march: 1 = odd strips walk phase A's rows downwards.  pair_refusal: why the module / the arguments do
// not qualify, NULL if they do; launch_sweep_pair returns false (nothing launched) in exactly those cases.
struct PairKnobs {
  int rows, zc, prefetch, xcd_log2, march;
};
const char* pair_refusal(const KernelSelector& sel, bool two_copy, const Geometry& g, const Physics& ph, const SweepArgs& a,
                         const PairKnobs& k);
bool launch_sweep_pair(const KernelSelector& sel, bool two_copy, const Geometry& g, const Physics& ph, const SweepArgs& a,
                       const PairKnobs& k, hipStream_t s, hipError_t* err);
int pair_default_rows(const Geometry& g);
int pair_default_zchunk(const Geometry& g);
int pair_default_prefetch();
int pair_default_xcd_log2();
int pair_default_march();
int pair_xcd_shift(int strips, int limit);

// ---- flow statistics (slf_stats.hip): 3-D lattices, fields in the module's dense layout ----
// Launch shape of a statistics pass: a function of the lattice size alone, so the order of every addition is too.
constexpr int STATS_PROFILE_COUNT = 22;   // f, f^2, f^3, f^4 of ux, uy, uz, rho; ux uy, ux uz, uy uz, ux rho, uy rho, uz rho
struct StatsShape {
  int block, grid_x;
  int chunks, per_chunk;       // profiles: workgroups that share one position (one x block), rows / planes each takes
  size_t workspace_doubles;    // partial sums the pass leaves for its finalize launch
};
StatsShape stats_ke_shape(const Geometry& g);
StatsShape stats_profiles_shape(const Geometry& g, int axis);
// Sum of v^2 and of |curl v|^2 over the real, non-excluded nodes -> out2[2] (device); map NULL: no node is excluded;
// v_sq / vort_sq: both NULL or both fields to store (0 on ghost and excluded nodes)
hipError_t launch_stats_ke_enstrophy(const KernelSelector& sel, const Geometry& g, const void* map, const void* const v[3],
                                     void* v_sq, void* vort_sq, double* workspace, double* out2, hipStream_t s);
// out[k * out_stride + offset + p] = sum over the two other axes of statistic k at position p along `axis`
hipError_t launch_stats_profiles(const KernelSelector& sel, const Geometry& g, int axis, const void* const v[3],
                                 const void* rho, double* workspace, double* out, size_t out_stride, size_t offset,
                                 hipStream_t s);

// ---- momentum-exchange force on bodies (slf_force.hip): lattice 0 of a module, any access pattern and addressing ----
constexpr int FORCE_CHUNK = 4096;   // links of one object a workgroup adds up; the chunks of an object are added in index order
struct ForceShape {
  int block, grid_x;           // grid_x: chunks of the longest object
  size_t workspace_doubles;    // partial sums of the chunks (0 when every object is one chunk: no second launch)
};
ForceShape force_shape(int n_objects, uint32_t max_links);
// out[3 o + k] = sum over the links l = seg[o] .. seg[o + 1] - 1 of (double)(dist[idx[l]] + dist[idx2[l]]) * e_opp(dir[l])[k]
hipError_t launch_force_objects(const KernelSelector& sel, const void* dist, const uint32_t* idx, const uint32_t* idx2,
                                const uint8_t* dir, const uint32_t* seg, int n_objects, uint32_t max_links,
                                double* workspace, double* out, hipStream_t s);

// ---- immersed boundary markers (slf_ibm.hip): D2Q9 / D3Q19 modules with an acceleration field, one lane per marker ----
// pos / ref: [d][n], stiff: [n], in the module's precision; acc: int64 [d][arr_nz][arr_ny][arr_nx]; origin: the global
// coordinates of the real node with array index 1 on every axis.  Operation order: the head of slf_ibm.hip.
size_t ibm_accumulator_bytes(const Geometry& g);
hipError_t launch_ibm_spread(const KernelSelector& sel, const Geometry& g, const int32_t origin[3], int n, const void* pos,
                             const void* ref, const void* stiff, void* acc, hipStream_t s);
hipError_t launch_ibm_gather(const KernelSelector& sel, const Geometry& g, const int32_t origin[3], int n, const void* pos,
                             const void* acc, void* field, hipStream_t s);
hipError_t launch_ibm_clear_and_advect(const KernelSelector& sel, const Geometry& g, const int32_t origin[3], int n, void* pos,
                                       void* acc, void* field, const void* map, const void* const v[3], uint32_t* outside,
                                       hipStream_t s);

// ---- thermal flows (slf_thermal.hip): the temperature lattice D2Q5 / D3Q7 beside a D2Q9 / D3Q19 module with an acceleration
// field, one lane per node.  g arrays: [i][arr_nz][arr_ny][arr_nx] in the module's precision; map NULL: every node is wet.
// Operation order: the head of slf_thermal.hip.
struct ThermalConstants {
  double omega, t_ref, b[3];   // rounded once to the module's precision by the launchers
  int periodic[3];
};
hipError_t launch_thermal_init(const KernelSelector& sel, const Geometry& g, const ThermalConstants& k, const void* map,
                               const void* t_field, const void* const v[3], void* g0, void* field, hipStream_t s);
hipError_t launch_thermal_step(const KernelSelector& sel, const Geometry& g, const ThermalConstants& k, const void* map,
                               const void* src, void* dst, const void* const v[3], const void* wall_t, void* t_field,
                               void* field, hipStream_t s);

}  // namespace slf
