// C ABI of libsailfish_hip.so (see include/sailfish_hip.h for the contract and
// the reference interfaces each entry point replaces).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sailfish_hip.h"
#include "slf_bind.h"
#include "slf_kernels.h"
#include "slf_node.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(SLF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define SLF_HIP(call)                            \
  do {                                           \
    hipError_t _e = (call);                      \
    if (_e != hipSuccess) return hip_fail(_e, #call); \
  } while (0)

}  // namespace

struct slf_ctx {
  int device;
};
struct slf_stream {
  slf_ctx* ctx;
  hipStream_t s;
};
struct slf_event {
  slf_ctx* ctx;
  hipEvent_t e;
};
struct slf_graph {
  hipGraph_t graph;
  hipGraphExec_t exec;
};
struct slf_module : slf::ModuleConfig {   // sel, geo, phys, sc, fe, sc3, access_pattern, block_x, n_node_params (slf_bind.h)
  slf_ctx* ctx;
  void* node_params;  // device copy, in the module's precision
  uint32_t* status;   // device {flag, x, y, z} of the on-GPU invalid value check
  void* xsend[2];     // x-face buffers (slf_module_set_xface_buffers), NULL = unused
  void* xrecv[2];
  void* sc_send[3][2];  // binary Shan-Chen over connected x faces (slf_module_set_xface_planes): [lattice 0, lattice 1,
  void* sc_recv[3][2];  // densities][low / high face], NULL = unused
  slf::RowClasses rows;   // slf_module_classify_rows; rows.map == NULL: nothing classified
  void* rows_mem;         // one device allocation behind the tables of `rows`
  slf::SlotTable slots;   // indirect addressing: slot -> node, built from the `nodes` table of the first launch that names it
  void* slots_mem;
  int precision;
  // slf_module_update_node_params: pinned staging buffers for long updates, each with the event of its last copy
  void* stage[4];
  hipEvent_t stage_ev[4];
  size_t stage_bytes[4];
  int stage_next;
  void* accf;         // the acceleration field of an accel_field module (slf_module_set_accel_field), NULL = not set yet
};
struct slf_kernel {
  slf_module* mod;
  const slf::KernelRow* row;   // of slf::KERNEL_TABLE (slf_kernel_get)
  slf::KernelKind kind;        // = row->kind
  slf::BoundArgs args;         // slf_kernel_set_args
  int needs_iteration;
  uint32_t iteration;
  bool bound;
  slf::PairKnobs pair = {};    // slf_kernel_set_pair: every launch advances two steps (slf_pair.hip); rows == 0: single steps
};

static hipStream_t native(slf_stream* s) { return s ? s->s : (hipStream_t)0; }

// D3Q15 / D3Q27 modules: their lattice-dependent kernels live in slf_lat.hip, every other family refuses them by name
static bool on_lat(const slf_module* m) { return slf::is_lat_lattice(m->sel.lattice); }
static const char* lat_name(const slf_module* m) { return m->sel.lattice == SLF_D3Q15 ? "D3Q15" : "D3Q27"; }

// Indirect addressing: the slot -> node table of `nodes` (SlotTable, slf_kernels.h), built on first use and whenever a
// launch names another table.  SLF_INDIRECT_SLOTS=0: never (one thread per dense node, the round-3 kernels: A/B switch).
static const slf::SlotTable* slot_table_for(slf_module* m, const void* nodes, hipStream_t s) {
  static const bool enabled = [] { const char* v = getenv("SLF_INDIRECT_SLOTS"); return !(v && atoi(v) == 0); }();
  if (!enabled || !nodes || !m->geo.indirect) return nullptr;
  if (m->slots.nodes == nodes) return &m->slots;
  if (m->geo.lat_ny > 65535 || m->geo.lat_nz > 65535) return nullptr;
  if (m->slots_mem) {
    hipFree(m->slots_mem);
    m->slots_mem = nullptr;
  }
  m->slots = slf::SlotTable{};
  const size_t n = m->geo.dist_size;
  char* mem = nullptr;
  if (hipMalloc((void**)&mem, 2 * n * sizeof(uint32_t) + 256) != hipSuccess) return nullptr;
  uint32_t* max_slot = (uint32_t*)(mem + 2 * n * sizeof(uint32_t));
  uint32_t h = 0;
  hipError_t e = hipMemsetAsync(mem, 0xFF, 2 * n * sizeof(uint32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(max_slot, 0, 256, s);
  if (e == hipSuccess) e = slf::launch_build_slot_table(m->geo, nodes, (uint32_t*)mem, (uint32_t*)mem + n, max_slot, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&h, max_slot, sizeof(h), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    hipFree(mem);
    return nullptr;
  }
  m->slots_mem = mem;
  m->slots.nodes = nodes;
  m->slots.slot_gi = (const uint32_t*)mem;
  m->slots.slot_yz = (const uint32_t*)mem + n;
  m->slots.n_slots = h + 1;
  return &m->slots;
}

extern "C" {

int slf_abi_version(void) { return SLF_ABI_VERSION; }

const char* slf_last_error(void) { return g_last_error.c_str(); }

int slf_device_count(int* count) {
  if (!count) return fail(SLF_ERR_INVALID, "count is NULL");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  return SLF_OK;
}

int slf_device_pci_bus_id(int device, char* out, size_t len) {
  if (!out || len < 13) return fail(SLF_ERR_INVALID, "buffer of at least 13 bytes needed");
  SLF_HIP(hipDeviceGetPCIBusId(out, (int)len, device));
  return SLF_OK;
}

int slf_ctx_create(int device, slf_ctx** out) {
  if (!out) return fail(SLF_ERR_INVALID, "out is NULL");
  int n = 0;
  SLF_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(SLF_ERR_INVALID, "no such HIP device");
  SLF_HIP(hipSetDevice(device));
  slf_ctx* c = new slf_ctx;
  c->device = device;
  *out = c;
  return SLF_OK;
}

int slf_ctx_destroy(slf_ctx* ctx) {
  delete ctx;
  return SLF_OK;
}

int slf_ctx_sync(slf_ctx* ctx) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipDeviceSynchronize());
  return SLF_OK;
}

int slf_ctx_info(slf_ctx* ctx, char* name, size_t name_len, size_t* total_mem, int* cu_count, int* wavefront) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  hipDeviceProp_t prop;
  SLF_HIP(hipGetDeviceProperties(&prop, ctx->device));
  if (name && name_len) {
    snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (total_mem) *total_mem = prop.totalGlobalMem;
  if (cu_count) *cu_count = prop.multiProcessorCount;
  if (wavefront) *wavefront = prop.warpSize;
  return SLF_OK;
}

int slf_ctx_free_memory(slf_ctx* ctx, size_t* free_bytes) {
  if (!ctx || !free_bytes) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(ctx->device));
  size_t total = 0;
  SLF_HIP(hipMemGetInfo(free_bytes, &total));
  return SLF_OK;
}

int slf_malloc(slf_ctx* ctx, size_t bytes, void** dptr) {
  if (!ctx || !dptr) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipMalloc(dptr, bytes ? bytes : 1));
  return SLF_OK;
}

int slf_free(slf_ctx* ctx, void* dptr) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  if (dptr) SLF_HIP(hipFree(dptr));
  return SLF_OK;
}

int slf_memset(slf_ctx* ctx, void* dptr, int value, size_t bytes, slf_stream* stream) {
  if (!ctx || !dptr) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipMemsetAsync(dptr, value, bytes, native(stream)));
  if (!stream) SLF_HIP(hipStreamSynchronize(nullptr));   // no stream given: complete before returning
  return SLF_OK;
}

// ---- placed allocations: one virtual range, backed by separately created physical chunks -----------------
// (HIP virtual memory management: hipMemAddressReserve / hipMemCreate / hipMemMap)
int slf_vmm_granularity(slf_ctx* ctx, size_t* bytes) {
  if (!ctx || !bytes) return fail(SLF_ERR_INVALID, "NULL argument");
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = ctx->device;
  SLF_HIP(hipMemGetAllocationGranularity(bytes, &prop, hipMemAllocationGranularityRecommended));
  return SLF_OK;
}

int slf_vmm_reserve(slf_ctx* ctx, size_t bytes, void** va) {
  if (!ctx || !va) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipMemAddressReserve(va, bytes, 0, nullptr, 0));
  return SLF_OK;
}

int slf_vmm_release_range(slf_ctx* ctx, void* va, size_t bytes) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipMemAddressFree(va, bytes));
  return SLF_OK;
}

int slf_vmm_chunk_create(slf_ctx* ctx, size_t bytes, uint64_t* handle) {
  if (!ctx || !handle) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(ctx->device));
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = ctx->device;
  hipMemGenericAllocationHandle_t h;
  SLF_HIP(hipMemCreate(&h, bytes, &prop, 0));
  static_assert(sizeof(h) <= sizeof(uint64_t), "allocation handle does not fit the ABI type");
  *handle = 0;
  memcpy(handle, &h, sizeof(h));
  return SLF_OK;
}

int slf_vmm_chunk_release(slf_ctx* ctx, uint64_t handle) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  hipMemGenericAllocationHandle_t h;
  memcpy(&h, &handle, sizeof(h));
  SLF_HIP(hipMemRelease(h));
  return SLF_OK;
}

int slf_vmm_map(slf_ctx* ctx, void* va, size_t bytes, uint64_t handle) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipSetDevice(ctx->device));
  hipMemGenericAllocationHandle_t h;
  memcpy(&h, &handle, sizeof(h));
  SLF_HIP(hipMemMap(va, bytes, 0, h, 0));
  hipMemAccessDesc acc = {};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = ctx->device;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  SLF_HIP(hipMemSetAccess(va, bytes, &acc, 1));
  return SLF_OK;
}

int slf_vmm_unmap(slf_ctx* ctx, void* va, size_t bytes) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipMemUnmap(va, bytes));
  return SLF_OK;
}

// ---- device-to-device halo exchange over RCCL (xGMI) --------------------------------------------------------
// RCCL is bound at run time (dlopen): the library has no link-time dependency on it, and a process that already
// carries an RCCL (PyTorch bundles one) keeps exactly that one.
namespace {
struct RcclUniqueId {      // ncclUniqueId: 128 opaque bytes, passed by value
  char b[128];
};
struct RcclApi {
  void* handle = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, RcclUniqueId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
  int (*CommUserRank)(void*, int*) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;

int rccl_load() {
  if (g_rccl.handle) return SLF_OK;
  // exactly one RCCL per process, and the one that belongs to the HIP runtime in use: the copy next to the
  // libamdhip64 this library is bound to (a PyTorch wheel bundles both; torch.distributed will load that same
  // file), then whatever the loader finds
  std::vector<std::string> names;
  Dl_info info;
  if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
    std::string dir(info.dli_fname);
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos) names.push_back(dir.substr(0, slash) + "/librccl.so");
  }
  names.push_back("librccl.so");
  names.push_back("librccl.so.1");
  void* h = nullptr;
  for (const std::string& n : names) {           // one that is loaded already wins
    h = dlopen(n.c_str(), RTLD_NOW | RTLD_NOLOAD);
    if (h) break;
  }
  for (size_t i = 0; !h && i < names.size(); i++) h = dlopen(names[i].c_str(), RTLD_NOW | RTLD_GLOBAL);
  if (!h) return fail(SLF_ERR_NOT_FOUND, std::string("librccl not found: ") + dlerror());
#define SLF_SYM(field, name)                                                        \
  *(void**)(&g_rccl.field) = dlsym(h, name);                                        \
  if (!g_rccl.field) return fail(SLF_ERR_NOT_FOUND, std::string("librccl lacks ") + name);
  SLF_SYM(GetUniqueId, "ncclGetUniqueId")
  SLF_SYM(CommInitRank, "ncclCommInitRank")
  SLF_SYM(CommDestroy, "ncclCommDestroy")
  SLF_SYM(CommCount, "ncclCommCount")
  SLF_SYM(CommUserRank, "ncclCommUserRank")
  SLF_SYM(Send, "ncclSend")
  SLF_SYM(Recv, "ncclRecv")
  SLF_SYM(GroupStart, "ncclGroupStart")
  SLF_SYM(GroupEnd, "ncclGroupEnd")
  SLF_SYM(GetErrorString, "ncclGetErrorString")
#undef SLF_SYM
  g_rccl.handle = h;
  return SLF_OK;
}

int rccl_fail(int rc, const char* what) {
  return fail(SLF_ERR_HIP, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?"));
}
}  // namespace

struct slf_comm {
  slf_ctx* ctx;
  void* comm;
  int nranks, rank;
};

int slf_comm_unique_id(void* id128) {
  if (!id128) return fail(SLF_ERR_INVALID, "id buffer is NULL");
  if (int e = rccl_load()) return e;
  int rc = g_rccl.GetUniqueId(id128);
  return rc ? rccl_fail(rc, "ncclGetUniqueId") : SLF_OK;
}

int slf_comm_init(slf_ctx* ctx, int nranks, int rank, const void* unique_id, slf_comm** out) {
  if (!ctx || !unique_id || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  if (int e = rccl_load()) return e;
  SLF_HIP(hipSetDevice(ctx->device));
  RcclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  void* comm = nullptr;
  int rc = g_rccl.CommInitRank(&comm, nranks, id, rank);
  if (rc) return rccl_fail(rc, "ncclCommInitRank");
  *out = new slf_comm{ctx, comm, nranks, rank};
  return SLF_OK;
}

int slf_comm_destroy(slf_comm* c) {
  if (!c) return SLF_OK;
  int rc = g_rccl.CommDestroy(c->comm);
  delete c;
  return rc ? rccl_fail(rc, "ncclCommDestroy") : SLF_OK;
}

// What RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank), not what the caller passed to
// slf_comm_init(): the evidence a benchmark line carries that RCCL saw N ranks.
int slf_comm_count(slf_comm* c, int* nranks, int* rank) {
  if (!c) return fail(SLF_ERR_INVALID, "comm is NULL");
  int n = 0, r = 0;
  int rc = g_rccl.CommCount(c->comm, &n);
  if (rc) return rccl_fail(rc, "ncclCommCount");
  rc = g_rccl.CommUserRank(c->comm, &r);
  if (rc) return rccl_fail(rc, "ncclCommUserRank");
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  return SLF_OK;
}

int slf_comm_group_begin(void) {
  if (int e = rccl_load()) return e;
  int rc = g_rccl.GroupStart();
  return rc ? rccl_fail(rc, "ncclGroupStart") : SLF_OK;
}

int slf_comm_group_end(void) {
  if (int e = rccl_load()) return e;
  int rc = g_rccl.GroupEnd();
  return rc ? rccl_fail(rc, "ncclGroupEnd") : SLF_OK;
}

int slf_comm_sendrecv(slf_comm* c, int peer, const void* send_dptr, size_t n_send, void* recv_dptr, size_t n_recv,
                      int elem_bytes, slf_stream* stream) {
  if (!c) return fail(SLF_ERR_INVALID, "comm is NULL");
  if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 1) return fail(SLF_ERR_INVALID, "elem_bytes must be 1, 4 or 8");
  const int dtype = elem_bytes == 4 ? 7 /* ncclFloat32 */ : (elem_bytes == 8 ? 8 /* ncclFloat64 */ : 0 /* ncclInt8 */);
  SLF_HIP(hipSetDevice(c->ctx->device));
  int rc = g_rccl.GroupStart();
  if (rc) return rccl_fail(rc, "ncclGroupStart");
  if (n_send) rc = g_rccl.Send(send_dptr, n_send, dtype, peer, c->comm, native(stream));
  if (!rc && n_recv) rc = g_rccl.Recv(recv_dptr, n_recv, dtype, peer, c->comm, native(stream));
  int rc2 = g_rccl.GroupEnd();
  if (rc) return rccl_fail(rc, "ncclSend/ncclRecv");
  return rc2 ? rccl_fail(rc2, "ncclGroupEnd") : SLF_OK;
}

// One RCCL group of n point-to-point operations, posted in the given order (= the matching order between a pair of
// ranks) on `stream`: the whole batch of a halo exchange in one call.
int slf_comm_exchange(slf_comm* c, const slf_comm_op* ops, int n, slf_stream* stream) {
  if (!c || (!ops && n > 0)) return fail(SLF_ERR_INVALID, "NULL argument");
  if (n <= 0) return SLF_OK;
  SLF_HIP(hipSetDevice(c->ctx->device));
  int rc = g_rccl.GroupStart();
  if (rc) return rccl_fail(rc, "ncclGroupStart");
  for (int i = 0; i < n && !rc; i++) {
    const slf_comm_op& o = ops[i];
    if (o.elem_bytes != 4 && o.elem_bytes != 8 && o.elem_bytes != 1) {
      g_rccl.GroupEnd();
      return fail(SLF_ERR_INVALID, "elem_bytes must be 1, 4 or 8");
    }
    const int dtype = o.elem_bytes == 4 ? 7 /* ncclFloat32 */ : (o.elem_bytes == 8 ? 8 /* ncclFloat64 */ : 0 /* ncclInt8 */);
    if (o.count == 0) continue;
    if (o.kind == SLF_COMM_SEND) rc = g_rccl.Send(o.dptr, o.count, dtype, o.peer, c->comm, native(stream));
    else rc = g_rccl.Recv(o.dptr, o.count, dtype, o.peer, c->comm, native(stream));
  }
  const int rc2 = g_rccl.GroupEnd();
  if (rc) return rccl_fail(rc, "ncclSend/ncclRecv");
  return rc2 ? rccl_fail(rc2, "ncclGroupEnd") : SLF_OK;
}

// ---- peer transport: receive buffers mapped into the neighbouring processes, progress counters instead of messages ---
// (include/sailfish_hip.h "peer transport".)  The producers of a halo store into the neighbour's memory themselves;
// what these entry points add is the ordering.
namespace {
typedef unsigned long long peer_u64;
constexpr int PEER_SLOT = 8;        // 64-bit words per counter: every counter has a 64-byte line to itself
constexpr int PEER_MAX = 32;        // ranks per signal / wait call (a block decomposition has at most 26 neighbours)

struct PeerSignalArgs {
  peer_u64* flag[PEER_MAX];
  peer_u64 value[PEER_MAX];
  int n;
};
struct PeerWaitArgs {
  const peer_u64* flag[PEER_MAX];
  peer_u64 value[PEER_MAX];
  int rank[PEER_MAX];
  int n, channel;
  peer_u64 timeout;                 // ticks of the 100 MHz wall clock
  volatile long long* status;       // pinned host memory
};

// One lane per counter.  The release makes everything this PROCESS enqueued before the launch on the same stream
// visible first (slf_peer_signal records an event in front: a system-scope release of the whole device, not only of
// the one XCD this wave runs on).
__global__ void peer_signal_kernel(PeerSignalArgs a) {
  const int i = threadIdx.x;
  if (i < a.n) __hip_atomic_store(a.flag[i], a.value[i], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One lane per counter, spinning (with sleeps) until it has reached its value -- bounded: after `timeout` ticks the lane
// reports and gives up, so that a neighbour that died leaves an error on the host instead of a device nobody can use.
__global__ void peer_wait_kernel(PeerWaitArgs a) {
  const int i = threadIdx.x;
  if (i < a.n) {
    const peer_u64 t0 = wall_clock64();
    peer_u64 seen;
    while ((seen = __hip_atomic_load(a.flag[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) < a.value[i]) {
      __builtin_amdgcn_s_sleep(4);
      if (wall_clock64() - t0 > a.timeout) {
        a.status[1] = a.rank[i];
        a.status[2] = a.channel;
        a.status[3] = (long long)a.value[i];
        a.status[4] = (long long)seen;
        a.status[5] = a.status[5] + 1;
        a.status[0] = 1;
        break;
      }
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

__global__ void peer_fill_kernel(uint32_t* dst, size_t n, uint32_t pattern, int one_word_per_block) {
  if (one_word_per_block) {
    const size_t i = blockIdx.x;
    if (threadIdx.x == 0 && i < n) dst[i] = pattern ^ (uint32_t)i;
    return;
  }
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = pattern ^ (uint32_t)i;
}

__global__ void peer_check_kernel(const uint32_t* src, size_t n, uint32_t pattern, uint32_t* bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && src[i] != (pattern ^ (uint32_t)i)) atomicAdd(bad, 1u);
}
}  // namespace

struct slf_peer {
  slf_ctx* ctx;
  int nranks, rank;
  peer_u64* flags;                       // my block: counter[src rank][channel], PEER_SLOT words each
  std::vector<peer_u64*> remote;         // the blocks of the other ranks as mapped here (mine: flags)
  std::vector<peer_u64> sent, awaited;   // [rank * SLF_PEER_CHANNELS + channel]
  long long* status;                     // pinned host memory, 8 words
  peer_u64 timeout;
  hipEvent_t ev;
  uint32_t* bad;                         // device word of the self-test
};

static int peer_check_ranks(slf_peer* p, const int32_t* ranks, int n, int channel) {
  if (!p || (!ranks && n > 0)) return fail(SLF_ERR_INVALID, "NULL argument");
  if (n < 0 || n > PEER_MAX) return fail(SLF_ERR_INVALID, "at most 32 ranks per peer signal / wait");
  if (channel < 0 || channel >= SLF_PEER_CHANNELS) return fail(SLF_ERR_INVALID, "bad peer channel");
  for (int i = 0; i < n; i++) {
    if (ranks[i] < 0 || ranks[i] >= p->nranks) return fail(SLF_ERR_INVALID, "peer rank out of range");
    if (!p->remote[ranks[i]]) return fail(SLF_ERR_INVALID, "peer rank not connected (slf_peer_connect)");
  }
  return SLF_OK;
}

int slf_peer_create(slf_ctx* ctx, int nranks, int rank, slf_peer** out) {
  if (!ctx || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(SLF_ERR_INVALID, "bad rank / nranks");
  SLF_HIP(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)nranks * SLF_PEER_CHANNELS * PEER_SLOT * sizeof(peer_u64);
  void* f = nullptr;
  // uncached: a counter stored by another process (another device) is seen by the spinning lane without any cache
  // maintenance; fine-grained as the second choice
  if (hipExtMallocWithFlags(&f, bytes, hipDeviceMallocUncached) != hipSuccess) {
    (void)hipGetLastError();
    SLF_HIP(hipExtMallocWithFlags(&f, bytes, hipDeviceMallocFinegrained));
  }
  SLF_HIP(hipMemset(f, 0, bytes));
  slf_peer* p = new slf_peer;
  p->ctx = ctx;
  p->nranks = nranks;
  p->rank = rank;
  p->flags = (peer_u64*)f;
  p->remote.assign(nranks, nullptr);
  p->remote[rank] = p->flags;
  p->sent.assign((size_t)nranks * SLF_PEER_CHANNELS, 0);
  p->awaited.assign((size_t)nranks * SLF_PEER_CHANNELS, 0);
  p->status = nullptr;
  p->timeout = 60ull * 100000000ull;
  p->ev = nullptr;
  p->bad = nullptr;
  hipError_t e = hipHostMalloc((void**)&p->status, 8 * sizeof(long long), hipHostMallocMapped);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&p->bad, sizeof(uint32_t));
  if (e != hipSuccess) {
    slf_peer_destroy(p);
    return hip_fail(e, "slf_peer_create");
  }
  memset(p->status, 0, 8 * sizeof(long long));
  SLF_HIP(hipDeviceSynchronize());
  *out = p;
  return SLF_OK;
}

int slf_peer_destroy(slf_peer* p) {
  if (!p) return SLF_OK;
  for (int r = 0; r < p->nranks; r++)
    if (r != p->rank && p->remote[r]) hipIpcCloseMemHandle(p->remote[r]);
  if (p->flags) hipFree(p->flags);
  if (p->status) hipHostFree(p->status);
  if (p->ev) hipEventDestroy(p->ev);
  if (p->bad) hipFree(p->bad);
  delete p;
  return SLF_OK;
}

int slf_peer_flags_handle(slf_peer* p, void* handle64) {
  if (!p || !handle64) return fail(SLF_ERR_INVALID, "NULL argument");
  static_assert(sizeof(hipIpcMemHandle_t) == SLF_PEER_HANDLE_BYTES, "IPC handle size");
  hipIpcMemHandle_t h;
  SLF_HIP(hipIpcGetMemHandle(&h, p->flags));
  memcpy(handle64, &h, sizeof(h));
  return SLF_OK;
}

int slf_peer_connect(slf_peer* p, int rank, const void* handle64) {
  if (!p || !handle64) return fail(SLF_ERR_INVALID, "NULL argument");
  if (rank < 0 || rank >= p->nranks) return fail(SLF_ERR_INVALID, "peer rank out of range");
  if (rank == p->rank || p->remote[rank]) return SLF_OK;
  SLF_HIP(hipSetDevice(p->ctx->device));
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, sizeof(h));
  void* m = nullptr;
  SLF_HIP(hipIpcOpenMemHandle(&m, h, hipIpcMemLazyEnablePeerAccess));
  p->remote[rank] = (peer_u64*)m;
  return SLF_OK;
}

int slf_peer_alloc(slf_peer* p, size_t bytes, void** dptr, void* handle64) {
  if (!p || !dptr || !handle64) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(p->ctx->device));
  void* m = nullptr;
  SLF_HIP(hipMalloc(&m, bytes ? bytes : 1));      // plain (cacheable) memory: one-word stores merge into lines in the L2
  hipIpcMemHandle_t h;
  hipError_t e = hipIpcGetMemHandle(&h, m);
  if (e != hipSuccess) {
    hipFree(m);
    return hip_fail(e, "hipIpcGetMemHandle");
  }
  memcpy(handle64, &h, sizeof(h));
  *dptr = m;
  return SLF_OK;
}

int slf_peer_free(slf_peer* p, void* dptr) {
  if (!p) return fail(SLF_ERR_INVALID, "peer is NULL");
  if (dptr) SLF_HIP(hipFree(dptr));
  return SLF_OK;
}

int slf_peer_open(slf_peer* p, const void* handle64, void** mapped) {
  if (!p || !handle64 || !mapped) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(p->ctx->device));
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, sizeof(h));
  SLF_HIP(hipIpcOpenMemHandle(mapped, h, hipIpcMemLazyEnablePeerAccess));
  return SLF_OK;
}

int slf_peer_close(slf_peer* p, void* mapped) {
  if (!p) return fail(SLF_ERR_INVALID, "peer is NULL");
  if (mapped) SLF_HIP(hipIpcCloseMemHandle(mapped));
  return SLF_OK;
}

int slf_peer_signal(slf_peer* p, const int32_t* ranks, int n, int channel, slf_stream* stream) {
  if (int e = peer_check_ranks(p, ranks, n, channel)) return e;
  if (n == 0) return SLF_OK;
  SLF_HIP(hipSetDevice(p->ctx->device));
  // the stream's work so far, released to system scope by the command processor (every XCD's L2, not only the one the
  // signalling wave will run on): the writes into the neighbours' buffers are in memory before the counters move
  SLF_HIP(hipEventRecord(p->ev, native(stream)));
  PeerSignalArgs a;
  a.n = n;
  for (int i = 0; i < n; i++) {
    const size_t k = (size_t)ranks[i] * SLF_PEER_CHANNELS + channel;
    a.flag[i] = p->remote[ranks[i]] + ((size_t)p->rank * SLF_PEER_CHANNELS + channel) * PEER_SLOT;
    a.value[i] = ++p->sent[k];
  }
  hipLaunchKernelGGL(peer_signal_kernel, dim3(1), dim3(64), 0, native(stream), a);
  SLF_HIP(hipGetLastError());
  return SLF_OK;
}

int slf_peer_wait(slf_peer* p, const int32_t* ranks, int n, int channel, int count, slf_stream* stream) {
  if (int e = peer_check_ranks(p, ranks, n, channel)) return e;
  if (count < 1) return fail(SLF_ERR_INVALID, "peer wait: count must be at least 1");
  if (n == 0) return SLF_OK;
  SLF_HIP(hipSetDevice(p->ctx->device));
  PeerWaitArgs a;
  a.n = n;
  a.channel = channel;
  a.timeout = p->timeout;
  a.status = p->status;
  for (int i = 0; i < n; i++) {
    const size_t k = (size_t)ranks[i] * SLF_PEER_CHANNELS + channel;
    a.flag[i] = p->flags + k * PEER_SLOT;
    a.value[i] = (p->awaited[k] += (peer_u64)count);
    a.rank[i] = ranks[i];
  }
  hipLaunchKernelGGL(peer_wait_kernel, dim3(1), dim3(64), 0, native(stream), a);
  SLF_HIP(hipGetLastError());
  return SLF_OK;
}

int slf_peer_set_timeout(slf_peer* p, double seconds) {
  if (!p || !(seconds > 0)) return fail(SLF_ERR_INVALID, "bad argument");
  p->timeout = (peer_u64)(seconds * 1e8);
  return SLF_OK;
}

int slf_peer_status(slf_peer* p, int64_t out[8]) {
  if (!p || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  for (int i = 0; i < 8; i++) out[i] = (int64_t)((volatile long long*)p->status)[i];
  return SLF_OK;
}

int slf_peer_progress(slf_peer* p, int rank, int channel, uint64_t* sent, uint64_t* awaited, uint64_t* arrived) {
  if (!p) return fail(SLF_ERR_INVALID, "peer is NULL");
  if (rank < 0 || rank >= p->nranks || channel < 0 || channel >= SLF_PEER_CHANNELS) return fail(SLF_ERR_INVALID, "bad rank / channel");
  const size_t k = (size_t)rank * SLF_PEER_CHANNELS + channel;
  if (sent) *sent = p->sent[k];
  if (awaited) *awaited = p->awaited[k];
  if (arrived) {
    peer_u64 v = 0;
    SLF_HIP(hipMemcpy(&v, p->flags + k * PEER_SLOT, sizeof(v), hipMemcpyDeviceToHost));
    *arrived = v;
  }
  return SLF_OK;
}

int slf_peer_selftest_fill(slf_peer* p, void* dst, size_t nwords, uint32_t pattern, int one_word_per_block, slf_stream* stream) {
  if (!p || !dst) return fail(SLF_ERR_INVALID, "NULL argument");
  if (nwords == 0) return SLF_OK;
  SLF_HIP(hipSetDevice(p->ctx->device));
  const unsigned blocks = one_word_per_block ? (unsigned)nwords : (unsigned)((nwords + 255) / 256);
  hipLaunchKernelGGL(peer_fill_kernel, dim3(blocks), dim3(one_word_per_block ? 64 : 256), 0, native(stream), (uint32_t*)dst, nwords,
                     pattern, one_word_per_block);
  SLF_HIP(hipGetLastError());
  return SLF_OK;
}

int slf_peer_selftest_check(slf_peer* p, const void* src, size_t nwords, uint32_t pattern, slf_stream* stream, uint32_t* bad_words) {
  if (!p || !src || !bad_words) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(p->ctx->device));
  SLF_HIP(hipMemsetAsync(p->bad, 0, sizeof(uint32_t), native(stream)));
  if (nwords)
    hipLaunchKernelGGL(peer_check_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, native(stream), (const uint32_t*)src,
                       nwords, pattern, p->bad);
  SLF_HIP(hipGetLastError());
  SLF_HIP(hipMemcpyAsync(bad_words, p->bad, sizeof(uint32_t), hipMemcpyDeviceToHost, native(stream)));
  SLF_HIP(hipStreamSynchronize(native(stream)));
  return SLF_OK;
}

int slf_host_alloc_pinned(size_t bytes, void** hptr) {
  if (!hptr) return fail(SLF_ERR_INVALID, "hptr is NULL");
  SLF_HIP(hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
  return SLF_OK;
}

int slf_host_free(void* hptr) {
  if (hptr) SLF_HIP(hipHostFree(hptr));
  return SLF_OK;
}

int slf_memcpy_h2d(slf_ctx* ctx, void* dptr, const void* hptr, size_t bytes) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipMemcpy(dptr, hptr, bytes, hipMemcpyHostToDevice));
  return SLF_OK;
}

int slf_memcpy_d2h(slf_ctx* ctx, void* hptr, const void* dptr, size_t bytes) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipMemcpy(hptr, dptr, bytes, hipMemcpyDeviceToHost));
  return SLF_OK;
}

int slf_memcpy_h2d_async(slf_ctx* ctx, void* dptr, const void* hptr, size_t bytes, slf_stream* s) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, native(s)));
  return SLF_OK;
}

int slf_memcpy_d2h_async(slf_ctx* ctx, void* hptr, const void* dptr, size_t bytes, slf_stream* s) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, native(s)));
  return SLF_OK;
}

int slf_memcpy_d2d_async(slf_ctx* ctx, void* dst, const void* src, size_t bytes, slf_stream* s) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, native(s)));
  return SLF_OK;
}

int slf_memcpy_peer_async(slf_ctx* ctx, void* dst, int dst_device, const void* src, int src_device, size_t bytes,
                          slf_stream* s) {
  if (!ctx) return fail(SLF_ERR_INVALID, "ctx is NULL");
  SLF_HIP(hipSetDevice(ctx->device));
  SLF_HIP(hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes, native(s)));
  return SLF_OK;
}

static int stream_create(slf_ctx* ctx, bool high_priority, slf_stream** out) {
  if (!ctx || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(ctx->device));
  int least = 0, greatest = 0;
  if (high_priority) SLF_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  slf_stream* s = new slf_stream;
  s->ctx = ctx;
  hipError_t e = high_priority ? hipStreamCreateWithPriority(&s->s, hipStreamNonBlocking, greatest)
                               : hipStreamCreateWithFlags(&s->s, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete s;
    return hip_fail(e, "hipStreamCreate");
  }
  *out = s;
  return SLF_OK;
}

int slf_stream_create(slf_ctx* ctx, slf_stream** out) { return stream_create(ctx, false, out); }

// The halo stream: its small pack / unpack kernels (and whatever waits behind them) are dispatched ahead of the bulk
// sweep's remaining workgroups instead of queueing behind a full chip.
int slf_stream_create_high_priority(slf_ctx* ctx, slf_stream** out) { return stream_create(ctx, true, out); }

int slf_stream_destroy(slf_stream* s) {
  if (s) {
    hipStreamDestroy(s->s);
    delete s;
  }
  return SLF_OK;
}

int slf_stream_sync(slf_stream* s) {
  SLF_HIP(hipStreamSynchronize(native(s)));
  return SLF_OK;
}

int slf_stream_native(slf_stream* s, void** hip_stream) {
  if (!hip_stream) return fail(SLF_ERR_INVALID, "hip_stream is NULL");
  *hip_stream = (void*)native(s);
  return SLF_OK;
}

int slf_graph_capture_begin(slf_stream* s) {
  if (!s) return fail(SLF_ERR_INVALID, "graph capture needs a stream created with slf_stream_create");
  // relaxed: a destructor that frees device memory while we record (Python's garbage collector can run one at
  // any time) must not invalidate the capture
  SLF_HIP(hipStreamBeginCapture(s->s, hipStreamCaptureModeRelaxed));
  return SLF_OK;
}

int slf_graph_capture_end(slf_stream* s, slf_graph** out) {
  if (!s || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  hipGraph_t graph = nullptr;
  SLF_HIP(hipStreamEndCapture(s->s, &graph));
  if (!graph) return fail(SLF_ERR_HIP, "stream capture produced no graph");
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    hipGraphDestroy(graph);
    return fail(SLF_ERR_HIP, hipGetErrorString(e));
  }
  slf_graph* g = new slf_graph;
  g->graph = graph;
  g->exec = exec;
  *out = g;
  return SLF_OK;
}

int slf_graph_launch(slf_graph* g, slf_stream* s) {
  if (!g) return fail(SLF_ERR_INVALID, "graph is NULL");
  if (s && s->ctx) SLF_HIP(hipSetDevice(s->ctx->device));
  SLF_HIP(hipGraphLaunch(g->exec, native(s)));
  return SLF_OK;
}

int slf_graph_destroy(slf_graph* g) {
  if (!g) return SLF_OK;
  hipGraphExecDestroy(g->exec);
  hipGraphDestroy(g->graph);
  delete g;
  return SLF_OK;
}

int slf_stream_wait_event(slf_stream* s, slf_event* ev) {
  if (!ev) return fail(SLF_ERR_INVALID, "event is NULL");
  if (s && s->ctx) SLF_HIP(hipSetDevice(s->ctx->device));      // the waiting stream's device; the event may belong to another
  SLF_HIP(hipStreamWaitEvent(native(s), ev->e, 0));
  return SLF_OK;
}

int slf_event_create(slf_ctx* ctx, int timing, slf_event** out) {
  if (!ctx || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipSetDevice(ctx->device));
  slf_event* ev = new slf_event;
  ev->ctx = ctx;
  hipError_t e = hipEventCreateWithFlags(&ev->e, timing ? hipEventDefault : hipEventDisableTiming);
  if (e != hipSuccess) {
    delete ev;
    return hip_fail(e, "hipEventCreateWithFlags");
  }
  *out = ev;
  return SLF_OK;
}

int slf_event_destroy(slf_event* ev) {
  if (ev) {
    hipEventDestroy(ev->e);
    delete ev;
  }
  return SLF_OK;
}

int slf_event_record(slf_event* ev, slf_stream* s) {
  if (!ev) return fail(SLF_ERR_INVALID, "event is NULL");
  if (ev->ctx) SLF_HIP(hipSetDevice(ev->ctx->device));
  SLF_HIP(hipEventRecord(ev->e, native(s)));
  return SLF_OK;
}

int slf_event_sync(slf_event* ev) {
  if (!ev) return fail(SLF_ERR_INVALID, "event is NULL");
  SLF_HIP(hipEventSynchronize(ev->e));
  return SLF_OK;
}

int slf_event_elapsed_ms(slf_event* start, slf_event* end, float* ms) {
  if (!start || !end || !ms) return fail(SLF_ERR_INVALID, "NULL argument");
  SLF_HIP(hipEventElapsedTime(ms, start->e, end->e));
  return SLF_OK;
}

int slf_module_create(slf_ctx* ctx, const slf_module_desc* d, slf_module** out) {
  if (!ctx || !d || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  slf::ModuleConfig cfg;
  const char* why = nullptr;
  if (int rc = slf::module_config(d, &cfg, &why)) return fail(rc, why);
  slf_module* m = new slf_module();     // everything the configuration does not hold: zero / NULL
  static_cast<slf::ModuleConfig&>(*m) = cfg;
  m->ctx = ctx;
  m->precision = d->precision;
  auto bail = [m](hipError_t e, const char* what) {      // frees what has been allocated by then
    slf_module_destroy(m);
    return hip_fail(e, what);
  };
  const int np = d->n_node_params > 0 ? d->n_node_params : 1;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMalloc(&m->node_params, (size_t)np * d->precision);
  if (e != hipSuccess) return bail(e, "hipMalloc(node_params)");
  if (d->precision == 4) {
    std::vector<float> tmp(np, 0.0f);
    for (int i = 0; i < d->n_node_params; i++) tmp[i] = (float)d->node_params[i];
    e = hipMemcpy(m->node_params, tmp.data(), np * sizeof(float), hipMemcpyHostToDevice);
  } else {
    std::vector<double> tmp(np, 0.0);
    for (int i = 0; i < d->n_node_params; i++) tmp[i] = d->node_params[i];
    e = hipMemcpy(m->node_params, tmp.data(), np * sizeof(double), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) return bail(e, "hipMemcpy(node_params)");
  e = hipMalloc((void**)&m->status, 4 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(m->status, 0, 4 * sizeof(uint32_t));
  if (e != hipSuccess) return bail(e, "hipMalloc(status)");
  *out = m;
  return SLF_OK;
}

int slf_module_destroy(slf_module* m) {
  if (m) {
    if (m->node_params) hipFree(m->node_params);
    if (m->status) hipFree(m->status);
    if (m->rows_mem) hipFree(m->rows_mem);
    if (m->slots_mem) hipFree(m->slots_mem);
    for (int i = 0; i < 4; i++) {
      if (m->stage[i]) hipHostFree(m->stage[i]);
      if (m->stage_ev[i]) hipEventDestroy(m->stage_ev[i]);
    }
    delete m;
  }
  return SLF_OK;
}

// Row classes of a node map (RowClasses, slf_kernels.h): which 64-node segments are plain fluid (their waves skip the
// map), which rows hold boundary-condition nodes (swept by a second launch of the full instantiation, so that all
// other rows run the small one).  Optional: without it every wave reads the map and the whole subdomain runs the
// instantiation for the module's node-type table.  Call again after the map's contents changed.
int slf_module_classify_rows(slf_module* m, const void* map_dptr, slf_stream* stream, int32_t out_counts[4]) {
  if (!m) return fail(SLF_ERR_INVALID, "module is NULL");
  const slf::Geometry& g = m->geo;
  if (m->rows_mem) {
    SLF_HIP(hipFree(m->rows_mem));
    m->rows_mem = nullptr;
  }
  m->rows = slf::RowClasses{};
  if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
  if (!map_dptr) return SLF_OK;                                   // forget the tables
  if (on_lat(m)) return fail(SLF_ERR_UNSUPPORTED, std::string(lat_name(m)) + ": row classes belong to the D3Q19 whole-row kernels");
  if (!m->sel.general || m->sel.lattice != 1 || g.indirect || !(g.variant & 8))
    return fail(SLF_ERR_UNSUPPORTED, "row classes: D3Q19 modules with a node map and direct addressing (whole-row kernels) only");
  SLF_HIP(hipSetDevice(m->ctx->device));
  const int nx = g.lat_nx - 2;
  const int nseg = (nx + 63) / 64;
  const size_t nrows_arr = (size_t)g.arr_ny * (size_t)g.arr_nz;
  const size_t seg_bytes = (nrows_arr * (size_t)nseg + 255) / 256 * 256 + 256;     // + slack: idle waves behind the last segment
  const size_t row_bytes = (nrows_arr + 255) / 256 * 256;
  const size_t list_bytes = ((size_t)(g.lat_ny - 2) * (size_t)(g.lat_nz - 2) * 4 + 255) / 256 * 256;
  char* mem = nullptr;
  SLF_HIP(hipMalloc((void**)&mem, seg_bytes + row_bytes + list_bytes + 256));
  hipStream_t s = native(stream);
  hipError_t e = hipMemsetAsync(mem, 1, seg_bytes + row_bytes, s);          // ghost rows: "mixed", never used
  if (e == hipSuccess) e = hipMemsetAsync(mem + seg_bytes + row_bytes, 0, list_bytes + 256, s);
  uint32_t* counters = (uint32_t*)(mem + seg_bytes + row_bytes + list_bytes);
  if (e == hipSuccess)
    e = slf::launch_classify_rows(g, map_dptr, (uint32_t*)mem, (uint8_t*)(mem + seg_bytes),
                                  (uint32_t*)(mem + seg_bytes + row_bytes), counters, nseg, s);
  uint32_t h[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(h, counters, sizeof(h), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    hipFree(mem);
    return hip_fail(e, "slf_module_classify_rows");
  }
  m->rows_mem = mem;
  m->rows.map = map_dptr;
  m->rows.seg_class = (const uint32_t*)mem;
  m->rows.row_class = (const uint8_t*)(mem + seg_bytes);
  m->rows.bc_rows = (const uint32_t*)(mem + seg_bytes + row_bytes);
  m->rows.nseg = nseg;
  m->rows.n_rows = (g.lat_ny - 2) * (g.dim == 3 ? g.lat_nz - 2 : 1);
  m->rows.n_bc_rows = (int)h[0];
  m->rows.n_fluid_segments = h[1];
  m->rows.n_segments = (long long)m->rows.n_rows * nseg;
  if (out_counts) {
    out_counts[0] = m->rows.n_rows;
    out_counts[1] = m->rows.n_bc_rows;
    out_counts[2] = (int32_t)(m->rows.n_segments > 0x7fffffff ? 0x7fffffff : m->rows.n_segments);
    out_counts[3] = (int32_t)(m->rows.n_fluid_segments > 0x7fffffff ? 0x7fffffff : m->rows.n_fluid_segments);
  }
  return SLF_OK;
}

namespace {
constexpr int PARAM_UPDATE_MAX = 256;
struct ParamUpdateF {
  float v[PARAM_UPDATE_MAX];
  int n;
};
struct ParamUpdateD {
  double v[PARAM_UPDATE_MAX];
  int n;
};
__global__ void update_params_kernel_f(float* table, ParamUpdateF u) {
  for (int i = threadIdx.x; i < u.n; i += blockDim.x) table[i] = u.v[i];
}
__global__ void update_params_kernel_d(double* table, ParamUpdateD u) {
  for (int i = threadIdx.x; i < u.n; i += blockDim.x) table[i] = u.v[i];
}
}  // namespace

int slf_module_update_node_params(slf_module* m, int first, const double* values, int n, slf_stream* stream) {
  if (!m || (!values && n > 0)) return fail(SLF_ERR_INVALID, "NULL argument");
  if (n <= 0) return SLF_OK;
  if (first < 0 || first + n > m->n_node_params) return fail(SLF_ERR_INVALID, "node parameter range outside the module's table");
  SLF_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = native(stream);
  char* dst = (char*)m->node_params + (size_t)first * m->precision;
  if (n <= PARAM_UPDATE_MAX) {
    // the values travel as kernel arguments: nothing the host must keep alive, nothing that could make the call wait
    if (m->precision == 4) {
      ParamUpdateF u;
      u.n = n;
      for (int i = 0; i < n; i++) u.v[i] = (float)values[i];
      hipLaunchKernelGGL(update_params_kernel_f, dim3(1), dim3(64), 0, s, (float*)dst, u);
    } else {
      ParamUpdateD u;
      u.n = n;
      for (int i = 0; i < n; i++) u.v[i] = values[i];
      hipLaunchKernelGGL(update_params_kernel_d, dim3(1), dim3(64), 0, s, (double*)dst, u);
    }
    SLF_HIP(hipGetLastError());
    return SLF_OK;
  }
  // long updates (a value per node of an inlet): through one of four pinned staging buffers, reused once its last copy is done
  const int k = m->stage_next;
  m->stage_next = (k + 1) & 3;
  const size_t bytes = (size_t)n * m->precision;
  if (m->stage_ev[k]) SLF_HIP(hipEventSynchronize(m->stage_ev[k]));
  else SLF_HIP(hipEventCreateWithFlags(&m->stage_ev[k], hipEventDisableTiming));
  if (m->stage_bytes[k] < bytes) {
    if (m->stage[k]) SLF_HIP(hipHostFree(m->stage[k]));
    m->stage[k] = nullptr;
    SLF_HIP(hipHostMalloc(&m->stage[k], bytes, hipHostMallocDefault));
    m->stage_bytes[k] = bytes;
  }
  if (m->precision == 4) for (int i = 0; i < n; i++) ((float*)m->stage[k])[i] = (float)values[i];
  else memcpy(m->stage[k], values, bytes);
  SLF_HIP(hipMemcpyAsync(dst, m->stage[k], bytes, hipMemcpyHostToDevice, s));
  SLF_HIP(hipEventRecord(m->stage_ev[k], s));
  return SLF_OK;
}

int slf_module_set_body_force(slf_module* m, int lattice, const double accel[3]) {
  if (!m || !accel) return fail(SLF_ERR_INVALID, "NULL argument");
  if (lattice == 0) {
    if (!m->phys.has_force) return fail(SLF_ERR_INVALID, "the module was created without a body force (has_force)");
    for (int i = 0; i < 3; i++) m->phys.accel[i] = accel[i];
  } else if (lattice == 1) {
    if (m->sc3.enabled) {
      for (int i = 0; i < 3; i++) m->sc3.accel1[i] = accel[i];
      return SLF_OK;
    }
    if (m->sc.enabled != 1) return fail(SLF_ERR_INVALID, "lattice 1 exists in binary models only");
    for (int i = 0; i < 3; i++) m->sc.accel1[i] = accel[i];
  } else if (lattice == 2) {
    if (!m->sc3.enabled) return fail(SLF_ERR_INVALID, "lattice 2 exists in ternary models (simtype = SLF_SIM_SHAN_CHEN_TERNARY) only");
    for (int i = 0; i < 3; i++) m->sc3.accel2[i] = accel[i];
  } else {
    return fail(SLF_ERR_INVALID, "lattice must be 0, 1 or 2");
  }
  return SLF_OK;
}

int slf_module_set_accel_field(slf_module* m, void* field) {
  if (!m) return fail(SLF_ERR_INVALID, "module is NULL");
  if (!m->phys.accel_field) return fail(SLF_ERR_INVALID, "the module was created without an acceleration field (accel_field)");
  if (!field) return fail(SLF_ERR_INVALID, "slf_module_set_accel_field: field is NULL");
  m->accf = field;
  return SLF_OK;
}

int slf_module_poll_invalid(slf_module* m, slf_stream* stream, int32_t out[4]) {
  if (!m || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  uint32_t h[4] = {0, 0, 0, 0};
  SLF_HIP(hipSetDevice(m->ctx->device));
  SLF_HIP(hipMemcpyAsync(h, m->status, sizeof(h), hipMemcpyDeviceToHost, native(stream)));
  SLF_HIP(hipStreamSynchronize(native(stream)));
  for (int i = 0; i < 4; i++) out[i] = (int32_t)h[i];
  if (h[0]) SLF_HIP(hipMemsetAsync(m->status, 0, sizeof(h), native(stream)));
  return SLF_OK;
}

// The four pointers of a module's x-face buffers (set < 0) or of its plane set `set` (0 / 1: lattice, 2: densities), in the
// order send low, send high, receive low, receive high (checked by slf_bind.h part (f)).
static void store_xface(slf_module* m, int set, void* const xf[4]) {
  void** send = set < 0 ? m->xsend : m->sc_send[set];
  void** recv = set < 0 ? m->xrecv : m->sc_recv[set];
  send[0] = xf[0]; send[1] = xf[1];
  recv[0] = xf[2]; recv[1] = xf[3];
}

int slf_module_set_xface_buffers(slf_module* m, void* send_low, void* send_high, void* recv_low, void* recv_high) {
  void* const xf[4] = {send_low, send_high, recv_low, recv_high};
  std::string why;
  if (int rc = slf::xface_buffers_check(m, xf, &why)) return fail(rc, why);
  store_xface(m, -1, xf);
  return SLF_OK;
}

// x-face planes of the binary model into the launch arguments; all six faces' worth or none (a sweep without the density
// planes would read ghost columns nobody fills)
static void sc_planes_of(const slf_module* m, slf::SweepArgs& a) {
  for (int f = 0; f < 2; f++) {
    a.xsend[f] = m->sc_send[0][f];   a.xrecv[f] = m->sc_recv[0][f];
    a.xsend2[f] = m->sc_send[1][f];  a.xrecv2[f] = m->sc_recv[1][f];
    a.msend[f] = m->sc_send[2][f];   a.mrecv[f] = m->sc_recv[2][f];
  }
}

int slf_module_set_xface_planes(slf_module* m, int32_t which, void* send_low, void* send_high, void* recv_low,
                                void* recv_high) {
  void* const xf[4] = {send_low, send_high, recv_low, recv_high};
  std::string why;
  if (int rc = slf::xface_planes_check(m, which, xf, &why)) return fail(rc, why);
  store_xface(m, which, xf);
  return SLF_OK;
}

// The ghost columns x = 0 (low) / x = nx + 1 (high) of this subdomain carry nothing the simulation uses (contract:
// include/sailfish_hip.h): the whole-row sweeps neither push into them nor pull out of them.  Refused for a face the
// module itself needs: x periodic without in-sweep wrap.
int slf_module_set_x_ghost_unused(slf_module* m, int low, int high) {
  if (!m) return fail(SLF_ERR_INVALID, "module is NULL");
  if ((low || high) && m->geo.axis_mode[0] == 1)
    return fail(SLF_ERR_INVALID, "x is periodic through the ghost-layer kernels: its ghost columns are read");
  m->geo.x_ghost_unused = (low ? 1 : 0) | (high ? 2 : 0);
  return SLF_OK;
}

int slf_module_block_size(slf_module* m, int* threads) {
  if (!m || !threads) return fail(SLF_ERR_INVALID, "NULL argument");
  *threads = m->block_x;
  return SLF_OK;
}

// ---- flow statistics (slf_stats.hip) ----------------------------------------------------------------------------
static int check_stats_module(const slf_module* m, const char* what) {
  if (!m) return fail(SLF_ERR_INVALID, "module is NULL");
  if (m->geo.dim != 3) return fail(SLF_ERR_UNSUPPORTED, std::string(what) + ": 3-D modules only (the statistics read vx, vy and vz)");
  return SLF_OK;
}

int slf_stats_workspace_bytes(slf_module* m, int what, size_t* bytes) {
  if (int e = check_stats_module(m, "slf_stats_workspace_bytes")) return e;
  if (!bytes) return fail(SLF_ERR_INVALID, "bytes is NULL");
  if (what < SLF_STATS_KE_ENSTROPHY || what > SLF_STATS_PROFILES_Z)
    return fail(SLF_ERR_INVALID, "slf_stats_workspace_bytes: what = SLF_STATS_KE_ENSTROPHY | SLF_STATS_PROFILES_X / _Y / _Z");
  const slf::StatsShape sh = what == SLF_STATS_KE_ENSTROPHY ? slf::stats_ke_shape(m->geo)
                                                            : slf::stats_profiles_shape(m->geo, what - SLF_STATS_PROFILES_X);
  *bytes = sh.workspace_doubles * sizeof(double);
  return SLF_OK;
}

int slf_stats_ke_enstrophy(slf_module* m, const void* map, const void* vx, const void* vy, const void* vz, void* v_sq,
                           void* vort_sq, void* workspace, double* out2, slf_stream* stream) {
  if (int e = check_stats_module(m, "slf_stats_ke_enstrophy")) return e;
  if (!vx || !vy || !vz) return fail(SLF_ERR_INVALID, "slf_stats_ke_enstrophy: a velocity field is NULL");
  if (!workspace || !out2) return fail(SLF_ERR_INVALID, "slf_stats_ke_enstrophy: workspace / out2 is NULL");
  if ((v_sq == nullptr) != (vort_sq == nullptr))
    return fail(SLF_ERR_INVALID, "slf_stats_ke_enstrophy: v_sq and vort_sq are stored together or not at all");
  const slf::Geometry& g = m->geo;
  if (g.lat_nx < 4 || g.lat_ny < 4 || g.lat_nz < 4)
    return fail(SLF_ERR_INVALID, "slf_stats_ke_enstrophy: an extent of 1 leaves the one-sided difference nothing but the ghost layer");
  SLF_HIP(hipSetDevice(m->ctx->device));
  const void* v[3] = {vx, vy, vz};
  SLF_HIP(slf::launch_stats_ke_enstrophy(m->sel, g, map, v, v_sq, vort_sq, (double*)workspace, out2, native(stream)));
  return SLF_OK;
}

int slf_stats_profiles(slf_module* m, int axis, const void* vx, const void* vy, const void* vz, const void* rho,
                       void* workspace, double* out, size_t out_stride, size_t offset, slf_stream* stream) {
  if (int e = check_stats_module(m, "slf_stats_profiles")) return e;
  if (axis < 0 || axis > 2) return fail(SLF_ERR_INVALID, "slf_stats_profiles: axis = 0 (x) | 1 (y) | 2 (z)");
  if (!vx || !vy || !vz || !rho) return fail(SLF_ERR_INVALID, "slf_stats_profiles: a field is NULL");
  if (!workspace || !out) return fail(SLF_ERR_INVALID, "slf_stats_profiles: workspace / out is NULL");
  const slf::Geometry& g = m->geo;
  const int n = (axis == 0 ? g.lat_nx : axis == 1 ? g.lat_ny : g.lat_nz) - 2;
  if (offset + (size_t)n > out_stride)
    return fail(SLF_ERR_INVALID, "slf_stats_profiles: offset + positions exceeds out_stride (the snapshot would run into the next statistic)");
  SLF_HIP(hipSetDevice(m->ctx->device));
  const void* v[3] = {vx, vy, vz};
  SLF_HIP(slf::launch_stats_profiles(m->sel, g, axis, v, rho, (double*)workspace, out, out_stride, offset, native(stream)));
  return SLF_OK;
}

// ---- force on bodies by momentum exchange (slf_force.hip) --------------------------------------------------------
static int check_force_call(const slf_module* m, int n_objects, uint32_t max_links, const char* what) {
  if (!m) return fail(SLF_ERR_INVALID, "module is NULL");
  if (on_lat(m)) return fail(SLF_ERR_UNSUPPORTED, std::string(what) + ": force objects are not implemented on " + lat_name(m));
  if (m->sc.enabled || m->fe.enabled || m->sc3.enabled)
    return fail(SLF_ERR_UNSUPPORTED, std::string(what) + ": single-fluid modules only (the force is read off lattice 0 alone)");
  if (n_objects < 0 || n_objects > 65535) return fail(SLF_ERR_INVALID, std::string(what) + ": 0 .. 65535 objects per call");
  if (max_links > 0x7FFFFFFFu) return fail(SLF_ERR_INVALID, std::string(what) + ": fewer than 2^31 links");
  return SLF_OK;
}

int slf_force_workspace_bytes(slf_module* m, int n_objects, uint32_t max_links, size_t* bytes) {
  if (int e = check_force_call(m, n_objects, max_links, "slf_force_workspace_bytes")) return e;
  if (!bytes) return fail(SLF_ERR_INVALID, "bytes is NULL");
  *bytes = slf::force_shape(n_objects, max_links).workspace_doubles * sizeof(double);
  return SLF_OK;
}

int slf_force_objects(slf_module* m, const void* dist, const uint32_t* idx, const uint32_t* idx2, const uint8_t* dir,
                      const uint32_t* seg, int n_objects, uint32_t max_links, void* workspace, double* out,
                      slf_stream* stream) {
  if (int e = check_force_call(m, n_objects, max_links, "slf_force_objects")) return e;
  if (n_objects == 0) return SLF_OK;
  if (!dist || !seg || !out) return fail(SLF_ERR_INVALID, "slf_force_objects: dist / seg / out is NULL");
  if (max_links && (!idx || !idx2 || !dir)) return fail(SLF_ERR_INVALID, "slf_force_objects: a link table is NULL");
  if (slf::force_shape(n_objects, max_links).workspace_doubles && !workspace)
    return fail(SLF_ERR_INVALID, "slf_force_objects: workspace is NULL (slf_force_workspace_bytes)");
  SLF_HIP(hipSetDevice(m->ctx->device));
  SLF_HIP(slf::launch_force_objects(m->sel, dist, idx, idx2, dir, seg, n_objects, max_links, (double*)workspace, out,
                                    native(stream)));
  return SLF_OK;
}

// ---- immersed boundary markers (slf_ibm.hip; argument checks: slf_bind.h ibm_check) ------------------------------
static int check_ibm_call(const slf_module* m, const char* what, int n, const int32_t* origin, const void* const* ptrs,
                          const char* const* names, int n_ptrs) {
  if (!m) return fail(SLF_ERR_INVALID, "module is NULL");
  std::string why;
  if (int rc = slf::ibm_check(*m, m->accf != nullptr, what, n, origin, ptrs, names, n_ptrs, &why)) return fail(rc, why);
  return SLF_OK;
}

int slf_ibm_workspace_bytes(slf_module* m, size_t* bytes) {
  if (!m || !bytes) return fail(SLF_ERR_INVALID, "NULL argument");
  if (!m->phys.accel_field)
    return fail(SLF_ERR_INVALID, "slf_ibm_workspace_bytes: the module was created without an acceleration field (accel_field)");
  *bytes = slf::ibm_accumulator_bytes(m->geo);
  return SLF_OK;
}

int slf_ibm_spread(slf_module* m, int n_markers, const int32_t origin[3], const void* pos, const void* ref,
                   const void* stiffness, void* acc, slf_stream* stream) {
  const void* ptrs[] = {pos, ref, stiffness, acc};
  const char* names[] = {"pos", "ref", "stiffness", "acc"};
  if (int e = check_ibm_call(m, "slf_ibm_spread", n_markers, origin, ptrs, names, 4)) return e;
  SLF_HIP(hipSetDevice(m->ctx->device));
  SLF_HIP(slf::launch_ibm_spread(m->sel, m->geo, origin, n_markers, pos, ref, stiffness, acc, native(stream)));
  return SLF_OK;
}

int slf_ibm_gather(slf_module* m, int n_markers, const int32_t origin[3], const void* pos, const void* acc,
                   slf_stream* stream) {
  const void* ptrs[] = {pos, acc};
  const char* names[] = {"pos", "acc"};
  if (int e = check_ibm_call(m, "slf_ibm_gather", n_markers, origin, ptrs, names, 2)) return e;
  SLF_HIP(hipSetDevice(m->ctx->device));
  SLF_HIP(slf::launch_ibm_gather(m->sel, m->geo, origin, n_markers, pos, acc, m->accf, native(stream)));
  return SLF_OK;
}

int slf_ibm_clear_and_advect(slf_module* m, int n_markers, const int32_t origin[3], void* pos, void* acc, const void* map,
                             const void* vx, const void* vy, const void* vz, uint32_t* outside, slf_stream* stream) {
  const void* ptrs[] = {pos, acc, vx, vy, outside, vz};
  const char* names[] = {"pos", "acc", "vx", "vy", "outside", "vz"};
  if (int e = check_ibm_call(m, "slf_ibm_clear_and_advect", n_markers, origin, ptrs, names, m && m->geo.dim == 3 ? 6 : 5))
    return e;
  if (!map && m->sel.general)
    return fail(SLF_ERR_INVALID, "slf_ibm_clear_and_advect: map is NULL, but the module has node types (which nodes are wet "
                                 "is read off the node map)");
  SLF_HIP(hipSetDevice(m->ctx->device));
  const void* v[3] = {vx, vy, vz};
  SLF_HIP(slf::launch_ibm_clear_and_advect(m->sel, m->geo, origin, n_markers, pos, acc, m->accf, map, v, outside,
                                           native(stream)));
  return SLF_OK;
}

// ---- thermal flows (slf_thermal.hip; argument checks: slf_bind.h thermal_check) -----------------------------------
static int check_thermal_call(const slf_module* m, const char* what, const slf_thermal_params* params, const void* map,
                              const void* const* ptrs, const char* const* names, int n_ptrs, const void* src, const void* dst) {
  if (!m) return fail(SLF_ERR_INVALID, "module is NULL");
  std::string why;
  if (int rc = slf::thermal_check(*m, m->accf != nullptr, what, params, map, ptrs, names, n_ptrs, src, dst, &why))
    return fail(rc, why);
  return SLF_OK;
}

static slf::ThermalConstants thermal_constants(const slf_thermal_params* p) {
  slf::ThermalConstants k{};
  k.omega = p->omega_T, k.t_ref = p->T_ref;
  for (int d = 0; d < 3; d++) k.b[d] = p->b[d], k.periodic[d] = p->periodic[d] != 0;
  return k;
}

int slf_thermal_init(slf_module* m, const slf_thermal_params* params, const void* map, const void* T, const void* vx,
                     const void* vy, const void* vz, void* g0, slf_stream* stream) {
  const void* ptrs[] = {T, vx, vy, g0, vz};
  const char* names[] = {"T", "vx", "vy", "g0", "vz"};
  if (int e = check_thermal_call(m, "slf_thermal_init", params, map, ptrs, names, m && m->geo.dim == 3 ? 5 : 4, nullptr, nullptr))
    return e;
  SLF_HIP(hipSetDevice(m->ctx->device));
  const void* v[3] = {vx, vy, vz};
  SLF_HIP(slf::launch_thermal_init(m->sel, m->geo, thermal_constants(params), map, T, v, g0, m->accf, native(stream)));
  return SLF_OK;
}

int slf_thermal_step(slf_module* m, const slf_thermal_params* params, const void* map, const void* g_src, void* g_dst,
                     const void* vx, const void* vy, const void* vz, const void* wall_temperature, void* T,
                     slf_stream* stream) {
  const void* ptrs[] = {g_src, g_dst, vx, vy, wall_temperature, T, vz};
  const char* names[] = {"g_src", "g_dst", "vx", "vy", "wall_temperature", "T", "vz"};
  if (int e = check_thermal_call(m, "slf_thermal_step", params, map, ptrs, names, m && m->geo.dim == 3 ? 7 : 6, g_src, g_dst))
    return e;
  SLF_HIP(hipSetDevice(m->ctx->device));
  const void* v[3] = {vx, vy, vz};
  SLF_HIP(slf::launch_thermal_step(m->sel, m->geo, thermal_constants(params), map, g_src, g_dst, v, wall_temperature, T, m->accf,
                                   native(stream)));
  return SLF_OK;
}

int slf_kernel_get(slf_module* m, const char* name, slf_kernel** out) {
  if (!m || !name || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  const slf::KernelRow* row = nullptr;
  std::string why;
  if (int rc = slf::resolve(*m, name, &row, &why)) return fail(rc, why);
  slf_kernel* k = new slf_kernel();
  k->mod = m;
  k->row = row;
  k->kind = row->kind;
  *out = k;
  return SLF_OK;
}

int slf_kernel_destroy(slf_kernel* k) {
  delete k;
  return SLF_OK;
}

int slf_kernel_set_args(slf_kernel* k, const char* fmt, const void* const* argv, int argc, int needs_iteration) {
  if (!k || !fmt || (!argv && argc > 0)) return fail(SLF_ERR_INVALID, "NULL argument");
  slf::BoundArgs b;
  std::string why;
  if (int rc = slf::bind(*k->mod, *k->row, fmt, argv, argc, &b, &why)) return fail(rc, why);
  if (k->kind == slf::KK_RESIDENT) {
    if (int rc = slf::resident_check(*k->mod, b, needs_iteration, &why)) return fail(rc, why);
  }
  k->args = b;
  k->pair = {};     // new arguments: slf_kernel_set_pair has to look at them again
  k->needs_iteration = needs_iteration;
  k->bound = true;
  if (b.build_slots) {
    // indirect addressing: the sweep is launched over the slots (slot_sweep_kernel); the slot -> node table of this
    // `nodes` argument is built here, once (a launch may be recorded into a graph, where nothing can be allocated)
    SLF_HIP(hipSetDevice(k->mod->ctx->device));
    slot_table_for(k->mod, b.sweep.nodes, (hipStream_t)0);
  }
  return SLF_OK;
}

int slf_kernel_set_iteration(slf_kernel* k, uint32_t iteration) {
  if (!k) return fail(SLF_ERR_INVALID, "kernel is NULL");
  k->iteration = iteration;
  return SLF_OK;
}

namespace {

// The launch arguments of a kernel: the bound ones, then the module state that may have changed since (the one place that
// copies it).  The single-fluid sweeps take the x-face buffers, the row classes, the field and the slot table (built when
// the arguments were bound, slf_kernel_set_args: a launch may be part of a graph capture); the Shan-Chen kinds the planes.
slf::SweepArgs launch_args(const slf_kernel* k) {
  const slf_module* m = k->mod;
  slf::SweepArgs a = k->args.sweep;
  a.node_params = m->node_params;
  a.status = m->status;
  if (k->kind == slf::KK_COLLIDE_AND_PROPAGATE || k->kind == slf::KK_COMPUTE_MACRO) {
    for (int f = 0; f < 2; f++) {
      a.xsend[f] = m->xsend[f];
      a.xrecv[f] = m->xrecv[f];
    }
    a.rows = m->rows.map ? &m->rows : nullptr;
    if (k->kind == slf::KK_COLLIDE_AND_PROPAGATE) {
      if (m->phys.accel_field) a.accf = m->accf;
      if (m->geo.indirect && m->slots.nodes == a.nodes) a.slots = &m->slots;
    }
  } else if (m->sc.enabled) {
    sc_planes_of(m, a);
  }
  return a;
}

// what a pair sweep (slf_kernel_set_pair) reads of them
slf::SweepArgs pair_args(const slf::SweepArgs& a) {
  slf::SweepArgs p = {};
  p.nodes = a.nodes;
  p.map = a.map;
  p.dist_in = a.dist_in;
  p.dist_out = a.dist_out;
  p.node_params = a.node_params;
  p.status = a.status;
  p.options = a.options;
  for (int f = 0; f < 2; f++) {
    p.xsend[f] = a.xsend[f];
    p.xrecv[f] = a.xrecv[f];
  }
  return p;
}

}  // namespace

int slf_kernel_set_pair(slf_kernel* k, int rows_per_strip, int planes_per_chunk) {
  if (!k) return fail(SLF_ERR_INVALID, "kernel is NULL");
  if (k->kind != slf::KK_COLLIDE_AND_PROPAGATE)
    return fail(SLF_ERR_UNSUPPORTED, "pair sweep: CollideAndPropagate kernels of single-fluid modules only");
  if (!k->bound) return fail(SLF_ERR_INVALID, "pair sweep: set the kernel arguments first (source and destination are checked)");
  if (rows_per_strip < 0 || planes_per_chunk < 0) return fail(SLF_ERR_INVALID, "pair sweep: negative strip / chunk size");
  const slf_module* m = k->mod;
  if (on_lat(m)) return fail(SLF_ERR_UNSUPPORTED, std::string("pair sweep: not implemented on ") + lat_name(m) + " (D3Q19, single precision, BGK modules only)");
  // The knobs of the kernel, read here, per kernel object (unset or empty: the default; not a small non-negative integer:
  // -1, which pair_refusal names).  SLF_PAIR_PREFETCH: the load path of phase A (0: synchronous); SLF_PAIR_XCD_LOG2:
  // neighbouring strips on one XCD, at most 1 << this each (0: off); SLF_PAIR_MARCH: 1 = odd strips walk downwards
  auto knob = [](const char* name, int dflt) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    return (end && !*end && v >= 0 && v < 1000) ? (int)v : -1;
  };
  const slf::PairKnobs knobs = {rows_per_strip ? rows_per_strip : slf::pair_default_rows(m->geo),
                                planes_per_chunk ? planes_per_chunk : slf::pair_default_zchunk(m->geo),
                                knob("SLF_PAIR_PREFETCH", slf::pair_default_prefetch()),
                                knob("SLF_PAIR_XCD_LOG2", slf::pair_default_xcd_log2()), knob("SLF_PAIR_MARCH", slf::pair_default_march())};
  if (m->sc.enabled || m->fe.enabled || m->sc3.enabled || m->sel.lattice != SLF_D3Q19 || k->args.alpha_arg)
    return fail(SLF_ERR_UNSUPPORTED, "pair sweep: D3Q19, single precision, BGK modules only");
  if (const char* why = slf::pair_refusal(m->sel, m->access_pattern == SLF_AB, m->geo, m->phys, pair_args(launch_args(k)), knobs))
    return fail(SLF_ERR_UNSUPPORTED, why);
  k->pair = knobs;
  return SLF_OK;
}

int slf_kernel_launch(slf_kernel* k, const slf_region* region, slf_stream* stream) {
  if (!k) return fail(SLF_ERR_INVALID, "kernel is NULL");
  if (!k->bound) return fail(SLF_ERR_INVALID, "kernel arguments not set");
  slf_module* m = k->mod;
  const slf::Geometry& g = m->geo;
  const slf::KernelKind kk = k->kind;
  const slf::BoundArgs& b = k->args;
  SLF_HIP(hipSetDevice(m->ctx->device));   // several contexts may live in one process (one per GPU): launch on ours
  hipStream_t s = native(stream);
  hipError_t e = hipSuccess;
  // what may be launched, where and with which propagation step: slf_bind.h part (f)
  slf::LaunchShape sh;
  slf::FaceBox box;
  std::string why;
  const slf::LaunchState state = {k->needs_iteration, k->iteration, m->accf != nullptr, k->pair.rows != 0};
  if (int rc = slf::launch_check(*m, *k->row, b, state, region, &sh, &box, &why)) return fail(rc, why);
  const slf::SweepArgs a = launch_args(k);
  const slf::Launch lc = {m->sel, sh.prop, g, m->phys, sh.y0, sh.y1, sh.z0, sh.z1, m->block_x, s};
  if (k->pair.rows) {
    // two steps per launch: whatever has changed since slf_kernel_set_pair accepted (a body force, face buffers)
    // is an error here, never a quiet single step
    const slf::SweepArgs pa = pair_args(a);
    if (!slf::launch_sweep_pair(m->sel, m->access_pattern == SLF_AB, g, m->phys, pa, k->pair, s, &e)) {
      const char* refusal = slf::pair_refusal(m->sel, m->access_pattern == SLF_AB, g, m->phys, pa, k->pair);
      return fail(SLF_ERR_UNSUPPORTED, refusal ? refusal : "pair sweep: no kernel for this strip size");
    }
  } else switch (kk) {
    case slf::KK_COLLIDE_AND_PROPAGATE: e = on_lat(m) ? slf::launch_lat_sweep(lc, a) : slf::launch_sweep(lc, a); break;
    case slf::KK_COMPUTE_MACRO: e = on_lat(m) ? slf::launch_lat_macro(lc, a) : slf::launch_macro(lc, a); break;
    case slf::KK_SC_MACRO: e = slf::launch_sc_macro(lc, m->sc, a); break;
    case slf::KK_SC_SWEEP0:
    case slf::KK_SC_SWEEP1: e = slf::launch_sc_sweep(lc, m->sc, a, kk == slf::KK_SC_SWEEP0 ? 0 : 1); break;
    case slf::KK_SC_FUSED: e = slf::launch_sc_fused(lc, m->sc, a); break;
    case slf::KK_SCS_MACRO: e = slf::launch_scs_macro(lc, m->sc, a); break;
    case slf::KK_SCS_SWEEP: e = slf::launch_scs_sweep(lc, m->sc, a); break;
    case slf::KK_FE_MACRO: e = slf::launch_fe_macro(lc, m->fe, a); break;
    case slf::KK_FE_FLUID:
    case slf::KK_FE_ORDER: e = slf::launch_fe_sweep(lc, m->fe, a, kk == slf::KK_FE_FLUID ? 0 : 1); break;
    case slf::KK_SC3_MACRO:
    case slf::KK_SC3_SWEEP0:
    case slf::KK_SC3_SWEEP1:
    case slf::KK_SC3_SWEEP2:
    case slf::KK_SC3_FUSED: {
      slf::Sc3Args a3 = b.sc3;
      if (!m->sel.general) a3.map = nullptr;
      if (kk == slf::KK_SC3_MACRO) e = slf::launch_sc3_macro(lc, m->sc3, a3);
      else if (kk == slf::KK_SC3_FUSED) e = slf::launch_sc3_fused(lc, m->sc3, a3);
      else e = slf::launch_sc3_sweep(lc, m->sc3, a3, (int)kk - (int)slf::KK_SC3_SWEEP0);
      break;
    }
    case slf::KK_RESIDENT: {
      // dist_in / dist_in2: source a / b, dist_out / dist_out2: destination a / b; the kernel's SweepArgs carry the map only
      const void* src[2] = {a.dist_in, a.dist_in2};
      void* dst[2] = {a.dist_out, a.dist_out2};
      slf::SweepArgs r = {};
      r.map = a.map;
      r.options = a.options & ~1u;       // no field output from inside a stretch of resident steps
      r.node_params = a.node_params;
      r.status = a.status;
      e = slf::launch_resident(m->sel, m->access_pattern == SLF_AA, g, m->phys, r, src, dst, (int)k->iteration, (int)b.ints[1],
                               (int)b.ints[2], (int)b.ints[3], (int)b.ints[4], s);
      break;
    }
    // the initial conditions: (dist.., v.., rho[, phi[, theta]]) in the order of the reference (lb_single.py:72-94,
    // lb_binary.py:107-127, lb_ternary.py:118-142)
    case slf::KK_SET_INITIAL_CONDITIONS:
      if (on_lat(m)) e = slf::launch_lat_init(m->sel, g, m->phys, a.dist_in, a.rho, a.v, s);
      else e = slf::launch_init(m->sel, g, m->phys, a.dist_in, a.rho, a.v, a.nodes, s);
      break;
    case slf::KK_SC_INIT:
      e = slf::launch_sc_init(m->sel, g, m->phys, a.dist_in, a.dist_in2, a.rho, a.phi, a.v, a.nodes, s);
      break;
    case slf::KK_FE_INIT:
      e = slf::launch_fe_init(m->sel, g, m->fe, a.dist_in, a.dist_in2, a.rho, a.phi, a.v, m->sel.general ? a.map : nullptr, s);
      break;
    case slf::KK_SC3_INIT:
      e = slf::launch_sc3_init(m->sel, g, b.sc3.dist_in, b.sc3.field, b.sc3.v, s);
      break;
    case slf::KK_PBC:
    case slf::KK_PBC_SWAP:
      if (on_lat(m)) e = slf::launch_lat_pbc(m->sel, g, (void*)b.ptrs[0], (int)b.ints[0], kk == slf::KK_PBC_SWAP, s);
      else e = slf::launch_pbc(m->sel, g, (void*)b.ptrs[0], (int)b.ints[0], kk == slf::KK_PBC_SWAP, s);
      break;
    case slf::KK_MACRO_PBC:
      e = slf::launch_macro_pbc(m->sel, g, (void*)b.ptrs[0], (int)b.ints[0], s);
      break;
    case slf::KK_COLLECT_BOX:
    case slf::KK_DISTRIBUTE_BOX:
    case slf::KK_COLLECT_FACE_SWAP:
    case slf::KK_DISTRIBUTE_FACE_SWAP:
    case slf::KK_COLLECT_MACRO_FACE:
    case slf::KK_DISTRIBUTE_MACRO_FACE: {      // `box`: the direction mask and the box, or the reference's face (launch_check)
      slf::Geometry gm = g;
      if (box.macro) gm.dist_size = 0;
      e = slf::launch_box(m->sel, gm, box.collect, (void*)b.ptrs[0], (void*)b.ptrs[1], box.dirs, box.nd, box.base, box.col_stride,
                          box.ncols, box.row_stride, box.nrows, box.buf_k_stride, box.buf_row_stride, box.macro, s);
      break;
    }
    case slf::KK_COLLECT_SPARSE:
    case slf::KK_DISTRIBUTE_SPARSE:
      e = slf::launch_sparse(m->sel, kk == slf::KK_COLLECT_SPARSE, (const unsigned long long*)b.ptrs[0],
                             (void*)b.ptrs[1], (void*)b.ptrs[2], (int)b.ints[0], s);
      break;
  }
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  return SLF_OK;
}

// ---- step plans: the launch list of one time step, built once, enqueued with ONE call ----------------------------
// (include/sailfish_hip.h "step plans".)  Every entry is what the corresponding slf_* call would do; slf_plan_run()
// walks the list on the calling thread -- no Python, no argument marshalling between the entries.
namespace {
enum PlanKind { PL_LAUNCH, PL_RECORD, PL_WAIT, PL_EXCHANGE, PL_MEMSET, PL_COPY, PL_XFACE, PL_PEER_SIGNAL, PL_PEER_WAIT };
struct PlanOp {
  PlanKind kind;
  slf_kernel* k = nullptr;
  bool has_region = false;
  slf_region region = {0, 0, 0, 0};
  slf_stream* stream = nullptr;
  slf_event* ev = nullptr;
  slf_comm* comm = nullptr;
  std::vector<slf_comm_op> ops;
  void* dst = nullptr;
  const void* src = nullptr;
  int value = 0;             // PL_MEMSET: the byte
  size_t bytes = 0;
  slf_module* mod = nullptr;
  int xface_set = -1;        // PL_XFACE: -1 the single-fluid buffers, 0 .. 2 that set of planes
  void* xf[4] = {nullptr, nullptr, nullptr, nullptr};
  slf_peer* peer = nullptr;
  std::vector<int32_t> ranks;
  int channel = 0;
  int count = 0;             // PL_PEER_WAIT: the signals to wait for
};
}  // namespace

struct slf_plan {
  slf_ctx* ctx;
  std::vector<PlanOp> ops;
};

int slf_plan_create(slf_ctx* ctx, slf_plan** out) {
  if (!ctx || !out) return fail(SLF_ERR_INVALID, "NULL argument");
  slf_plan* p = new slf_plan;
  p->ctx = ctx;
  *out = p;
  return SLF_OK;
}

int slf_plan_destroy(slf_plan* p) {
  delete p;
  return SLF_OK;
}

int slf_plan_size(slf_plan* p, int* n_ops) {
  if (!p || !n_ops) return fail(SLF_ERR_INVALID, "NULL argument");
  *n_ops = (int)p->ops.size();
  return SLF_OK;
}

int slf_plan_add_launch(slf_plan* p, slf_kernel* k, const slf_region* region, slf_stream* stream) {
  if (!p || !k) return fail(SLF_ERR_INVALID, "NULL argument");
  if (!k->bound) return fail(SLF_ERR_INVALID, "kernel arguments not set");
  PlanOp o;
  o.kind = PL_LAUNCH;
  o.k = k;
  o.has_region = region != nullptr;
  if (region) o.region = *region;
  o.stream = stream;
  p->ops.push_back(o);
  return SLF_OK;
}

int slf_plan_add_record(slf_plan* p, slf_event* ev, slf_stream* stream) {
  if (!p || !ev) return fail(SLF_ERR_INVALID, "NULL argument");
  PlanOp o;
  o.kind = PL_RECORD;
  o.ev = ev;
  o.stream = stream;
  p->ops.push_back(o);
  return SLF_OK;
}

int slf_plan_add_wait(slf_plan* p, slf_stream* stream, slf_event* ev) {
  if (!p || !ev) return fail(SLF_ERR_INVALID, "NULL argument");
  PlanOp o;
  o.kind = PL_WAIT;
  o.ev = ev;
  o.stream = stream;
  p->ops.push_back(o);
  return SLF_OK;
}

int slf_plan_add_exchange(slf_plan* p, slf_comm* comm, const slf_comm_op* ops, int n, slf_stream* stream) {
  if (!p || !comm || (!ops && n > 0)) return fail(SLF_ERR_INVALID, "NULL argument");
  for (int i = 0; i < n; i++) {
    if (ops[i].elem_bytes != 4 && ops[i].elem_bytes != 8 && ops[i].elem_bytes != 1)
      return fail(SLF_ERR_INVALID, "elem_bytes must be 1, 4 or 8");
    if (ops[i].kind != SLF_COMM_SEND && ops[i].kind != SLF_COMM_RECV) return fail(SLF_ERR_INVALID, "bad slf_comm_op kind");
  }
  PlanOp o;
  o.kind = PL_EXCHANGE;
  o.comm = comm;
  o.ops.assign(ops, ops + (n > 0 ? n : 0));
  o.stream = stream;
  p->ops.push_back(o);
  return SLF_OK;
}

int slf_plan_add_memset(slf_plan* p, void* dptr, int value, size_t bytes, slf_stream* stream) {
  if (!p || !dptr) return fail(SLF_ERR_INVALID, "NULL argument");
  if (!stream) return fail(SLF_ERR_INVALID, "plan entries are asynchronous: a stream is needed");
  PlanOp o;
  o.kind = PL_MEMSET;
  o.dst = dptr;
  o.value = value;
  o.bytes = bytes;
  o.stream = stream;
  p->ops.push_back(o);
  return SLF_OK;
}

int slf_plan_add_copy(slf_plan* p, void* dst, const void* src, size_t bytes, slf_stream* stream) {
  if (!p || !dst || !src) return fail(SLF_ERR_INVALID, "NULL argument");
  if (!stream) return fail(SLF_ERR_INVALID, "plan entries are asynchronous: a stream is needed");
  PlanOp o;
  o.kind = PL_COPY;
  o.dst = dst;
  o.src = src;
  o.bytes = bytes;
  o.stream = stream;
  p->ops.push_back(o);
  return SLF_OK;
}

// planes: set `which` of them, else the buffers.  Validated now, with the module's rules, so that slf_plan_run cannot fail on it
static int plan_add_xface(slf_plan* p, slf_module* m, bool planes, int32_t which, void* send_low, void* send_high, void* recv_low,
                          void* recv_high) {
  if (!p || !m) return fail(SLF_ERR_INVALID, "NULL argument");
  PlanOp o;
  o.kind = PL_XFACE;
  o.mod = m;
  o.xface_set = planes ? which : -1;
  o.xf[0] = send_low; o.xf[1] = send_high; o.xf[2] = recv_low; o.xf[3] = recv_high;
  std::string why;
  if (int rc = planes ? slf::xface_planes_check(m, which, o.xf, &why) : slf::xface_buffers_check(m, o.xf, &why)) return fail(rc, why);
  p->ops.push_back(o);
  return SLF_OK;
}

int slf_plan_add_xface_buffers(slf_plan* p, slf_module* m, void* send_low, void* send_high, void* recv_low, void* recv_high) {
  return plan_add_xface(p, m, false, 0, send_low, send_high, recv_low, recv_high);
}

int slf_plan_add_xface_planes(slf_plan* p, slf_module* m, int32_t which, void* send_low, void* send_high, void* recv_low,
                              void* recv_high) {
  return plan_add_xface(p, m, true, which, send_low, send_high, recv_low, recv_high);
}

static int plan_add_peer(slf_plan* p, PlanKind kind, slf_peer* peer, const int32_t* ranks, int n, int channel, int count,
                         slf_stream* stream) {
  if (!p) return fail(SLF_ERR_INVALID, "NULL argument");
  if (count < 1) return fail(SLF_ERR_INVALID, "peer wait: count must be at least 1");
  // validated now, with the transport's rules, so that slf_plan_run cannot fail on it
  if (int e = peer_check_ranks(peer, ranks, n, channel)) return e;
  if (!stream) return fail(SLF_ERR_INVALID, "plan entries are asynchronous: a stream is needed");
  PlanOp o;
  o.kind = kind;
  o.peer = peer;
  o.ranks.assign(ranks, ranks + n);
  o.channel = channel;
  o.count = count;
  o.stream = stream;
  p->ops.push_back(o);
  return SLF_OK;
}

int slf_plan_add_peer_signal(slf_plan* p, slf_peer* peer, const int32_t* ranks, int n, int channel, slf_stream* stream) {
  return plan_add_peer(p, PL_PEER_SIGNAL, peer, ranks, n, channel, 1, stream);
}

int slf_plan_add_peer_wait(slf_plan* p, slf_peer* peer, const int32_t* ranks, int n, int channel, int count, slf_stream* stream) {
  return plan_add_peer(p, PL_PEER_WAIT, peer, ranks, n, channel, count, stream);
}

int slf_plan_run(slf_plan* p, uint32_t iteration) {
  if (!p) return fail(SLF_ERR_INVALID, "plan is NULL");
  for (PlanOp& o : p->ops) {
    int e = SLF_OK;
    switch (o.kind) {
      case PL_LAUNCH:
        if (o.k->needs_iteration) o.k->iteration = iteration;
        e = slf_kernel_launch(o.k, o.has_region ? &o.region : nullptr, o.stream);
        break;
      case PL_RECORD: e = slf_event_record(o.ev, o.stream); break;
      case PL_WAIT: e = slf_stream_wait_event(o.stream, o.ev); break;
      case PL_EXCHANGE: e = slf_comm_exchange(o.comm, o.ops.data(), (int)o.ops.size(), o.stream); break;
      case PL_MEMSET: e = slf_memset(p->ctx, o.dst, o.value, o.bytes, o.stream); break;
      case PL_COPY: e = slf_memcpy_d2d_async(p->ctx, o.dst, o.src, o.bytes, o.stream); break;
      case PL_XFACE: store_xface(o.mod, o.xface_set, o.xf); break;
      case PL_PEER_SIGNAL: e = slf_peer_signal(o.peer, o.ranks.data(), (int)o.ranks.size(), o.channel, o.stream); break;
      case PL_PEER_WAIT: e = slf_peer_wait(o.peer, o.ranks.data(), (int)o.ranks.size(), o.channel, o.count, o.stream); break;
    }
    if (e) return e;
  }
  return SLF_OK;
}

}  // extern "C"
