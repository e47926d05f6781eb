// fbk_group_api.inc — several GPUs behind ONE process (included by fbk.hip).
//
// The reference maps per-shard functions on the node that owns each shard and folds the
// count-valued results with an associative reduceFn IN THE SAME PROCESS (mapReduce / mapperLocal,
// executor.go:6449-6533, 6742-6790; reduceFn of executeCount :5880, mergeGroupCounts :3728).  A Go
// server is one process that owns all GPUs of the node, so the equivalent here is a *group*: one
// context per device, shard s living on member s mod G, every member's kernels enqueued on its own
// stream (nothing serialises the devices against each other), and the partial counts reduced by
//   FBK_REDUCE_HOST  G small device->pinned-host copies and an add on the host
//   FBK_REDUCE_PEER  one kernel on member 0 that loads the partials of the other devices through
//                    peer access (xGMI loads) and adds them
//   FBK_REDUCE_RCCL  ncclAllReduce over single-process communicators (ncclCommInitAll), the same
//                    collective the one-process-per-GPU deployment (featurebase_amd/dist.py) uses.
//                    librccl is dlopen'ed on first use: libfbk.so itself links only the HIP runtime.
// Bitmap-valued results are never exchanged (they stay per shard, executor.go:1767).
// The same device ordinal may appear more than once in a group (members then share the device):
// that is how the complete G > 1 code path is exercised on a one-GPU box; RCCL refuses such a
// group, the other two reduce modes do not care.

#include <dlfcn.h>

namespace fbk {

constexpr int kMaxGroup = 32;
struct PeerPtrs {
  const u64* p[kMaxGroup];
};

// total[c] = sum over members of partial_m[c]; member 0's device reads the other devices' memory
__global__ void __launch_bounds__(256) k_sum_peers(PeerPtrs src, uint32_t n, uint64_t words, u64* __restrict__ total) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= words) return;
  u64 acc = 0;
  for (uint32_t m = 0; m < n; ++m) acc += __builtin_nontemporal_load(&src.p[m][c]);
  total[c] = acc;
}

// dst[k] = src[ids[k]]: a member's totals of the merged candidate rows (second pass of a group TopN)
__global__ void __launch_bounds__(256) k_gather_u64(const u64* __restrict__ src, const uint32_t* __restrict__ ids, uint64_t n, u64* __restrict__ dst) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) dst[k] = src[ids[k]];
}

}  // namespace fbk

// the few RCCL entry points the group needs (types as in <rccl/rccl.h>: ncclComm_t is an opaque
// pointer, ncclResult_t / ncclDataType_t / ncclRedOp_t are ints: ncclSuccess 0, ncclUint64 5, ncclSum 0)
struct NcclId {  // ncclUniqueId: 128 opaque bytes, passed BY VALUE to ncclCommInitRank
  char internal[128];
};
struct FbkRccl {
  void* handle = nullptr;
  int (*GetUniqueId)(NcclId* id) = nullptr;
  int (*CommInitRank)(void** comm, int nranks, NcclId id, int rank) = nullptr;
  int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
  int (*CommDestroy)(void* comm) = nullptr;
  int (*AllReduce)(const void* send, void* recv, size_t count, int dtype, int op, void* comm, hipStream_t stream) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};

struct fbk_group {
  std::vector<fbk_ctx*> members;
  std::vector<int> devices;
  std::mutex mu;  // one group operation at a time
  int reduce_mode = FBK_REDUCE_HOST;
  // per member: a device vector for its partial counts (grown on demand) and an event that marks
  // "partial of the current operation produced"
  std::vector<u64*> d_partial;
  std::vector<uint64_t> partial_cap;  // in uint64 words
  std::vector<hipEvent_t> ev;
  u64* d_total0 = nullptr;  // on member 0: result of the peer reduce
  uint64_t total0_cap = 0;
  u64* h_partial = nullptr;  // pinned: members x words
  uint64_t h_cap = 0;
  bool peer_checked = false, peer_ok = false;
  FbkRccl rccl;
  std::vector<void*> comms;
  // last failing fbk_group_* call (fbk_group_last_error_r): group-level failures — argument checks, "plan was
  // not created on member", peer / RCCL set-up, the reserve — have no member context to be recorded on
  std::mutex err_mu;
  std::string err_msg;
  int32_t err_code = 0;
};

namespace {

void group_record_error(fbk_group* g, int32_t code, const std::string& msg) {
  std::lock_guard<std::mutex> lk(g->err_mu);
  g->err_msg = msg;
  g->err_code = code;
}

// first statement of every fbk_group_* entry point: failures of the call are recorded on the group
struct GroupScope {
  fbk_group* prev;
  explicit GroupScope(fbk_group* g) : prev(g_scope_group) { g_scope_group = g; }
  ~GroupScope() { g_scope_group = prev; }
};

// the group functions' closing handler (see FBK_ABI_CATCH in fbk.hip): the message is recorded for the group
#define FBK_ABI_CATCH_GROUP(g)                                                               \
  catch (const std::bad_alloc&) {                                                            \
    GroupScope gs_(g);                                                                       \
    return fail(FBK_E_NOMEM, std::string(__func__) + ": host allocation failed");            \
  }                                                                                          \
  catch (const std::exception& e_) {                                                         \
    GroupScope gs_(g);                                                                       \
    return fail(FBK_E_HIP, std::string(__func__) + ": " + e_.what());                        \
  }                                                                                          \
  catch (...) {                                                                              \
    GroupScope gs_(g);                                                                       \
    return fail(FBK_E_HIP, std::string(__func__) + ": unknown exception");                   \
  }

// Every member's context lock, taken in member order and HELD until the group operation has synchronised
// the member streams.  The enqueue helpers stage row indexes in the member's pinned h_stage and rely on
// "each call that uses it synchronises the stream before returning" (fbk.hip): another thread calling on a
// member context between a group call's enqueue and its reduce would reset h_stage_used and overwrite
// staging whose H2D copy is still in flight.  (The group lock comes first, so the order is fixed.)
struct MemberLocks {
  std::vector<std::unique_lock<std::mutex>> held;
  explicit MemberLocks(fbk_group* g) {
    held.reserve(g->members.size());
    for (fbk_ctx* c : g->members) held.emplace_back(c->mu);
  }
};

// after a failure in the middle of a group call: nothing a member has enqueued may still be running (or
// reading its staging) when the locks are released
void group_drain(fbk_group* g) {
  for (fbk_ctx* c : g->members) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
  }
  (void)hipGetLastError();
}

int32_t group_check(fbk_group* g) {
  if (!g) return fail(FBK_E_INVALID, "group is NULL");
  return FBK_OK;
}

// make room for `words` uint64 of partial counts on every member (and the host / member-0 side buffers)
int32_t group_reserve(fbk_group* g, uint64_t words) {
  const uint32_t n = uint32_t(g->members.size());
  for (uint32_t m = 0; m < n; ++m) {
    if (g->partial_cap[m] >= words) continue;
    fbk_ctx* c = g->members[m];
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (g->d_partial[m]) ctx_free(c, g->d_partial[m]);
    g->d_partial[m] = nullptr;
    g->partial_cap[m] = 0;
    HIP_TRY(ctx_malloc(c, reinterpret_cast<void**>(&g->d_partial[m]), words * 8));
    g->partial_cap[m] = words;
  }
  if (g->total0_cap < words) {
    fbk_ctx* c = g->members[0];
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (g->d_total0) ctx_free(c, g->d_total0);
    g->d_total0 = nullptr;
    g->total0_cap = 0;
    HIP_TRY(ctx_malloc(c, reinterpret_cast<void**>(&g->d_total0), words * 8));
    g->total0_cap = words;
  }
  if (g->h_cap < uint64_t(n) * words) {
    if (g->h_partial) (void)hipHostFree(g->h_partial);
    g->h_partial = nullptr;
    g->h_cap = 0;
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, uint64_t(n) * words * 8, hipHostMallocPortable));
    g->h_partial = static_cast<u64*>(p);
    g->h_cap = uint64_t(n) * words;
  }
  return FBK_OK;
}

int32_t group_enable_peer(fbk_group* g) {
  if (g->peer_checked) return g->peer_ok ? FBK_OK : fail(FBK_E_INVALID, "group: peer access between the devices is not available");
  g->peer_checked = true;
  const int d0 = g->devices[0];
  for (size_t m = 1; m < g->devices.size(); ++m) {
    const int dm = g->devices[m];
    if (dm == d0) continue;
    int can = 0;
    hipError_t e = hipDeviceCanAccessPeer(&can, d0, dm);
    if (e != hipSuccess || !can) {
      (void)hipGetLastError();
      return fail(FBK_E_INVALID, "group: device " + std::to_string(d0) + " cannot access device " + std::to_string(dm));
    }
    HIP_TRY(hipSetDevice(d0));
    e = hipDeviceEnablePeerAccess(dm, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
      (void)hipGetLastError();
      return fail(FBK_E_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
    }
    (void)hipGetLastError();
  }
  g->peer_ok = true;
  return FBK_OK;
}

FbkRccl g_rccl;  // the process's copy for the fbk_comm_* calls (a group keeps its own)
std::mutex g_rccl_mu;

// librccl, dlopen'ed on first use (libfbk.so itself links only the HIP runtime)
int32_t rccl_load(FbkRccl& r) {
  if (r.handle) return FBK_OK;
  // a process that already carries an RCCL (PyTorch bundles one next to its HIP runtime) must
  // use THAT one: ask for the loaded copy first
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
  for (const char* nm : names)
    if ((r.handle = dlopen(nm, RTLD_NOW | RTLD_NOLOAD))) break;
  for (size_t i = 0; !r.handle && i < 3; ++i) r.handle = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
  if (!r.handle) return fail(FBK_E_INVALID, std::string("librccl not found: ") + (dlerror() ? dlerror() : "?"));
  r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.handle, "ncclGetUniqueId"));
  r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.handle, "ncclCommInitRank"));
  r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(r.handle, "ncclCommInitAll"));
  r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.handle, "ncclCommDestroy"));
  r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.handle, "ncclAllReduce"));
  r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.handle, "ncclGroupStart"));
  r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.handle, "ncclGroupEnd"));
  r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.handle, "ncclGetErrorString"));
  if (!r.CommInitAll || !r.CommDestroy || !r.AllReduce || !r.GroupStart || !r.GroupEnd || !r.GetUniqueId || !r.CommInitRank) {
    r.handle = nullptr;
    return fail(FBK_E_INVALID, "librccl does not export the ncclCommInit* / ncclAllReduce family");
  }
  return FBK_OK;
}

int32_t group_init_rccl(fbk_group* g) {
  if (!g->comms.empty()) return FBK_OK;
  const uint32_t n = uint32_t(g->members.size());
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = i + 1; j < n; ++j)
      if (g->devices[i] == g->devices[j])
        return fail(FBK_E_INVALID, "group: FBK_REDUCE_RCCL needs distinct devices (device " + std::to_string(g->devices[i]) +
                                       " appears twice); use FBK_REDUCE_HOST or FBK_REDUCE_PEER");
  FbkRccl& r = g->rccl;
  if (int32_t rc = rccl_load(r)) return rc;
  g->comms.assign(n, nullptr);
  const int rc = r.CommInitAll(g->comms.data(), int(n), g->devices.data());
  if (rc != 0) {
    g->comms.clear();
    return fail(FBK_E_HIP, std::string("ncclCommInitAll: ") + (r.GetErrorString ? r.GetErrorString(rc) : std::to_string(rc)));
  }
  return FBK_OK;
}

// Every member has enqueued its partial (`words` uint64 at d_partial[m]) on its stream.  Reduce
// them into out_total (host).  mode: FBK_REDUCE_*.
int32_t group_reduce(fbk_group* g, uint64_t words, uint64_t* out_total) {
  const uint32_t n = uint32_t(g->members.size());
  switch (g->reduce_mode) {
    case FBK_REDUCE_HOST: {
      for (uint32_t m = 0; m < n; ++m) {
        fbk_ctx* c = g->members[m];
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpyAsync(g->h_partial + uint64_t(m) * words, g->d_partial[m], words * 8, hipMemcpyDeviceToHost, c->stream));
      }
      for (uint32_t m = 0; m < n; ++m) {
        HIP_TRY(hipSetDevice(g->members[m]->device));
        HIP_TRY(hipStreamSynchronize(g->members[m]->stream));
      }
      for (uint64_t c = 0; c < words; ++c) {
        u64 acc = 0;
        for (uint32_t m = 0; m < n; ++m) acc += g->h_partial[uint64_t(m) * words + c];
        out_total[c] = acc;
      }
      return FBK_OK;
    }
    case FBK_REDUCE_PEER: {
      if (int32_t rc = group_enable_peer(g)) return rc;
      fbk_ctx* c0 = g->members[0];
      fbk::PeerPtrs pp{};
      for (uint32_t m = 0; m < n; ++m) {
        pp.p[m] = g->d_partial[m];
        if (m == 0) continue;
        HIP_TRY(hipSetDevice(g->members[m]->device));
        HIP_TRY(hipEventRecord(g->ev[m], g->members[m]->stream));
      }
      HIP_TRY(hipSetDevice(c0->device));
      for (uint32_t m = 1; m < n; ++m) HIP_TRY(hipStreamWaitEvent(c0->stream, g->ev[m], 0));
      hipLaunchKernelGGL(fbk::k_sum_peers, dim3(uint32_t((words + 255) / 256)), dim3(256), 0, c0->stream, pp, n, words, g->d_total0);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(g->h_partial, g->d_total0, words * 8, hipMemcpyDeviceToHost, c0->stream));
      HIP_TRY(hipStreamSynchronize(c0->stream));
      std::memcpy(out_total, g->h_partial, words * 8);
      return FBK_OK;
    }
    case FBK_REDUCE_RCCL: {
      if (int32_t rc = group_init_rccl(g)) return rc;
      FbkRccl& r = g->rccl;
      int rc = r.GroupStart();
      for (uint32_t m = 0; m < n && rc == 0; ++m) {
        HIP_TRY(hipSetDevice(g->members[m]->device));
        rc = r.AllReduce(g->d_partial[m], g->d_partial[m], words, /*ncclUint64*/ 5, /*ncclSum*/ 0, g->comms[m], g->members[m]->stream);
      }
      const int rc2 = r.GroupEnd();
      if (rc == 0) rc = rc2;
      if (rc != 0) return fail(FBK_E_HIP, std::string("ncclAllReduce: ") + (r.GetErrorString ? r.GetErrorString(rc) : std::to_string(rc)));
      fbk_ctx* c0 = g->members[0];
      HIP_TRY(hipSetDevice(c0->device));
      HIP_TRY(hipMemcpyAsync(g->h_partial, g->d_partial[0], words * 8, hipMemcpyDeviceToHost, c0->stream));
      for (uint32_t m = 0; m < n; ++m) {  // every rank's collective must have finished before its buffer is reused
        HIP_TRY(hipSetDevice(g->members[m]->device));
        HIP_TRY(hipStreamSynchronize(g->members[m]->stream));
      }
      std::memcpy(out_total, g->h_partial, words * 8);
      return FBK_OK;
    }
    default:
      return fail(FBK_E_INVALID, "group: unknown reduce mode");
  }
}

}  // namespace

extern "C" {

int32_t fbk_group_open(const int32_t* devices, uint32_t n, uint32_t /*flags*/, fbk_group** out_group) try {
  if (!devices || !out_group || n == 0) return fail(FBK_E_INVALID, "NULL argument");
  *out_group = nullptr;
  if (n > uint32_t(fbk::kMaxGroup)) return fail(FBK_E_INVALID, "group: at most " + std::to_string(fbk::kMaxGroup) + " members");
  fbk_group* g = new (std::nothrow) fbk_group();
  if (!g) return fail(FBK_E_NOMEM, "host allocation failed");
  int32_t rc = FBK_OK;
  for (uint32_t m = 0; m < n && !rc; ++m) {
    fbk_ctx* c = nullptr;
    rc = open_on_device(devices[m], nullptr, &c);
    if (rc) break;
    g->members.push_back(c);
    g->devices.push_back(devices[m]);
    g->d_partial.push_back(nullptr);
    g->partial_cap.push_back(0);
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) rc = fail(FBK_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
    g->ev.push_back(ev);
  }
  if (!rc) rc = group_reserve(g, 1);
  if (rc) {
    const std::string msg = g_err;
    (void)fbk_group_close(g);
    return fail(rc, msg);
  }
  *out_group = g;
  return FBK_OK;
} FBK_ABI_CATCH(nullptr)

int32_t fbk_group_close(fbk_group* g) try {
  if (!g) return FBK_OK;
  for (void* c : g->comms)
    if (c && g->rccl.CommDestroy) (void)g->rccl.CommDestroy(c);
  for (size_t m = 0; m < g->members.size(); ++m) {
    fbk_ctx* c = g->members[m];
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (g->d_partial[m]) ctx_free(c, g->d_partial[m]);
    if (m == 0 && g->d_total0) ctx_free(c, g->d_total0);
    if (g->ev[m]) (void)hipEventDestroy(g->ev[m]);
  }
  if (g->h_partial) (void)hipHostFree(g->h_partial);
  for (fbk_ctx* c : g->members) (void)fbk_close(c);
  delete g;
  return FBK_OK;
} FBK_ABI_CATCH(nullptr)  // (the group may be gone: nothing is recorded on it)

int32_t fbk_group_size(const fbk_group* g, uint32_t* out_n) try {
  if (!g || !out_n) return fail(FBK_E_INVALID, "NULL argument");
  *out_n = uint32_t(g->members.size());
  return FBK_OK;
} FBK_ABI_CATCH_GROUP(const_cast<fbk_group*>(g))

int32_t fbk_group_member(fbk_group* g, uint32_t i, fbk_ctx** out_ctx) try {
  if (!g || !out_ctx) return fail(FBK_E_INVALID, "NULL argument");
  if (i >= g->members.size()) return fail(FBK_E_INVALID, "group: member index out of range");
  *out_ctx = g->members[i];
  return FBK_OK;
} FBK_ABI_CATCH_GROUP(g)

int32_t fbk_group_set_reduce(fbk_group* g, int32_t mode) try {
  if (int32_t rc = group_check(g)) return rc;
  GroupScope gs(g);
  if (mode < FBK_REDUCE_HOST || mode > FBK_REDUCE_RCCL) return fail(FBK_E_INVALID, "group: unknown reduce mode");
  std::lock_guard<std::mutex> lk(g->mu);
  if (mode == FBK_REDUCE_PEER)
    if (int32_t rc = group_enable_peer(g)) return rc;
  if (mode == FBK_REDUCE_RCCL)
    if (int32_t rc = group_init_rccl(g)) return rc;
  g->reduce_mode = mode;
  return FBK_OK;
} FBK_ABI_CATCH_GROUP(g)

// One step of Count(Intersect(Row, Row)) over the shards of ALL members: plans[m] (created on
// member m's context over the shards it owns, NULL = the member has none) is enqueued as ONE launch
// per device with the per-device sum fused (fbk_plan_intersection_count_total), all devices
// running concurrently; *out_total = the sum over the members (mapReduce + reduceFn of
// executeCount, executor.go:6449-6533, 5871-5880).
int32_t fbk_group_plan_intersection_count_total(fbk_group* g, fbk_plan* const* plans, uint64_t* out_total) try {
  if (int32_t rc = group_check(g)) return rc;
  GroupScope gs(g);
  if (!plans || !out_total) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t n = uint32_t(g->members.size());
  for (uint32_t m = 0; m < n; ++m)
    if (plans[m] && plans[m]->ctx != g->members[m]) return fail(FBK_E_INVALID, "group: plan " + std::to_string(m) + " was not created on member " + std::to_string(m));
  MemberLocks locks(g);
  int32_t rc = FBK_OK;
  for (uint32_t m = 0; m < n && !rc; ++m) {
    fbk_ctx* c = g->members[m];
    FBK_ENTER_QUIET(c);  // (the member's hot plan stays hot, as in fbk_plan_intersection_count_total)
    rc = set_device(c);
    if (rc) break;
    if (plans[m]) {
      rc = plan_icount_enqueue_locked(c, plans[m], g->d_partial[m]);
    } else {
      const hipError_t e = hipMemsetAsync(g->d_partial[m], 0, 8, c->stream);
      if (e != hipSuccess) rc = fail(FBK_E_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    }
  }
  if (!rc) rc = group_reduce(g, 1, out_total);
  if (rc) group_drain(g);
  return rc;
} FBK_ABI_CATCH_GROUP(g)

// GroupBy / TopN-style count matrix over the shards of all members: per_member[m] describes member
// m's local shards exactly as the arguments of fbk_count_matrix do; out_total[i * n_b + j] = the sum
// over every shard of every member (mergeGroupCounts / Pairs.Add across nodes, executor.go:3728,
// 2852).  Per-shard matrices stay on their device.
int32_t fbk_group_count_matrix(fbk_group* g, const fbk_matrix_args* per_member, uint32_t n_a, uint32_t n_b, uint64_t* out_total) try {
  if (int32_t rc = group_check(g)) return rc;
  GroupScope gs(g);
  if (!per_member || !out_total) return fail(FBK_E_INVALID, "NULL argument");
  const uint64_t width = uint64_t(n_a) * n_b;
  if (width == 0) return FBK_OK;
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t n = uint32_t(g->members.size());
  for (uint32_t m = 0; m < n; ++m) {
    const fbk_matrix_args& a = per_member[m];
    if (a.n_shards == 0) continue;
    if (int32_t rc = count_matrix_args_ok(a.a, a.rows_a, n_a, a.b, a.rows_b, n_b, a.filter, a.rows_f, a.n_shards)) return rc;
    if (a.a->ctx != g->members[m] || a.b->ctx != g->members[m] || (a.filter && a.filter->ctx != g->members[m]))
      return fail(FBK_E_INVALID, "group: the batches of member " + std::to_string(m) + " live on another context");
  }
  MemberLocks locks(g);
  int32_t rc = group_reserve(g, width);
  for (uint32_t m = 0; m < n && !rc; ++m) {
    fbk_ctx* c = g->members[m];
    const fbk_matrix_args& a = per_member[m];
    FBK_ENTER(c);
    rc = set_device(c);
    if (rc) break;
    if (a.n_shards == 0) {
      const hipError_t e = hipMemsetAsync(g->d_partial[m], 0, width * 8, c->stream);
      if (e != hipSuccess) rc = fail(FBK_E_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
      continue;
    }
    MatrixPlan p;
    rc = matrix_prepare(c, p, a.a, a.rows_a, n_a, a.b, a.rows_b, n_b, a.filter, a.rows_f, a.n_shards, false);
    if (!rc) rc = matrix_enqueue(c, p, g->d_partial[m], false);
    if (rc) group_drain(g);  // (before the plan's buffers go back to the member's pool)
  }
  if (!rc) rc = group_reduce(g, width, out_total);
  if (rc) group_drain(g);
  return rc;
} FBK_ABI_CATCH_GROUP(g)

// The reduce alone, for count-valued partials the caller produced itself with the member contexts
// (BSI sums, TopK counts, fold counts ...): device_partials[m] = `words` uint64 on member m's device,
// produced on member m's stream (or synchronised).
int32_t fbk_group_reduce_u64(fbk_group* g, void* const* device_partials, uint64_t words, uint64_t* out_total) try {
  if (int32_t rc = group_check(g)) return rc;
  GroupScope gs(g);
  if (!device_partials || !out_total) return fail(FBK_E_INVALID, "NULL argument");
  if (words == 0) return FBK_OK;
  std::lock_guard<std::mutex> lk(g->mu);
  MemberLocks locks(g);
  int32_t rc = group_reserve(g, words);
  for (uint32_t m = 0; m < g->members.size() && !rc; ++m) {
    fbk_ctx* c = g->members[m];
    FBK_ENTER(c);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess)
      e = device_partials[m] ? hipMemcpyAsync(g->d_partial[m], device_partials[m], words * 8, hipMemcpyDeviceToDevice, c->stream)
                             : hipMemsetAsync(g->d_partial[m], 0, words * 8, c->stream);
    if (e != hipSuccess) rc = fail(FBK_E_HIP, std::string("group partial copy: ") + hipGetErrorString(e));
  }
  if (!rc) rc = group_reduce(g, words, out_total);
  if (rc) group_drain(g);
  return rc;
} FBK_ABI_CATCH_GROUP(g)


// Sum(field = v) over the shards of all members: every member runs the BSI sum kernel over the shards it owns
// (executeSumCountShard, executor.go:2155; fragment.sum, fragment.go:724-750) and folds them on its device into
// {psum, nsum, count}; the three words are reduced over the members (ValCount.Add, executor.go:8438).
// *out_sum = int64(psum) - int64(nsum) with the reference's uint64 wrap-around (roaring/filter.go:1103-1108);
// the caller adds count * Base (executor.go:2205).
int32_t fbk_group_bsi_sum(fbk_group* g, const fbk_bsi_args* per_member, uint32_t bit_depth, int64_t* out_sum, uint64_t* out_count) try {
  if (int32_t rc = group_check(g)) return rc;
  GroupScope gs(g);
  if (!per_member || !out_sum || !out_count) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t n = uint32_t(g->members.size());
  for (uint32_t m = 0; m < n; ++m) {
    const fbk_bsi_args& a = per_member[m];
    if (a.n_shards == 0) continue;
    if (!a.batch || !a.base_rows || (a.filter && !a.rows_f)) return fail(FBK_E_INVALID, "group: NULL argument for member " + std::to_string(m));
    if (a.batch->ctx != g->members[m] || (a.filter && a.filter->ctx != g->members[m]))
      return fail(FBK_E_INVALID, "group: the batches of member " + std::to_string(m) + " live on another context");
    if (int32_t rc = bsi_rows_ok(a.base_rows, a.n_shards, bit_depth, a.batch->n_rows)) return rc;
  }
  MemberLocks locks(g);
  int32_t rc = group_reserve(g, 3);
  std::vector<DevBuf> dbase(n), drf(n), d3(n);  // alive until the reduce has synchronised the member streams
  for (uint32_t m = 0; m < n && !rc; ++m) {
    fbk_ctx* c = g->members[m];
    const fbk_bsi_args& a = per_member[m];
    FBK_ENTER(c);
    rc = set_device(c);
    if (rc) break;
    hipError_t e = hipMemsetAsync(g->d_partial[m], 0, 24, c->stream);
    if (e != hipSuccess) {
      rc = fail(FBK_E_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
      break;
    }
    if (a.n_shards == 0) continue;
    rc = upload_rows(c, a.base_rows, a.n_shards, a.batch->n_rows, dbase[m]);
    if (!rc && a.filter) rc = upload_rows(c, a.rows_f, a.n_shards, a.filter->n_rows, drf[m]);
    if (!rc && d3[m].alloc(c, uint64_t(a.n_shards) * 24) != hipSuccess) rc = fail(FBK_E_NOMEM, "group: device allocation failed");
    if (!rc) rc = bsi_sum_launch(c, a.batch, dbase[m].as<uint32_t>(), a.n_shards, bit_depth, a.filter, drf[m].as<uint32_t>(), d3[m].as<u64>());
    if (!rc) {
      // the member's shards folded on its device: {psum, nsum, count} (uint64 sums wrap exactly as the reference's)
      hipLaunchKernelGGL(fbk::k_reduce_shards, dim3(1, std::min<uint32_t>(a.n_shards, 64)), dim3(256), 0, c->stream, d3[m].as<u64>(), a.n_shards, uint64_t(3),
                         g->d_partial[m]);
      e = hipGetLastError();
      if (e != hipSuccess) rc = fail(FBK_E_HIP, std::string("k_reduce_shards: ") + hipGetErrorString(e));
    }
  }
  uint64_t tot[3] = {0, 0, 0};
  if (!rc) rc = group_reduce(g, 3, tot);
  if (rc) {
    group_drain(g);
    return rc;
  }
  *out_sum = int64_t(uint64_t(tot[0]) - uint64_t(tot[1]));
  *out_count = tot[2];
  return FBK_OK;
} FBK_ABI_CATCH_GROUP(g)

// TopN over the shards of all members (executeTopN, executor.go:2779-2864).  In the reference the first pass truncates per
// SHARD (fragment.top with N = n inside executeTopNShard :2869-2944); executeTopNShards merges all shards' pairs with
// Pairs.Add and never trims a node's answer, so which node owns which shard does not matter.  Here every member counts
// every row of its shards exactly and (option topn_semantics = 1) flags the rows that some shard of its own would have
// returned (k_topn_candidates); ONE reduce of [totals | candidate flags] (2 n_a words) over the members gives both the
// candidate set and the second pass's totals; non-candidates are dropped, the rest ordered and trimmed to n (:2823-2825).
// topn_semantics = 0 (or n = 0 / n >= n_a): the exact top n, one reduce of n_a words.  Either way the result does not
// depend on how the shards are dealt to the members.
int32_t fbk_group_topn(fbk_group* g, const fbk_topn_args* per_member, uint32_t n_a, uint32_t top_n, uint64_t min_threshold, uint64_t tanimoto_threshold,
                       uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n) try {
  if (int32_t rc = group_check(g)) return rc;
  GroupScope gs(g);
  if (!per_member || !out_n || (cap && (!out_index || !out_count))) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = topn_args_ok(n_a, tanimoto_threshold)) return rc;
  *out_n = 0;
  if (n_a == 0) return FBK_OK;
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t n = uint32_t(g->members.size());
  for (uint32_t m = 0; m < n; ++m) {
    const fbk_topn_args& a = per_member[m];
    if (a.n_shards == 0) continue;
    if (!a.a || !a.rows_a || (a.filter && !a.rows_f)) return fail(FBK_E_INVALID, "group: NULL argument for member " + std::to_string(m));
    if (a.a->ctx != g->members[m] || (a.filter && a.filter->ctx != g->members[m]))
      return fail(FBK_E_INVALID, "group: the batches of member " + std::to_string(m) + " live on another context");
  }
  MemberLocks locks(g);
  const uint32_t cand_n = topn_cand_n(g->members[0], top_n, n_a, true);
  for (uint32_t m = 1; m < n; ++m)  // one rule for the whole group: members that disagree would reduce vectors of different meaning
    if (topn_cand_n(g->members[m], top_n, n_a, true) != cand_n)
      return fail(FBK_E_INVALID, "group topn: member " + std::to_string(m) + " has another topn_semantics than member 0 (set the option on every member context)");
  const uint64_t words = uint64_t(n_a) * (cand_n ? 2 : 1);
  int32_t rc = group_reserve(g, words);
  // ---- every member enqueues its counts straight into its reduce buffer (the devices run concurrently)
  for (uint32_t m = 0; m < n && !rc; ++m) {
    fbk_ctx* c = g->members[m];
    const fbk_topn_args& a = per_member[m];
    FBK_ENTER(c);
    rc = set_device(c);
    if (rc) break;
    u64* part = static_cast<u64*>(g->d_partial[m]);
    if (a.n_shards == 0) {
      if (hipMemsetAsync(part, 0, words * 8, c->stream) != hipSuccess) rc = fail(FBK_E_HIP, "group topn: memset failed");
      continue;
    }
    TopnBuffers scratch;  // (totals and flags go to `part`; not masked: the flags of all members are reduced first)
    rc = topn_totals_locked(c, a.a, a.rows_a, n_a, a.filter, a.rows_f, a.n_shards, min_threshold, tanimoto_threshold, cand_n, scratch, /*mask=*/false, part, part + n_a);
  }
  std::vector<uint64_t> tot(words);
  if (!rc) rc = group_reduce(g, words, tot.data());
  if (rc) {
    group_drain(g);
    return rc;
  }
  // ---- candidates only, then order (Pairs.Less by count; ties by row index ascending, as fbk_topn), drop empty rows, trim to n
  return topn_order_host("topn", tot.data(), cand_n ? tot.data() + n_a : nullptr, n_a, top_n, out_index, out_count, cap, out_n);
} FBK_ABI_CATCH_GROUP(g)

/* Message and status code of the last failing fbk_group_* call on THIS group, copied into a caller buffer
 * (the cgo-safe form, like fbk_last_error_r for contexts: nothing thread-local). */
int32_t fbk_group_last_error_r(fbk_group* g, char* buf, uint64_t cap, int32_t* out_code) try {
  if (!g) return fail(FBK_E_INVALID, "group is NULL");
  std::string msg;
  int32_t code = 0;
  {
    std::lock_guard<std::mutex> lk(g->err_mu);
    msg = g->err_msg;
    code = g->err_code;
  }
  if (out_code) *out_code = code;
  if (buf && cap) {
    const uint64_t k = std::min<uint64_t>(cap - 1, msg.size());
    std::memcpy(buf, msg.data(), k);
    buf[k] = 0;
  }
  return FBK_OK;
} FBK_ABI_CATCH_GROUP(g)

// ---- one process per GPU: the context's own communicator (include/fbk.h, fbk_comm_*) ---------------------------------

int32_t fbk_comm_unique_id(uint8_t* out_id) try {
  if (!out_id) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (int32_t rc = rccl_load(g_rccl)) return rc;
  NcclId id;
  const int rc = g_rccl.GetUniqueId(&id);
  if (rc != 0) return fail(FBK_E_HIP, std::string("ncclGetUniqueId: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : std::to_string(rc)));
  static_assert(sizeof(NcclId) == FBK_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  std::memcpy(out_id, &id, sizeof(id));
  return FBK_OK;
} FBK_ABI_CATCH(nullptr)

int32_t fbk_comm_init(fbk_ctx* ctx, const uint8_t* id, int32_t n_ranks, int32_t rank) try {
  FBK_ENTER(ctx);
  if (!ctx || !id) return fail(FBK_E_INVALID, "NULL argument");
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(FBK_E_INVALID, "comm: rank out of range");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (ctx->comm) return fail(FBK_E_INVALID, "comm: the context already has a communicator (fbk_comm_close first)");
  if (int32_t rc = set_device(ctx)) return rc;
  {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (int32_t rc = rccl_load(g_rccl)) return rc;
  }
  NcclId nid;
  std::memcpy(&nid, id, sizeof(nid));
  void* comm = nullptr;
  const int rc = g_rccl.CommInitRank(&comm, n_ranks, nid, rank);
  if (rc != 0) return fail(FBK_E_HIP, std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : std::to_string(rc)));
  hipError_t e = hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->comm_ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->comm_ev_out, hipEventDisableTiming);
  ctx->comm = comm;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    comm_release(ctx);
    return fail(FBK_E_HIP, std::string("comm: ") + hipGetErrorString(e));
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_comm_all_reduce_u64(fbk_ctx* ctx, void* device_words, uint64_t n_words) try {
  FBK_ENTER_QUIET(ctx);
  if (!ctx || !device_words) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!ctx->comm) return fail(FBK_E_INVALID, "comm: the context has no communicator (fbk_comm_init)");
  if (int32_t rc = set_device(ctx)) return rc;
  if (n_words == 0) return FBK_OK;
  // after what the context's stream holds now, on the communicator's stream: the next queries' kernels overlap it
  HIP_TRY(hipEventRecord(ctx->comm_ev_in, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->comm_stream, ctx->comm_ev_in, 0));
  const int rc = g_rccl.AllReduce(device_words, device_words, n_words, /*ncclUint64*/ 5, /*ncclSum*/ 0, ctx->comm, ctx->comm_stream);
  if (rc != 0) return fail(FBK_E_HIP, std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : std::to_string(rc)));
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_comm_fence(fbk_ctx* ctx) try {
  FBK_ENTER_QUIET(ctx);
  if (!ctx) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!ctx->comm) return fail(FBK_E_INVALID, "comm: the context has no communicator (fbk_comm_init)");
  if (int32_t rc = set_device(ctx)) return rc;
  HIP_TRY(hipEventRecord(ctx->comm_ev_out, ctx->comm_stream));
  HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->comm_ev_out, 0));
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_comm_close(fbk_ctx* ctx) try {
  FBK_ENTER(ctx);
  if (!ctx) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  comm_release(ctx);
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"

namespace {
// (fbk_close: the stream is drained, then the communicator goes)
void comm_release(fbk_ctx* ctx) {
  if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
  if (ctx->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->comm);
  if (ctx->comm_ev_in) (void)hipEventDestroy(ctx->comm_ev_in);
  if (ctx->comm_ev_out) (void)hipEventDestroy(ctx->comm_ev_out);
  if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
  ctx->comm = nullptr;
  ctx->comm_stream = nullptr;
  ctx->comm_ev_in = ctx->comm_ev_out = nullptr;
}
}  // namespace
