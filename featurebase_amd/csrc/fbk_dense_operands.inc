// fbk_dense_operands.inc — the operands of kernels that read dense rows only (fbk_count_matrix_sum, fbk_count_matrix_distinct,
// fbk_bsi_distinct, fbk_extract_*, fbk_bsi_sort), and small argument checks the BSI and extract calls share.  Included by fbk.hip
// before fbk_query_api.inc.
//
// An operand of a dense batch is read in place.  One of a batch that is not dense is densified a chunk of shards at a time
// (k_densify_rows) into scratch, and the kernel reads the scratch through a list of the rows' places in it.  DenseOperands decides
// which, builds the lists, lays the operands of a call out in ONE scratch buffer in the order they were added, and hands a call
// site the (arena, rows) pair its kernel takes for the chunk [s0, s0 + ns).  How many shards a chunk holds is the caller's own
// arithmetic (fbk_dense_policy.h's even_chunk with its budget and per-shard term: fbk.h documents it per call); the loop over the
// chunks is for_each_chunk.  Two frames stand on it: GroupFieldOperands (fbk_group_field.inc), FieldOperands (fbk_sort_api.inc).

namespace {

using fbk::even_chunk;  // fbk_dense_policy.h, as the size of a dense row
using fbk::kDenseRowBytes;
static_assert(kDenseRowBytes == uint64_t(fbk::kSlots) * 8192, "");

void densify_launch(fbk_ctx* ctx, const std::vector<fbk::DensifySrc>& srcs) {  // three sources per launch
  for (size_t k0 = 0; k0 < srcs.size(); k0 += 3) {
    fbk::DensifyArgs args{};
    uint64_t cells = 0;
    for (size_t k = k0; k < std::min(srcs.size(), k0 + 3); ++k) {
      args.src[k - k0] = srcs[k];
      cells += srcs[k].n_rows * fbk::kSlots;
    }
    hipLaunchKernelGGL(fbk::k_densify_rows, dim3(uint32_t((cells + 3) / 4)), dim3(256), 0, ctx->stream, args);
  }
}

struct DenseView {
  const uint8_t* arena = nullptr;
  const uint32_t* rows = nullptr;  // of the chunk's first shard
  uint32_t stride = 0;             // list entries per shard
};

class DenseOperands {
 public:
  // An operand: rps rows per shard in `rows` (host), or a BSI fragment of rps = depth + 2 rows per shard behind the one base row
  // per shard in `rows`.  batch == nullptr: the call has no such operand (its view is empty).  Returns the operand's number.
  // force: through scratch even if the batch is dense.
  int add(const fbk_batch* batch, const uint32_t* rows, uint32_t rps, bool fragment = false, bool force = false) {
    Op o;
    o.batch = batch, o.h_rows = rows, o.rps = rps, o.fragment = fragment;
    o.was_dense = batch && batch->dense, o.densified = batch && (force || !batch->dense);
    ops_.push_back(o);
    return int(ops_.size()) - 1;
  }

  // rows per shard that go through scratch: kDenseRowBytes times this is their share of a caller's per-shard term
  uint64_t densified_rows() const {
    uint64_t n = 0;
    for (const Op& o : ops_) n += o.densified ? o.rps : 0;
    return n;
  }

  // Every list of the call in one host->device copy, and the scratch for chunks of `chunk` shards.  block_rows < rps (one operand,
  // chunk == 1): the scratch holds that many rows of a shard at a time (densify_one's i0, nr).
  int32_t upload(fbk_ctx* ctx, uint32_t n_shards, uint32_t chunk, uint32_t block_rows = UINT32_MAX) {
    std::vector<std::vector<uint32_t>> lists;
    lists.reserve(2 * ops_.size());
    std::vector<RowsArg> args;
    uint64_t at = 0;  // rows of scratch so far
    for (Op& o : ops_) {
      if (!o.batch) continue;
      args.push_back({o.h_rows, uint64_t(n_shards) * (o.fragment ? 1 : o.rps), UINT32_MAX});
      if (!o.densified) continue;
      o.held = std::min(o.rps, block_rows);
      o.at = at;
      std::vector<uint32_t> idx(o.fragment ? chunk : uint64_t(chunk) * o.held);
      for (uint64_t i = 0; i < idx.size(); ++i) idx[i] = uint32_t(at + (o.fragment ? i * o.rps : i));
      at += uint64_t(chunk) * o.held;
      lists.push_back(std::move(idx));
      args.push_back({lists.back().data(), lists.back().size(), UINT32_MAX});
      if (!o.fragment) continue;
      std::vector<uint32_t> all(uint64_t(n_shards) * o.rps);
      for (uint32_t s = 0; s < n_shards; ++s)
        for (uint32_t r = 0; r < o.rps; ++r) all[uint64_t(s) * o.rps + r] = o.h_rows[s] + r;
      lists.push_back(std::move(all));
      args.push_back({lists.back().data(), lists.back().size(), UINT32_MAX});
    }
    std::vector<const uint32_t*> d(args.size());
    if (int32_t rc = upload_rows_multi(ctx, args, lists_, d.data())) return rc;
    size_t k = 0;
    for (Op& o : ops_) {
      if (!o.batch) continue;
      o.d_rows = o.d_src = d[k++];
      if (o.densified) o.d_idx = d[k++];
      if (o.densified && o.fragment) o.d_src = d[k++];
      o.h_rows = nullptr;  // (the caller's list: not kept beyond the call)
    }
    if (at) HIP_TRY(scratch_.alloc(ctx, at * kDenseRowBytes));
    n_shards_ = n_shards, chunk_ = chunk;
    return FBK_OK;
  }

  // THE walk over the shards upload() laid out: for every chunk [s0, s0 + ns), densify, then fn(s0, ns).  fn returns nothing, or an
  // error code that ends the walk and is returned.  A call that walks more than once says which walk is its first: a single chunk
  // is still in the scratch for the later ones and is not densified again.
  enum class Densify { together, each };  // one launch for all operands, or one per operand in the order they were added
  template <class Fn>
  int32_t for_each_chunk(fbk_ctx* ctx, bool first_walk, Densify how, Fn&& fn) {
    const bool stale = first_walk || chunk_ < n_shards_;
    for (uint32_t s0 = 0; s0 < n_shards_; s0 += chunk_) {
      const uint32_t ns = std::min(chunk_, n_shards_ - s0);
      if (stale && how == Densify::together) densify(ctx, s0, ns);
      else if (stale)
        for (size_t k = 0; k < ops_.size(); ++k) densify_one(ctx, int(k), s0, ns);
      if constexpr (std::is_void_v<decltype(fn(s0, ns))>) fn(s0, ns);
      else if (int32_t rc = fn(s0, ns)) return rc;
    }
    return FBK_OK;
  }

  // the chunk [s0, s0 + ns) of every operand that goes through scratch
  void densify(fbk_ctx* ctx, uint32_t s0, uint32_t ns) {
    std::vector<fbk::DensifySrc> srcs;
    for (const Op& o : ops_)
      if (o.densified) srcs.push_back(src(o, s0, ns, 0, o.rps));
    densify_launch(ctx, srcs);
  }
  // ... of one operand, in a launch of its own; rows [i0, i0 + nr) of the shard s0 with upload's block_rows (ns == 1)
  void densify_one(fbk_ctx* ctx, int k, uint32_t s0, uint32_t ns, uint32_t i0 = 0, uint32_t nr = UINT32_MAX) {
    const Op& o = ops_[k];
    if (o.densified) densify_launch(ctx, {src(o, s0, ns, i0, std::min(nr, o.rps))});
  }

  // what the kernel takes for a chunk that starts at shard s0 (and at row i0 of it)
  DenseView view(int k, uint32_t s0, uint32_t i0 = 0) const {
    const Op& o = ops_[k];
    if (!o.batch) return {};
    if (o.densified) return {static_cast<const uint8_t*>(scratch_.p), o.d_idx, o.fragment ? 1 : o.held};
    return {o.batch->d_arena, rows(k, s0) + i0, o.fragment ? 1 : o.rps};
  }
  // the operand's own list on the device, from shard s0 on
  const uint32_t* rows(int k, uint32_t s0) const {
    const Op& o = ops_[k];
    return o.d_rows + uint64_t(s0) * (o.fragment ? 1 : o.rps);
  }

  // a batch was re-encoded since add(): what upload() laid out no longer fits it
  bool layout_changed() const {
    for (const Op& o : ops_)
      if (o.batch && o.batch->dense != o.was_dense) return true;
    return false;
  }

 private:
  struct Op {
    const fbk_batch* batch;
    const uint32_t* h_rows;
    uint32_t rps;
    bool fragment, densified, was_dense;
    uint32_t held = 0;  // rows of a shard the scratch holds
    uint64_t at = 0;    // first row of the operand's part of the scratch
    const uint32_t *d_rows = nullptr, *d_src = nullptr, *d_idx = nullptr;  // as given; every row to densify; places in the scratch
  };
  fbk::DensifySrc src(const Op& o, uint32_t s0, uint32_t ns, uint32_t i0, uint32_t nr) const {
    return {o.batch->d_slots, o.batch->d_arena, o.d_src + uint64_t(s0) * o.rps + i0, uint64_t(ns) * nr, static_cast<uint8_t*>(scratch_.p) + o.at * kDenseRowBytes};
  }
  std::vector<Op> ops_;
  uint32_t n_shards_ = 0, chunk_ = 0;  // upload()'s
  DevBuf lists_;
  DevBuf scratch_;
};

// out[0 .. n] = *carry + the exclusive prefix of counts[0 .. n); *carry moves on by the total (k_bsi_cell_scan over plain counts)
void exclusive_scan_u32(fbk_ctx* ctx, const uint32_t* counts, uint32_t n, u64* out, u64* carry) {
  hipLaunchKernelGGL(fbk::k_bsi_cell_scan, dim3(1), dim3(1024), 0, ctx->stream, static_cast<const Slot*>(nullptr), static_cast<const uint32_t*>(nullptr), counts, n,
                     out, carry);
}

int32_t bsi_rows_ok(const uint32_t* base_rows, uint64_t n_shards, uint64_t bit_depth, uint64_t n_rows) {
  for (uint64_t s = 0; s < n_shards; ++s)
    if (uint64_t(base_rows[s]) + 2 + bit_depth > n_rows) return fail(FBK_E_INVALID, "bsi: fragment rows (exists, sign, bit planes) exceed the batch");
  return FBK_OK;
}

int32_t shard_ids_ok(const uint64_t* shard_ids, uint32_t n_shards, const char* what) {
  for (uint32_t s = 0; s < n_shards; ++s) {
    if (shard_ids[s] >= (1ull << 44)) return fail(FBK_E_INVALID, std::string(what) + ": shard id >= 2^44 (column ids are shard * 2^20 + position)");
    if (s && shard_ids[s] <= shard_ids[s - 1]) return fail(FBK_E_INVALID, std::string(what) + ": shard_ids must be strictly ascending");
  }
  return FBK_OK;
}

}  // namespace
