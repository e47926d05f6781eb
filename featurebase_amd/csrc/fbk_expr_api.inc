// fbk_expr_api.inc — host side of fbk_expr_count / fbk_expr_eval / fbk_expr_bsi_agg and the pieces fbk_query_expr and
// fbk_query_expr_bsi share with them (included by fbk.hip before fbk_prepared_api.inc).  The planner is fbk_expr_plan.h (HIP-free),
// the kernels k_expr_slot and k_expr_agg_slot (fbk_expr.hip.h).

namespace {

// What one call tree needs on the device: the row list of every leaf, the leaf table and the lowered program, ONE upload.
struct ExprProgram {
  fbk_expr::Plan plan;
  std::vector<const fbk_batch*> batches;  // per leaf
  std::vector<fbk::ExprLeaf> h_leaves;    // the leaf table as uploaded (a batch whose arena was rewritten since is patched at the next launch)
  std::vector<uint8_t> blob;              // host image of the upload (alive until the copy has landed)
  DevBuf buf;
  uint64_t off_leaves = 0, off_prog = 0;
  uint32_t n_shards = 0;
  bool encode = false;  // a prepared query with rows: FBK_SETOP_OPTIMIZE, the kernel encodes
  const fbk::ExprLeaf* d_leaves() const { return reinterpret_cast<const fbk::ExprLeaf*>(static_cast<const uint8_t*>(buf.p) + off_leaves); }
  const uint32_t* d_prog() const { return reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(buf.p) + off_prog); }
  uint32_t lds_bytes() const { return (1u + plan.slots) * 8192u; }
  // fbk_expr_bsi_agg / fbk_query_expr_bsi: the BSI field the aggregate terminal scans (agg_batch == nullptr: none)
  const fbk_batch* agg_batch = nullptr;
  DevBuf agg_base;  // its base rows [n_shards]
  uint32_t agg = 0, agg_depth = 0;
  // words per shard the aggregate leaves on the device: {psum, nsum, count}, or 16 slots of {magnitude, count | scan flag}
  uint64_t agg_words() const { return agg == FBK_AGG_SUM ? 3 : 2 * uint64_t(fbk::kSlots); }
};

// Declared after the ExprProgram (fbk_expr_topk_api.inc: the ExprRows) of a one-shot call: the upload reads P.blob, nothing of it may go
// while the stream still holds work.
struct StreamDrain {
  fbk_ctx* c;
  ~StreamDrain() { (void)hipStreamSynchronize(c->stream); }
};

int32_t expr_args_ok(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog) {
  if (!ctx || (n_leaves && !leaves) || (n_prog && !prog)) return fail(FBK_E_INVALID, "NULL argument");
  return FBK_OK;
}

// Validates everything (program, leaves, row lists) and enqueues the upload.  Nothing is launched on a failure.
int32_t expr_prepare(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                     ExprProgram& P) {
  if (fbk_expr::Error e = fbk_expr::plan(leaves, n_leaves, prog, n_prog, P.plan)) return fail(FBK_E_INVALID, e.msg);
  P.n_shards = n_shards;
  P.batches.resize(n_leaves);
  P.h_leaves.resize(n_leaves);
  const uint64_t seg = (uint64_t(n_shards) + 3) & ~uint64_t(3);  // 16-byte aligned row lists
  for (uint32_t l = 0; l < n_leaves; ++l) {
    const fbk_expr_leaf& f = leaves[l];
    const uint32_t n_rows = f.kind == FBK_EXPR_ROW ? 1u : f.bit_depth + 2u;
    if (n_shards && !f.rows) return fail(FBK_E_INVALID, "NULL argument");
    for (uint32_t s = 0; s < n_shards; ++s)
      if (uint64_t(f.rows[s]) + n_rows > f.batch->n_rows)
        return fail(FBK_E_INVALID, f.kind == FBK_EXPR_ROW ? "expr: row index out of range" : "expr: fragment rows (exists, sign, bit planes) exceed the batch");
    P.batches[l] = f.batch;
    P.h_leaves[l] = fbk::ExprLeaf{f.batch->d_slots, f.batch->d_arena, nullptr, n_rows, 0};
  }
  if (n_shards == 0) return FBK_OK;
  P.off_leaves = seg * 4 * n_leaves;
  P.off_prog = P.off_leaves + uint64_t(n_leaves) * sizeof(fbk::ExprLeaf);
  const uint64_t total = P.off_prog + P.plan.ins.size() * 4;
  HIP_TRY(P.buf.alloc(ctx, total));
  P.blob.assign(total, 0);
  for (uint32_t l = 0; l < n_leaves; ++l) {
    std::memcpy(P.blob.data() + seg * 4 * l, leaves[l].rows, uint64_t(n_shards) * 4);
    P.h_leaves[l].rows = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(P.buf.p) + seg * 4 * l);
  }
  std::memcpy(P.blob.data() + P.off_leaves, P.h_leaves.data(), uint64_t(n_leaves) * sizeof(fbk::ExprLeaf));
  std::memcpy(P.blob.data() + P.off_prog, P.plan.ins.data(), P.plan.ins.size() * 4);
  HIP_TRY(hipMemcpyAsync(P.buf.p, P.blob.data(), total, hipMemcpyHostToDevice, ctx->stream));
  if (P.lds_bytes() > 65536u)  // a deep tree's stack: beyond the default cap of a workgroup's dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fbk::k_expr_slot), hipFuncAttributeMaxDynamicSharedMemorySize, int(P.lds_bytes())));
  return FBK_OK;
}

// a leaf's batch that was optimised / compacted since the upload: its pointers in the device's leaf table are renewed
int32_t expr_patch_leaves(fbk_ctx* ctx, ExprProgram& P) {
  bool patched = false;
  for (size_t l = 0; l < P.batches.size(); ++l) {
    fbk::ExprLeaf& h = P.h_leaves[l];
    if (h.slots != P.batches[l]->d_slots || h.arena != P.batches[l]->d_arena) {
      h.slots = P.batches[l]->d_slots;
      h.arena = P.batches[l]->d_arena;
      patched = true;
    }
  }
  if (patched) {
    HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(P.buf.p) + P.off_leaves, P.h_leaves.data(), P.h_leaves.size() * sizeof(fbk::ExprLeaf), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return FBK_OK;
}

// one launch: the tree over every (shard, slot).  outSlots == NULL: counts only.
int32_t expr_launch(fbk_ctx* ctx, ExprProgram& P, uint8_t* arenaO, Slot* outSlots, uint32_t* outRuns, u64* d_counts, bool encode) {
  if (int32_t rc = expr_patch_leaves(ctx, P)) return rc;
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_expr_slot, dim3(uint32_t(uint64_t(P.n_shards) * fbk::kSlots)), dim3(64), P.lds_bytes(), ctx->stream, P.d_leaves(), P.d_prog(),
                       uint32_t(P.plan.ins.size()), P.n_shards, P.plan.slots, arenaO, outSlots, outRuns, d_counts, uint32_t(encode));
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// a run of the prepared form: memset (unless the counts accumulate) + ONE launch; o == NULL: FBK_EXPR_COUNT_ONLY
int32_t expr_enqueue(fbk_ctx* ctx, ExprProgram& P, fbk_batch* o, u64* d_counts, bool accumulate) {
  if (!accumulate) HIP_TRY(hipMemsetAsync(d_counts, 0, uint64_t(P.n_shards) * 8, ctx->stream));
  if (int32_t rc = expr_launch(ctx, P, o ? o->d_arena : nullptr, o ? o->d_slots : nullptr, nullptr, d_counts, o && P.encode)) return rc;
  if (o) slots_rewritten(o);
  return FBK_OK;
}

// output keys of a tree whose first pushed leaf is a ROW: those of that row (a row without containers: 0), as a fold takes its
// first row's.  A tree that starts with a BSI predicate keeps the default keys (row ordinal * 16 + slot), as fbk_bsi_range does.
int32_t expr_output_keys(const fbk_expr_leaf* leaves, const ExprProgram& P, fbk_batch* o) {
  const fbk_expr_leaf& f = leaves[P.plan.first_leaf];
  if (f.kind != FBK_EXPR_ROW) return FBK_OK;
  if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(f.batch))) return rc;
  for (uint32_t s = 0; s < P.n_shards; ++s) {
    uint64_t high = 0;
    (void)row_key_high(f.batch, f.rows[s], &high);
    set_row_keys(o, s, high);
  }
  return FBK_OK;
}

// ---- the tree, then Sum / Min / Max of a BSI field over its result (k_expr_agg_slot) -------------------------------------------

// what fbk_expr_bsi_agg and fbk_query_expr_bsi ask of the aggregate's own arguments (the tree's: expr_prepare); no device work
int32_t expr_agg_args_ok(uint32_t agg, const fbk_batch* batch, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards) {
  if (agg > FBK_AGG_MAX) return fail(FBK_E_INVALID, "expr: unknown aggregate (FBK_AGG_SUM, FBK_AGG_MIN, FBK_AGG_MAX)");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (!batch || (n_shards && !base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (n_shards > (1u << 26)) return fail(FBK_E_INVALID, "too many shards in one call");
  return bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows);
}

// expr_prepare plus the field: everything validated, the base rows uploaded.  Nothing is launched on a failure.
int32_t expr_agg_prepare(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                         uint32_t agg, const fbk_batch* batch, const uint32_t* base_rows, uint32_t bit_depth, ExprProgram& P) {
  if (int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, P)) return rc;
  P.agg_batch = batch;
  P.agg = agg;
  P.agg_depth = bit_depth;
  if (n_shards == 0) return FBK_OK;
  if (int32_t rc = upload_rows(ctx, base_rows, n_shards, UINT32_MAX, P.agg_base)) return rc;  // (validated: expr_agg_args_ok)
  if (P.lds_bytes() > 65536u)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fbk::k_expr_agg_slot), hipFuncAttributeMaxDynamicSharedMemorySize, int(P.lds_bytes())));
  return FBK_OK;
}

// one launch into d_out [n_shards * P.agg_words()].  Sum adds to what is there (the caller zeroes it, or accumulates); Min / Max
// write every word.  The field's batch is read where it is NOW (a batch compacted since the prepare has new pointers).
int32_t expr_agg_launch(fbk_ctx* ctx, ExprProgram& P, u64* d_out) {
  if (int32_t rc = expr_patch_leaves(ctx, P)) return rc;
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_expr_agg_slot, dim3(uint32_t(uint64_t(P.n_shards) * fbk::kSlots)), dim3(64), P.lds_bytes(), ctx->stream, P.d_leaves(), P.d_prog(),
                       uint32_t(P.plan.ins.size()), P.n_shards, P.plan.slots, P.agg_batch->d_slots, P.agg_batch->d_arena, P.agg_base.as<uint32_t>(),
                       P.agg_depth, P.agg, d_out);
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// a run of the prepared form into d_out; Sum: zeroed first unless it accumulates
int32_t expr_agg_enqueue(fbk_ctx* ctx, ExprProgram& P, u64* d_out, bool accumulate) {
  if (P.agg == FBK_AGG_SUM && !accumulate) HIP_TRY(hipMemsetAsync(d_out, 0, uint64_t(P.n_shards) * P.agg_words() * 8, ctx->stream));
  return expr_agg_launch(ctx, P, d_out);
}

// the downloaded words -> per-shard (value, count), as fbk_bsi_sum / fbk_bsi_min / fbk_bsi_max give them; either output may be NULL
void expr_agg_fold(const ExprProgram& P, const u64* h, int64_t* out_vals, uint64_t* out_counts) {
  std::vector<int64_t> v(P.n_shards);
  std::vector<uint64_t> c(P.n_shards);
  if (P.agg == FBK_AGG_SUM) bsi_sum_fold(h, P.n_shards, v.data(), c.data());
  else bsi_minmax_fold(h, P.n_shards, P.agg == FBK_AGG_MAX ? 1u : 0u, v.data(), c.data());
  if (out_vals) std::memcpy(out_vals, v.data(), uint64_t(P.n_shards) * 8);
  if (out_counts) std::memcpy(out_counts, c.data(), uint64_t(P.n_shards) * 8);
}

// the raw words of a run at d_raw -> per-shard (value, count) on the host (one synchronisation)
int32_t expr_agg_read(fbk_ctx* ctx, const ExprProgram& P, const void* d_raw, int64_t* out_vals, uint64_t* out_counts) {
  std::vector<u64> h;
  if (int32_t rc = download_words(ctx, d_raw, uint64_t(P.n_shards) * P.agg_words(), h)) return rc;
  expr_agg_fold(P, h.data(), out_vals, out_counts);
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_expr_count(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                       uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (n_shards && !out_counts) return fail(FBK_E_INVALID, "NULL argument");
  if (n_shards > (1u << 26)) return fail(FBK_E_INVALID, "too many shards in one call");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  ExprProgram P;
  DevBuf dcnt;
  StreamDrain drain{ctx};
  if (int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, P)) return rc;
  if (n_shards == 0) return FBK_OK;
  HIP_TRY(dcnt.alloc(ctx, uint64_t(n_shards) * 8));
  if (int32_t rc = expr_enqueue(ctx, P, nullptr, dcnt.as<u64>(), false)) return rc;
  D2H back(ctx);
  HIP_TRY(back.add(out_counts, dcnt.p, uint64_t(n_shards) * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_expr_eval(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                      uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (!out_batch) return fail(FBK_E_INVALID, "NULL argument");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  if (n_shards > (1u << 26)) return fail(FBK_E_INVALID, "too many shards in one call");
  *out_batch = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  ExprProgram P;
  StreamDrain drain{ctx};
  CellOutput out;  // (after the drain guard: freed first, and its own destructor drains as well)
  if (int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, P)) return rc;
  if (int32_t rc = out.alloc(ctx, n_shards, n_shards, "expr")) return rc;
  if (n_shards) {
    if (int32_t rc = expr_output_keys(leaves, P, out.batch())) return rc;
    if (int32_t rc = expr_launch(ctx, P, out.batch()->d_arena, out.batch()->d_slots, out.runs(), out.counts(), out.kernel_encodes(flags))) return rc;
    if (int32_t rc = out.finish(n_shards, out_counts)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_expr_bsi_agg(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                         uint32_t agg, const fbk_batch* batch, const uint32_t* base_rows, uint32_t bit_depth, int64_t* out_vals,
                         uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (n_shards && (!out_vals || !out_counts)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = expr_agg_args_ok(agg, batch, base_rows, bit_depth, n_shards)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  ExprProgram P;
  DevBuf dout;
  StreamDrain drain{ctx};
  if (int32_t rc = expr_agg_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, agg, batch, base_rows, bit_depth, P)) return rc;
  if (n_shards == 0) return FBK_OK;
  HIP_TRY(dout.alloc(ctx, uint64_t(n_shards) * P.agg_words() * 8));
  if (int32_t rc = expr_agg_enqueue(ctx, P, dout.as<u64>(), false)) return rc;
  return expr_agg_read(ctx, P, dout.p, out_vals, out_counts);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
