// fbk_expr_api.inc — host side of fbk_expr_count / fbk_expr_eval and the pieces fbk_query_expr shares with them (included by
// fbk.hip before fbk_prepared_api.inc).  The planner is fbk_expr_plan.h (HIP-free), the kernel k_expr_slot (fbk_expr.hip.h).

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
  const fbk::ExprLeaf* d_leaves() const { return reinterpret_cast<const fbk::ExprLeaf*>(static_cast<const uint8_t*>(buf.p) + off_leaves); }
  const uint32_t* d_prog() const { return reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(buf.p) + off_prog); }
  uint32_t lds_bytes() const { return (1u + plan.slots) * 8192u; }
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

// one launch: the tree over every (shard, slot).  outSlots == NULL: counts only.
int32_t expr_launch(fbk_ctx* ctx, ExprProgram& P, uint8_t* arenaO, Slot* outSlots, uint32_t* outRuns, u64* d_counts, bool encode) {
  bool patched = false;
  for (size_t l = 0; l < P.batches.size(); ++l) {
    fbk::ExprLeaf& h = P.h_leaves[l];
    if (h.slots != P.batches[l]->d_slots || h.arena != P.batches[l]->d_arena) {
      h.slots = P.batches[l]->d_slots;
      h.arena = P.batches[l]->d_arena;
      patched = true;
    }
  }
  if (patched) {  // (a leaf's batch was optimised / compacted since the upload)
    HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(P.buf.p) + P.off_leaves, P.h_leaves.data(), P.h_leaves.size() * sizeof(fbk::ExprLeaf), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_expr_slot, dim3(uint32_t(uint64_t(P.n_shards) * fbk::kSlots)), dim3(64), P.lds_bytes(), ctx->stream, P.d_leaves(), P.d_prog(),
                       uint32_t(P.plan.ins.size()), P.n_shards, P.plan.slots, arenaO, outSlots, outRuns, d_counts, uint32_t(encode));
  }
  HIP_TRY(hipGetLastError());
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
  struct Drain {  // the upload reads P.blob: nothing of P may go while the stream still holds work
    fbk_ctx* c;
    ~Drain() { (void)hipStreamSynchronize(c->stream); }
  } drain{ctx};
  if (int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, P)) return rc;
  if (n_shards == 0) return FBK_OK;
  HIP_TRY(dcnt.alloc(ctx, uint64_t(n_shards) * 8));
  HIP_TRY(hipMemsetAsync(dcnt.p, 0, uint64_t(n_shards) * 8, ctx->stream));
  if (int32_t rc = expr_launch(ctx, P, nullptr, nullptr, nullptr, dcnt.as<u64>(), false)) return rc;
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
  struct Drain {
    fbk_ctx* c;
    ~Drain() { (void)hipStreamSynchronize(c->stream); }
  } drain{ctx};
  CellOutput out;  // (after the drain guard: freed first, and its own destructor drains as well)
  if (int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, P)) return rc;
  if (int32_t rc = out.alloc(ctx, n_shards, n_shards, "expr")) return rc;
  if (n_shards) {
    if (int32_t rc = expr_output_keys(leaves, P, out.batch())) return rc;
    // optimize() asked for: applied by the kernel itself (option setop_direct_encode = 2; otherwise the separate re-encode pass)
    const bool enc = (flags & FBK_SETOP_OPTIMIZE) && ctx->opt.setop_direct_encode == 2;
    if (int32_t rc = expr_launch(ctx, P, out.batch()->d_arena, out.batch()->d_slots, out.runs(), out.counts(), enc)) return rc;
    if (int32_t rc = out.finish(enc ? (flags & ~uint32_t(FBK_SETOP_OPTIMIZE)) : flags, n_shards, out_counts, enc)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
