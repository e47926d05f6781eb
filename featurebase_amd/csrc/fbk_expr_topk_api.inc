// fbk_expr_topk_api.inc — host side of fbk_expr_row_counts / fbk_expr_topk / fbk_expr_topn: the counting operators over a call
// tree (included by fbk.hip after fbk_topn_api.inc).  The tree is prepared as for fbk_expr_count (expr_prepare: one upload), the
// field's rows are one more upload, and topn_totals_enqueue (fbk_topn_api.inc) runs with the tree as its filter source: its
// buffers (TopnBuffers, sized by fbk_topn_plan::plan), its passes and topn_order_locked are those of fbk_topk / fbk_topn — only the
// counting launch (expr_rows_launch there: k_expr_rows_vs_filter, fbk_expr_topk.hip.h) and the origin of the per-shard filter
// counts differ.  No output batch, one synchronisation.
//
// Not here: a prepared fbk_query_* form; fbk_topn_partials / fbk_group_topn over a tree (with out_per_shard and out_total of
// fbk_expr_row_counts a rank can still reduce counts itself); k_expr_slot on the block-wide evaluator.

namespace {

constexpr uint32_t kExprRowsStaticLds = 20480;  // F + rank + T of k_expr_rows_vs_filter

// What the three calls keep on the device until their results are read: the tree, the field's rows, and in B the totals [n_a]
// (d_total), the (last) pass's per-shard counts (shard) and every shard's filter count (src).
struct ExprRows {
  ExprProgram P;
  DevBuf drows;
  TopnBuffers B;
};

int32_t expr_rows_args_ok(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a,
                          const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards) {
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (!a || (n_shards && n_a && !rows_a)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = topn_args_ok(n_a, 0)) return rc;  // (the Tanimoto range: after the outputs' NULL check, expr_topn_impl)
  if (n_shards > (1u << 26)) return fail(FBK_E_INVALID, "too many shards in one call");
  return FBK_OK;
}

// ctx->mu held.  Validates everything, then enqueues the uploads and the launches.  keep_per_shard: one pass over all shards (R.B.shard
// = [n_shards][n_a]); keep_src: R.B.src = [n_shards] filter counts.  *done: nothing to count (n_a == 0 or n_shards == 0).
int32_t expr_rows_totals_locked(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a,
                                const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards, uint64_t min_threshold, uint64_t tanimoto_threshold, uint32_t cand_n,
                                bool keep_per_shard, bool keep_src, ExprRows& R, bool* done) {
  *done = true;
  if (int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, R.P)) return rc;
  if (n_shards == 0 || n_a == 0) return FBK_OK;
  if (int32_t rc = check_rows(rows_a, uint64_t(n_shards) * n_a, a->n_rows, "topk rows")) return rc;
  if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(a))) return rc;
  *done = false;
  if (int32_t rc = upload_rows(ctx, rows_a, uint64_t(n_shards) * n_a, UINT32_MAX, R.drows)) return rc;
  const uint32_t stack_bytes = R.P.plan.slots * 8192u;
  if (kExprRowsStaticLds + stack_bytes > 65536u)  // a deep tree's saved values: beyond the default cap of a workgroup's LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fbk::k_expr_rows_vs_filter), hipFuncAttributeMaxDynamicSharedMemorySize, int(stack_bytes)));
  const TopnSource S{nullptr, nullptr, nullptr, &R.P};
  HIP_TRY(R.B.alloc(ctx, topn_plan(ctx, n_a, n_shards, S, min_threshold, tanimoto_threshold, cand_n, keep_per_shard, keep_src)));
  return topn_totals_enqueue(ctx, a, R.drows.as<uint32_t>(), S, R.B, /*mask=*/true);
}

int32_t expr_topn_impl(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a, const uint32_t* rows_a,
                       uint32_t n_a, uint32_t n_shards, uint32_t k, uint64_t min_threshold, uint64_t tanimoto_threshold, uint32_t* out_index, uint64_t* out_count,
                       uint32_t cap, uint32_t* out_n, bool reference_operator) {
  if (int32_t rc = expr_rows_args_ok(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards)) return rc;
  if (!out_n || (cap && (!out_index || !out_count))) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = topn_args_ok(n_a, tanimoto_threshold)) return rc;
  *out_n = 0;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  ExprRows R;
  StreamDrain drain{ctx};
  const uint32_t cand_n = topn_cand_n(ctx, k, n_a, reference_operator);
  bool done = false;
  if (int32_t rc = expr_rows_totals_locked(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards, min_threshold, tanimoto_threshold, cand_n, false, false, R,
                                           &done))
    return rc;
  if (done) return FBK_OK;
  return topn_order_locked(ctx, R.B.d_total, n_a, k, out_index, out_count, cap, out_n);
}

}  // namespace

extern "C" {

int32_t fbk_expr_row_counts(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a,
                            const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards, uint64_t* out_total, uint64_t* out_per_shard,
                            uint64_t* out_filter_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = expr_rows_args_ok(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards)) return rc;
  if (n_a && !out_total) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  ExprRows R;
  StreamDrain drain{ctx};
  bool done = false;
  if (int32_t rc = expr_rows_totals_locked(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards, 0, 0, 0, out_per_shard != nullptr,
                                           out_filter_counts != nullptr, R, &done))
    return rc;
  if (done) {
    if (n_a == 0) return FBK_OK;  // nothing written
    std::memset(out_total, 0, uint64_t(n_a) * 8);  // (n_shards == 0)
    return FBK_OK;
  }
  D2H back(ctx);
  HIP_TRY(back.add(out_total, R.B.d_total, uint64_t(n_a) * 8));
  if (out_per_shard) HIP_TRY(back.add(out_per_shard, R.B.shard.p, uint64_t(n_shards) * n_a * 8));
  if (out_filter_counts) HIP_TRY(back.add(out_filter_counts, R.B.src.p, uint64_t(n_shards) * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_expr_topk(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a,
                      const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards, uint32_t k, uint32_t* out_index, uint64_t* out_count, uint32_t cap,
                      uint32_t* out_n) try {
  FBK_ENTER(ctx);
  return expr_topn_impl(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards, k, 0, 0, out_index, out_count, cap, out_n, false);
} FBK_ABI_CATCH(ctx)

int32_t fbk_expr_topn(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a,
                      const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards, uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold,
                      uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n) try {
  FBK_ENTER(ctx);
  return expr_topn_impl(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards, n, min_threshold, tanimoto_threshold, out_index, out_count, cap, out_n,
                        /*reference_operator=*/true);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
