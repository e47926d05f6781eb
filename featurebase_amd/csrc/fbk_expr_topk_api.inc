// fbk_expr_topk_api.inc — host side of fbk_expr_row_counts / fbk_expr_topk / fbk_expr_topn: the counting operators over a call
// tree (included by fbk.hip after fbk_expr_api.inc).  The tree is prepared as for fbk_expr_count (expr_prepare: one upload), the
// field's rows are one more upload, and topn_totals_enqueue (fbk_query_api.inc) runs with the tree as its filter source: its
// passes, k_row_cardinality, k_topn_candidates, k_topn_filter, k_reduce_shards and topn_order_locked are those of fbk_topk /
// fbk_topn — only the counting launch (k_expr_rows_vs_filter, fbk_expr_topk.hip.h) and the origin of the per-shard filter counts
// differ.  No output batch, one synchronisation.
//
// Not here: a prepared fbk_query_* form; fbk_topn_partials / fbk_group_topn over a tree (with out_per_shard and out_total of
// fbk_expr_row_counts a rank can still reduce counts itself); k_expr_slot on the block-wide evaluator.

namespace {

// the counting launch of one pass: shards [p0, p0 + pn) of the call, d_ra = their rows of the field, dshard [pn][n_a] zeroed by the
// caller, dsrc [pn] (zeroed) or nullptr
int32_t expr_rows_launch(fbk_ctx* ctx, ExprProgram& P, const fbk_batch* a, const uint32_t* d_ra, uint32_t n_a, uint32_t p0, uint32_t pn, u64* dshard, u64* dsrc) {
  if (int32_t rc = expr_patch_leaves(ctx, P)) return rc;
  const uint32_t rpb = fbk_expr::rows_per_block(n_a, pn, fbk_expr::operand_reads(P.plan.ins));
  const uint32_t chunks = (n_a + rpb - 1) / rpb;
  const uint32_t stack_bytes = P.plan.slots * 8192u;
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_expr_rows_vs_filter, dim3(pn * 16 * chunks), dim3(256), stack_bytes, ctx->stream, P.d_leaves(), P.d_prog(), uint32_t(P.plan.ins.size()),
                       P.plan.slots, p0, a->d_slots, a->d_arena, d_ra, n_a, pn, rpb, dshard, dsrc);
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

constexpr uint32_t kExprRowsStaticLds = 20480;  // F + rank + T of k_expr_rows_vs_filter

// What the three calls keep on the device until their results are read: the tree, the field's rows, the totals [n_a] in dtot, the
// (last) pass's per-shard counts in dshard and every shard's filter count in dsrc.
struct ExprRows {
  ExprProgram P;
  DevBuf drows, dshard, dcards, dsrc, dtot, dcand;
};

int32_t expr_rows_args_ok(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a,
                          const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards) {
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (!a || (n_shards && n_a && !rows_a)) return fail(FBK_E_INVALID, "NULL argument");
  if (n_a > (1u << 22)) return fail(FBK_E_INVALID, "topk: at most 2^22 rows");
  if (n_shards > (1u << 26)) return fail(FBK_E_INVALID, "too many shards in one call");
  return FBK_OK;
}

// ctx->mu held.  Validates everything, then enqueues the uploads and the launches.  keep_per_shard: one pass over all shards (dshard
// = [n_shards][n_a]); keep_src: dsrc = [n_shards] filter counts.  *done: nothing to count (n_a == 0 or n_shards == 0).
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
  const bool thresholds = min_threshold > 0 || tanimoto_threshold > 0;
  const uint64_t pass_bytes = uint64_t(ctx->opt.matrix_pass_kb) << 10;
  const uint64_t pass_shards = keep_per_shard ? n_shards : std::max<uint64_t>(1, std::min<uint64_t>(n_shards, pass_bytes / (uint64_t(n_a) * 8)));
  HIP_TRY(R.dtot.alloc(ctx, uint64_t(n_a) * 8));
  HIP_TRY(R.dshard.alloc(ctx, pass_shards * n_a * 8));
  if (thresholds || cand_n) HIP_TRY(R.dcards.alloc(ctx, pass_shards * n_a * 8));
  if (thresholds || cand_n || keep_src) HIP_TRY(R.dsrc.alloc(ctx, uint64_t(n_shards) * 8));
  if (cand_n) HIP_TRY(R.dcand.alloc(ctx, uint64_t(n_a) * 8));
  return topn_totals_enqueue(ctx, a, R.drows.as<uint32_t>(), n_a, nullptr, nullptr, n_shards, min_threshold, tanimoto_threshold, pass_shards, R.dshard.as<u64>(),
                             R.dcards.as<u64>(), R.dsrc.as<u64>(), R.dtot.as<u64>(), nullptr, cand_n, R.dcand.as<u64>(), &R.P);
}

int32_t expr_topn_impl(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, const fbk_batch* a, const uint32_t* rows_a,
                       uint32_t n_a, uint32_t n_shards, uint32_t k, uint64_t min_threshold, uint64_t tanimoto_threshold, uint32_t* out_index, uint64_t* out_count,
                       uint32_t cap, uint32_t* out_n, bool reference_operator) {
  if (int32_t rc = expr_rows_args_ok(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards)) return rc;
  if (!out_n || (cap && (!out_index || !out_count))) return fail(FBK_E_INVALID, "NULL argument");
  if (tanimoto_threshold > 100) return fail(FBK_E_INVALID, "topn: Tanimoto threshold is a percentage (0..100)");
  *out_n = 0;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  ExprRows R;
  struct Drain {  // the upload reads P.blob: nothing of R may go while the stream still holds work
    fbk_ctx* c;
    ~Drain() { (void)hipStreamSynchronize(c->stream); }
  } drain{ctx};
  const uint32_t cand_n = topn_cand_n(ctx, k, n_a, reference_operator);
  bool done = false;
  if (int32_t rc = expr_rows_totals_locked(ctx, leaves, n_leaves, prog, n_prog, a, rows_a, n_a, n_shards, min_threshold, tanimoto_threshold, cand_n, false, false, R,
                                           &done))
    return rc;
  if (done) return FBK_OK;
  if (cand_n) hipLaunchKernelGGL(fbk::k_topn_mask, dim3((n_a + 255) / 256), dim3(256), 0, ctx->stream, R.dtot.as<u64>(), R.dcand.as<u64>(), n_a);
  HIP_TRY(hipGetLastError());
  return topn_order_locked(ctx, R.dtot, n_a, k, out_index, out_count, cap, out_n);
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
  struct Drain {
    fbk_ctx* c;
    ~Drain() { (void)hipStreamSynchronize(c->stream); }
  } drain{ctx};
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
  HIP_TRY(back.add(out_total, R.dtot.p, uint64_t(n_a) * 8));
  if (out_per_shard) HIP_TRY(back.add(out_per_shard, R.dshard.p, uint64_t(n_shards) * n_a * 8));
  if (out_filter_counts) HIP_TRY(back.add(out_filter_counts, R.dsrc.p, uint64_t(n_shards) * 8));
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
