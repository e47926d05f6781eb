// fbk_prepared_api.inc — prepared (launch-only) forms of the query-level calls (included by fbk.hip).
//
// fbk_plan_* made the PAIR operations launch-only in round 1: row lists resident, results left on the device.
// The query-level calls — the GroupBy / TopK count matrix, the n-way fold with its fused count, BSI Sum and the
// one-pass Sum(Range) — still paid 35-80 us around every kernel for what does not change between two executions
// of the same query shape on resident fragments: validating and uploading the row lists, allocating the result
// vectors, downloading the result, synchronising (round-2 bench line: BSI Range kernel 130.7 us, call 196.9 us).
// A prepared query (fbk_query) holds the row lists, the plane plan and the result buffers on the device:
//     fbk_query_*      create (validates and uploads once; synchronous)
//     fbk_query_run    memset + kernel(s) on the context's stream — asynchronous, no allocation, no copy, no sync;
//                      the result may be written to (or, for the count-valued kinds, accumulated into) a
//                      caller-owned device buffer: the cell of an all-reduce, the next operator's input
//     fbk_query_read   synchronise and copy the result of the last run to the host
// It is the unit one (query, node) call of mapperLocal (executor.go:6742) becomes when the same query runs again —
// and what the multi-GPU reduce wants: the partial matrix stays on the device for the collective.

enum FbkQueryKind : int32_t { kQCountMatrix = 1, kQFoldICount = 2, kQBsiSum = 3, kQBsiRangeSum = 4, kQBsiRange = 5, kQFold = 6, kQTopN = 7, kQCountMatrixSum = 8, kQExpr = 9, kQExprBsi = 10 };

struct fbk_query {
  fbk_ctx* ctx = nullptr;
  int32_t kind = 0;
  const fbk_batch *a = nullptr, *b = nullptr, *filter = nullptr;
  uint32_t n_a = 0, n_b = 0, k = 0, depth = 0;
  int32_t op = 0;
  uint64_t n = 0;  // shards / groups
  DevBuf rows;  // every row list of the query, one allocation
  const uint32_t* dr[3] = {nullptr, nullptr, nullptr};
  DevBuf result;   // count matrix: total [n_a * n_b]; fold: counts [n]; BSI: raw per-shard triples / quadruples
  DevBuf dplan;    // BSI range-sum: the RangeSumPlan
  fbk::RangeSumPlan plan{};
  uint64_t result_bytes = 0;
  // the kinds with a ROW result (BSI Range, materialised fold): an output batch of 8 KiB-strided cells the query owns and
  // every run rewrites (fbk_query_output lends it out until the next run / fbk_query_free), counts in `result`
  fbk_batch* out = nullptr;
  uint32_t out_flags = 0;   // FBK_SETOP_OPTIMIZE: the fold encodes in its epilogue
  DevBuf dprog;             // BSI Range: the plane program
  uint32_t prog_len = 0;
  // TopN (fbk_topn_api.inc): the n asked for, the pass buffers with their plan (thresholds, the candidate pass's n under the
  // semantics in force at prepare; totals in `result`) and the scratch of the on-device ordering — all sized at prepare
  struct Topn {
    uint32_t top_n = 0;
    TopnBuffers buf;
    TopnSort sort;
  };
  std::unique_ptr<Topn> topn;
  bool ran = false;
  void* last_out = nullptr;  // where the last run wrote (result.p or the caller's buffer)
  // folds and TopN: the resolved records of the rows dr[0] of `a` (fbk_query_api.inc)
  RowRecords recs;
  // the GroupBy count matrix (fbk_count_matrix_api.inc): row lists, per-shard matrices, and what its runs keep — the resolved records
  // of the TopK shape, the prepared program of the kernel over encoded rows; the totals are in `result`
  std::unique_ptr<MatrixPlan> matrix;
  // GroupBy with aggregate=Sum (fbk_matrix_sum_api.inc): row lists, scratch and the result {sums, counts}
  std::unique_ptr<MsumPlan> msum;
  // a whole call tree (fbk_expr_api.inc): row lists, leaf table and lowered program; out == nullptr: FBK_EXPR_COUNT_ONLY.
  // kQExprBsi: with the field of the aggregate terminal; `result` holds the raw words (ExprProgram::agg_words per shard)
  std::unique_ptr<ExprProgram> expr;
};

namespace {

int32_t query_check(fbk_ctx* ctx, const fbk_query* q) {
  if (!ctx || !q) return fail(FBK_E_INVALID, "NULL argument");
  if (q->ctx != ctx) return fail(FBK_E_INVALID, "query was prepared on another context");
  return FBK_OK;
}

int32_t query_finish_create(fbk_ctx* ctx, fbk_query* q, int32_t rc, fbk_query** out) {
  // the row lists went through the context's pinned staging: they must have landed before the call returns
  if (!rc) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = fail(FBK_E_HIP, std::string("query prepare: ") + hipGetErrorString(e));
  } else {
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (rc) {
    if (q->out) free_batch_storage(q->out);
    delete q;
    return rc;
  }
  *out = q;
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_query_count_matrix(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                               const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards,
                               uint32_t keep_per_shard, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !out_query) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (int32_t rc = count_matrix_args_ok(a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  const uint64_t width = uint64_t(n_a) * n_b;
  if (n_shards == 0 || width == 0) return fail(FBK_E_INVALID, "query: empty count matrix");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQCountMatrix;
  q->a = a;
  q->b = b;
  q->filter = filter;
  q->n_a = n_a;
  q->n_b = n_b;
  q->n = n_shards;
  q->result_bytes = width * 8;
  q->matrix.reset(new MatrixPlan());
  q->matrix->kept = true;
  int32_t rc = matrix_prepare(ctx, *q->matrix, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards, keep_per_shard != 0);
  if (!rc) {
    const hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);
} FBK_ABI_CATCH(ctx)

int32_t fbk_query_count_matrix_sum(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                                   uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, const fbk_batch* bsi, const uint32_t* base_rows,
                                   uint32_t bit_depth, uint32_t n_shards, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !out_query) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (int32_t rc = msum_args_ok(a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards)) return rc;
  if (n_shards == 0 || n_a == 0 || n_b == 0) return fail(FBK_E_INVALID, "query: empty count matrix");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQCountMatrixSum;
  q->a = a;
  q->b = b;
  q->filter = filter;
  q->n_a = n_a;
  q->n_b = n_b;
  q->n = n_shards;
  q->depth = bit_depth;
  q->result_bytes = uint64_t(n_a) * n_b * 16;
  q->msum.reset(new MsumPlan());
  const int32_t rc = msum_prepare(ctx, *q->msum, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards);
  return query_finish_create(ctx, q, rc, out_query);
} FBK_ABI_CATCH(ctx)

int32_t fbk_query_fold_intersection_count(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k,
                                          const fbk_batch* filter, const uint32_t* rows_f, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_query || (n_groups && ((k && !rows) || (filter && !rows_f)))) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (int32_t rc = fold_args_ok(op, n_groups, k)) return rc;
  if (n_groups == 0) return fail(FBK_E_INVALID, "query: no groups");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQFoldICount;
  q->a = batch;
  q->filter = filter;
  q->op = op;
  q->k = k;
  q->n = n_groups;
  q->result_bytes = n_groups * 8;
  int32_t rc = fold_n_icount_upload_rows(ctx, batch, rows, n_groups, k, filter, rows_f, q->rows, q->dr);
  if (!rc) {
    const hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);
} FBK_ABI_CATCH(ctx)

// op == 0: Sum over exists ∩ filter (fragment.sum); op = FBK_BSI_EQ .. FBK_BSI_GTE: Sum(Row(v op predicate), field = v) in one pass
// (only for the predicates the one-pass kernel serves: FBK_E_INVALID otherwise — the caller then runs fbk_bsi_range_sum)
int32_t fbk_query_bsi_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth, int32_t op,
                          int64_t predicate, const fbk_batch* filter, const uint32_t* rows_f, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_query || !base_rows || (filter && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (op != 0 && (op < FBK_BSI_EQ || op > FBK_BSI_GTE)) return fail(FBK_E_INVALID, "invalid range operation");
  if (n_shards == 0) return fail(FBK_E_INVALID, "query: no shards");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = op ? kQBsiRangeSum : kQBsiSum;
  q->a = batch;
  q->filter = filter;
  q->op = op;
  q->depth = bit_depth;
  q->n = n_shards;
  q->result_bytes = uint64_t(n_shards) * (op ? 32 : 24);
  int32_t rc = FBK_OK;
  if (op && !plan_range_sum(op, bit_depth, predicate, q->plan))
    rc = fail(FBK_E_INVALID, "query: this predicate is not served by the one-pass Sum(Range) (a special form of the reference): use fbk_bsi_range_sum");
  if (!rc) rc = upload_rows_multi(ctx, {{base_rows, n_shards, batch->n_rows}, {rows_f, filter ? uint64_t(n_shards) : 0, filter ? filter->n_rows : UINT32_MAX}}, q->rows, q->dr);
  if (!rc) {
    hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e == hipSuccess && op) {
      e = q->dplan.alloc(ctx, sizeof(q->plan));
      if (e == hipSuccess) e = hipMemcpyAsync(q->dplan.p, &q->plan, sizeof(q->plan), hipMemcpyHostToDevice, ctx->stream);
    }
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);
} FBK_ABI_CATCH(ctx)

// Row(v op predicate) over a BSI field with the result ROWS kept on the device (fragment.rangeOp, fragment.go:937-1303):
// the plane program is generated and uploaded once, the output batch (one row of 8 KiB cells per shard) and the
// per-shard counts belong to the query; a run is memset + k_bsi_range_slot.
int32_t fbk_query_bsi_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op, uint32_t bit_depth,
                            int64_t predicate, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_query || !base_rows) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (n_shards == 0) return fail(FBK_E_INVALID, "query: no shards");
  BsiProg prog;
  if (!gen_range_op(prog, op, bit_depth, predicate)) return fail(FBK_E_INVALID, "invalid range operation");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQBsiRange;
  q->a = batch;
  q->op = op;
  q->depth = bit_depth;
  q->n = n_shards;
  q->result_bytes = uint64_t(n_shards) * 8;
  q->prog_len = uint32_t(prog.v.size());
  int32_t rc = alloc_cell_batch(ctx, n_shards, &q->out);
  if (!rc) rc = upload_rows_multi(ctx, {{base_rows, n_shards, batch->n_rows}}, q->rows, q->dr);
  if (!rc) {
    hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e == hipSuccess) e = q->dprog.alloc(ctx, std::max<size_t>(prog.v.size(), 1) * 4);
    if (e == hipSuccess && !prog.v.empty()) e = hipMemcpyAsync(q->dprog.p, prog.v.data(), prog.v.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);  // (synchronises: `prog` is read by the copy above)
} FBK_ABI_CATCH(ctx)

// The n-way Union / Xor / Difference of k rows per group MATERIALISED (executeUnionShard executor.go:5382, executeXorShard
// :5513, executeDifferenceShard :2950; Bitmap.Union roaring.go:1272-1284), with Container.optimize() in the kernel's
// epilogue when flags has FBK_SETOP_OPTIMIZE: group lists resident, the output batch and the per-group counts owned by the
// query; a run is memset + ONE launch of k_fold_scatter.
int32_t fbk_query_fold(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k, uint32_t flags,
                       fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_query || (n_groups && k && !rows)) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  if (int32_t rc = fold_args_ok(op, n_groups, k)) return rc;
  if (n_groups == 0) return fail(FBK_E_INVALID, "query: no groups");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = check_rows(rows, n_groups * k, batch->n_rows, "fold_n")) return rc;
  if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(batch))) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQFold;
  q->a = batch;
  q->op = op;
  q->k = k;
  q->n = n_groups;
  q->out_flags = flags;
  q->result_bytes = n_groups * 8;
  int32_t rc = alloc_cell_batch(ctx, n_groups, &q->out);
  if (!rc) {
    fold_output_keys(batch, rows, n_groups, k, q->out);
    q->out->dense = false;
    rc = upload_rows_multi(ctx, {{rows, n_groups * k, UINT32_MAX}}, q->rows, q->dr);
  }
  if (!rc) {
    const hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);
} FBK_ABI_CATCH(ctx)

// A whole bitmap call tree (fbk_expr_eval / fbk_expr_count) prepared: the row list of every leaf, the leaf table and the lowered
// program are validated and uploaded once, the output batch (one row of 8 KiB cells per shard; none with FBK_EXPR_COUNT_ONLY)
// and the per-shard counts belong to the query; a run is memset + ONE launch of k_expr_slot.
int32_t fbk_query_expr(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                       uint32_t flags, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (!out_query) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (flags & ~(FBK_SETOP_OPTIMIZE | FBK_EXPR_COUNT_ONLY)) return fail(FBK_E_INVALID, "unknown flags");
  if (n_shards > (1u << 26)) return fail(FBK_E_INVALID, "too many shards in one call");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQExpr;
  q->n = n_shards;
  q->out_flags = flags;
  q->result_bytes = uint64_t(n_shards) * 8;
  q->expr.reset(new ExprProgram());
  int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, *q->expr);
  if (!rc && n_shards == 0) rc = fail(FBK_E_INVALID, "query: no shards");
  if (!rc && !(flags & FBK_EXPR_COUNT_ONLY)) {
    rc = alloc_cell_batch(ctx, n_shards, &q->out);
    if (!rc) rc = expr_output_keys(leaves, *q->expr, q->out);
  }
  if (!rc) {
    const hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);  // (synchronises: the upload reads the program's host image)
} FBK_ABI_CATCH(ctx)

// Sum / Min / Max of a BSI field over a whole call tree (fbk_expr_bsi_agg) prepared: row lists, leaf table, program and the field's
// base rows are validated and uploaded once; a run is memset + ONE launch of k_expr_agg_slot into the raw per-shard words.
int32_t fbk_query_expr_bsi(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                           uint32_t agg, const fbk_batch* batch, const uint32_t* base_rows, uint32_t bit_depth, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (!out_query) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (int32_t rc = expr_agg_args_ok(agg, batch, base_rows, bit_depth, n_shards)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQExprBsi;
  q->a = batch;
  q->depth = bit_depth;
  q->n = n_shards;
  q->expr.reset(new ExprProgram());
  int32_t rc = expr_agg_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, agg, batch, base_rows, bit_depth, *q->expr);
  if (!rc && n_shards == 0) rc = fail(FBK_E_INVALID, "query: no shards");
  if (!rc) {
    q->result_bytes = uint64_t(n_shards) * q->expr->agg_words() * 8;
    const hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);  // (synchronises: the upload reads the program's host image)
} FBK_ABI_CATCH(ctx)

// TopN / TopK (fragment.top's per-shard rules, executeTopN's sum over shards: fbk_topn) with nothing left to the host:
// row lists resident, per-shard counts, totals, and the ORDERING (a stable descending radix sort of (count, index) pairs that
// start in index order: count descending, row index ascending inside one count) on the device with its scratch sized at
// prepare.  A run leaves {counts, indexes, number of non-empty rows} on the device; fbk_query_read copies the first n.
int32_t fbk_query_topn(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f,
                       uint32_t n_shards, uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !out_query || !rows_a || (filter && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (int32_t rc = topn_args_ok(n_a, tanimoto_threshold)) return rc;
  if (n_shards == 0 || n_a == 0) return fail(FBK_E_INVALID, "query: empty TopN");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = check_rows(rows_a, uint64_t(n_shards) * n_a, a->n_rows, "topk rows")) return rc;
  fbk_query* q = new (std::nothrow) fbk_query();
  if (!q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->ctx = ctx;
  q->kind = kQTopN;
  q->a = a;
  q->filter = filter;
  q->n_a = n_a;
  q->n = n_shards;
  q->result_bytes = uint64_t(n_a) * 8;
  q->topn.reset(new fbk_query::Topn());
  q->topn->top_n = n;
  // (the semantics and option matrix_pass_kb in force when the query is prepared)
  const fbk_topn_plan::Sizes sizes = topn_plan(ctx, n_a, n_shards, TopnSource{filter}, min_threshold, tanimoto_threshold, topn_cand_n(ctx, n, n_a, true));
  int32_t rc = upload_rows_multi(ctx, {{rows_a, uint64_t(n_shards) * n_a, UINT32_MAX}, {rows_f, filter ? uint64_t(n_shards) : 0, filter ? filter->n_rows : UINT32_MAX}}, q->rows,
                                 q->dr);
  if (!rc) {
    hipError_t e = q->result.alloc(ctx, q->result_bytes);
    if (e == hipSuccess) e = q->topn->buf.alloc(ctx, sizes, q->result.as<u64>());
    if (e == hipSuccess) e = q->topn->sort.alloc(ctx, n_a);
    if (e != hipSuccess) rc = fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  return query_finish_create(ctx, q, rc, out_query);
} FBK_ABI_CATCH(ctx)

// The output batch of the last run of a query with a ROW result (fbk_query_bsi_range, fbk_query_fold): BORROWED — owned by the
// query, rewritten by its next run, freed with it.  Usable as an input of any
// later call on the same context (a filter for fbk_bsi_sum, an operand of a plan): everything is ordered by the stream.
int32_t fbk_query_output(fbk_ctx* ctx, fbk_query* q, fbk_batch** out_batch) try {
  FBK_ENTER(ctx);
  if (int32_t rc = query_check(ctx, q)) return rc;
  if (!out_batch) return fail(FBK_E_INVALID, "NULL argument");
  *out_batch = nullptr;
  if (!q->out) return fail(FBK_E_INVALID, "query: this kind of query has no row output");
  if (!q->ran) return fail(FBK_E_INVALID, "query: output asked for before the first run");
  *out_batch = q->out;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_query_run(fbk_ctx* ctx, fbk_query* q, void* device_out, uint32_t flags) try {
  FBK_ENTER(ctx);
  if (int32_t rc = query_check(ctx, q)) return rc;
  if (flags & ~FBK_QUERY_ACCUMULATE) return fail(FBK_E_INVALID, "unknown flags");
  const bool acc = (flags & FBK_QUERY_ACCUMULATE) != 0;
  if (acc && (q->kind == kQBsiSum || q->kind == kQBsiRangeSum)) return fail(FBK_E_INVALID, "query: BSI results are per-shard records, not accumulable");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  void* out = device_out ? device_out : q->result.p;
  int32_t rc = FBK_OK;
  switch (q->kind) {
    case kQCountMatrix:
      rc = matrix_enqueue(ctx, *q->matrix, static_cast<u64*>(out), acc);
      break;
    case kQCountMatrixSum:
      if (acc || device_out) return fail(FBK_E_INVALID, "query: a GroupBy Sum writes its own two arrays (fbk_query_read), nothing to accumulate");
      rc = msum_enqueue(ctx, *q->msum);
      if (!rc) out = q->msum->result.p;
      break;
    case kQFoldICount: {
      const Slot* recs = nullptr;
      if (q->op != FBK_OP_AND) rc = query_row_records(ctx, q->recs, q->a, q->dr[0], q->n, q->k, &recs);  // (the scatter kernels)
      if (!rc) rc = fold_n_icount_launch(ctx, q->op, q->a, q->dr, q->n, q->k, q->filter, static_cast<u64*>(out), acc, recs);
      break;
    }
    case kQBsiSum:
      rc = bsi_sum_launch(ctx, q->a, q->dr[0], uint32_t(q->n), q->depth, q->filter, q->filter ? q->dr[1] : nullptr, static_cast<u64*>(out));
      break;
    case kQBsiRangeSum:
      rc = bsi_range_sum_launch(ctx, q->a, q->dr[0], uint32_t(q->n), q->plan, q->dplan.as<fbk::RangeSumPlan>(), q->filter, q->filter ? q->dr[1] : nullptr,
                                static_cast<u64*>(out));
      break;
    case kQBsiRange: {
      if (acc) return fail(FBK_E_INVALID, "query: a row result cannot be accumulated");
      HIP_TRY(hipMemsetAsync(out, 0, q->n * 8, ctx->stream));
      {
        KernelSpan span(ctx);
        hipLaunchKernelGGL(fbk::k_bsi_range_slot, dim3(uint32_t(q->n * fbk::kSlots)), dim3(64), 0, ctx->stream, q->a->d_slots, q->a->d_arena, q->dr[0], uint32_t(q->n),
                           q->dprog.as<uint32_t>(), q->prog_len, uint32_t(q->depth + 2), q->out->d_arena, q->out->d_slots, (uint32_t*)nullptr, static_cast<u64*>(out), 0u);
      }
      HIP_TRY(hipGetLastError());
      slots_rewritten(q->out);
      break;
    }
    case kQFold: {
      if (acc) return fail(FBK_E_INVALID, "query: a row result cannot be accumulated");
      const Slot* recs = nullptr;
      if (q->op != FBK_OP_AND)
        if (int32_t rr = query_row_records(ctx, q->recs, q->a, q->dr[0], q->n, q->k, &recs)) return rr;
      HIP_TRY(hipMemsetAsync(out, 0, q->n * 8, ctx->stream));
      {
        KernelSpan span(ctx);
        if (q->out_flags & FBK_SETOP_OPTIMIZE)
          launch_fold<2>(q->op, uint32_t(q->n * fbk::kSlots), ctx->stream, q->a->d_slots, q->a->d_arena, q->dr[0], q->n, q->k, nullptr, nullptr, nullptr,
                         q->out->d_arena, q->out->d_slots, nullptr, static_cast<u64*>(out), recs);
        else
          launch_fold<1>(q->op, uint32_t(q->n * fbk::kSlots), ctx->stream, q->a->d_slots, q->a->d_arena, q->dr[0], q->n, q->k, nullptr, nullptr, nullptr,
                         q->out->d_arena, q->out->d_slots, nullptr, static_cast<u64*>(out), recs);
      }
      HIP_TRY(hipGetLastError());
      slots_rewritten(q->out);
      break;
    }
    case kQExpr: {
      const bool rows = q->out != nullptr;
      if (rows && (acc || device_out)) return fail(FBK_E_INVALID, "query: a row result cannot be accumulated or redirected (only the FBK_EXPR_COUNT_ONLY form)");
      if (!acc) HIP_TRY(hipMemsetAsync(out, 0, q->n * 8, ctx->stream));
      rc = expr_launch(ctx, *q->expr, rows ? q->out->d_arena : nullptr, rows ? q->out->d_slots : nullptr, nullptr, static_cast<u64*>(out),
                       rows && (q->out_flags & FBK_SETOP_OPTIMIZE));
      if (!rc && rows) slots_rewritten(q->out);
      break;
    }
    case kQExprBsi: {
      const bool sum = q->expr->agg == FBK_AGG_SUM;  // {psum, nsum, count} add up; the slot records of Min / Max do not
      if (!sum && (acc || device_out)) return fail(FBK_E_INVALID, "query: Min / Max write per-slot records of their own (fbk_query_read), nothing to accumulate or redirect");
      if (sum && !acc) HIP_TRY(hipMemsetAsync(out, 0, q->result_bytes, ctx->stream));
      rc = expr_agg_launch(ctx, *q->expr, static_cast<u64*>(out));
      break;
    }
    case kQTopN: {
      if (acc) return fail(FBK_E_INVALID, "query: TopN totals are ordered by the run, not accumulable");
      if (device_out) return fail(FBK_E_INVALID, "query: a TopN writes its own buffers (fbk_query_read)");
      const Slot* recs = nullptr;
      if (q->filter) rc = query_row_records(ctx, q->recs, q->a, q->dr[0], q->n, q->n_a, &recs);  // (k_rows_vs_filter; without a filter the stored cardinalities answer)
      if (rc) break;
      TopnSort& s = q->topn->sort;
      rc = topn_totals_enqueue(ctx, q->a, q->dr[0], TopnSource{q->filter, q->dr[1], recs}, q->topn->buf, /*mask=*/true);
      if (rc) break;
      if (q->n_a <= fbk::kRankSortMax) {
        // a field of a few thousand rows: every row finds its own rank (one launch; the radix sort's five launches were 30 of
        // the 154 us of TopN(10) over config 3's 64 rows)
        HIP_TRY(hipMemsetAsync(s.dnz.p, 0, 4, ctx->stream));
        hipLaunchKernelGGL(fbk::k_rank_sort_desc, dim3((q->n_a + 255) / 256), dim3(256), 0, ctx->stream, q->result.as<u64>(), q->n_a, s.dsk.as<u64>(), s.dsv.as<uint32_t>(),
                           s.dnz.as<uint32_t>());
        HIP_TRY(hipGetLastError());
      } else {
        rc = topn_radix_enqueue(ctx, s, q->result.as<u64>(), q->n_a);
      }
      break;
    }
    default:
      rc = fail(FBK_E_INVALID, "query: unknown kind");
  }
  if (!rc) {
    q->ran = true;
    q->last_out = out;
  }
  return rc;
} FBK_ABI_CATCH(ctx)

int32_t fbk_query_result(fbk_ctx* ctx, fbk_query* q, void** out_device_ptr, uint64_t* out_bytes) try {
  FBK_ENTER(ctx);
  if (int32_t rc = query_check(ctx, q)) return rc;
  if (out_device_ptr) *out_device_ptr = q->msum ? q->msum->result.p : q->result.p;  // (GroupBy Sum: {sums, counts})
  if (out_bytes) *out_bytes = q->result_bytes;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_query_read(fbk_ctx* ctx, fbk_query* q, void* out0, void* out1) try {
  FBK_ENTER(ctx);
  if (int32_t rc = query_check(ctx, q)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!q->ran) return fail(FBK_E_INVALID, "query: read before the first run");
  if (int32_t rc = set_device(ctx)) return rc;
  D2H back(ctx);
  switch (q->kind) {
    case kQCountMatrix:
      // out0 = total [n_a * n_b] (may be NULL), out1 = per-shard matrices [n_shards][n_a * n_b] (prepared with keep_per_shard)
      if (out1 && !q->matrix->keep_per_shard) return fail(FBK_E_INVALID, "query: prepared without keep_per_shard");
      return matrix_read(ctx, *q->matrix, static_cast<const u64*>(q->last_out), static_cast<uint64_t*>(out0), static_cast<uint64_t*>(out1));
    case kQCountMatrixSum:  // out0 = int64 sums [n_a * n_b], out1 = uint64 counts [n_a * n_b]
      return msum_read(ctx, *q->msum, static_cast<int64_t*>(out0), static_cast<uint64_t*>(out1));
    case kQFoldICount:
    case kQBsiRange:  // out0 = the per-shard cardinalities of the result rows
    case kQFold:      // out0 = the per-group cardinalities
    case kQExpr:      // out0 = the per-shard cardinalities of the tree's result
      if (out0) HIP_TRY(back.add(out0, q->last_out, q->result_bytes));
      HIP_TRY(back.finish());
      return FBK_OK;
    case kQTopN: {
      // out0 = uint32 {number of results, then that many row indexes}  (1 + min(n, n_a) words, n = 0: 1 + n_a);
      // out1 = uint64 counts of those rows
      const fbk_query::Topn& t = *q->topn;
      uint32_t nz = 0;
      HIP_TRY(back.add(&nz, t.sort.dnz.p, 4));
      HIP_TRY(back.finish());
      const uint32_t want = t.top_n ? std::min(t.top_n, nz) : nz;  // rows without a single common column are not results
      uint32_t* idx = static_cast<uint32_t*>(out0);
      if (idx) idx[0] = want;
      if (want) {
        D2H back2(ctx);
        if (idx) HIP_TRY(back2.add(idx + 1, t.sort.dsv.p, uint64_t(want) * 4));
        if (out1) HIP_TRY(back2.add(out1, t.sort.dsk.p, uint64_t(want) * 8));
        HIP_TRY(back2.finish());
      }
      return FBK_OK;
    }
    case kQBsiSum:
    case kQBsiRangeSum: {
      // out0 = int64 sums [n_shards], out1 = uint64 counts [n_shards]
      const int w = q->kind == kQBsiSum ? 3 : 4;
      std::vector<u64> h(q->n * w);
      HIP_TRY(back.add(h.data(), q->last_out, h.size() * 8));
      HIP_TRY(back.finish());
      int64_t* sums = static_cast<int64_t*>(out0);
      uint64_t* counts = static_cast<uint64_t*>(out1);
      for (uint64_t s = 0; s < q->n; ++s) {
        if (q->kind == kQBsiSum) {  // Total(): int64(psum) - int64(nsum) (roaring/filter.go:1106-1108)
          if (sums) sums[s] = int64_t(h[s * 3 + 0] - h[s * 3 + 1]);
          if (counts) counts[s] = h[s * 3 + 2];
        } else {
          const uint64_t sm = h[s * 4 + 0], so = h[s * 4 + 1];
          if (sums) sums[s] = int64_t(q->plan.scan_positive ? sm - so : so - sm);
          if (counts) counts[s] = h[s * 4 + 2] + h[s * 4 + 3];
        }
      }
      return FBK_OK;
    }
    case kQExprBsi: {  // out0 = int64 values [n_shards], out1 = uint64 counts [n_shards]
      std::vector<u64> h(q->n * q->expr->agg_words());
      HIP_TRY(back.add(h.data(), q->last_out, h.size() * 8));
      HIP_TRY(back.finish());
      expr_agg_fold(*q->expr, h.data(), static_cast<int64_t*>(out0), static_cast<uint64_t*>(out1));
      return FBK_OK;
    }
    default:
      return fail(FBK_E_INVALID, "query: unknown kind");
  }
} FBK_ABI_CATCH(ctx)

int32_t fbk_query_free(fbk_ctx* ctx, fbk_query* q) try {
  FBK_ENTER(ctx);
  if (!q) return FBK_OK;
  if (!ctx) ctx = q->ctx;
  if (q->ctx != ctx) return fail(FBK_E_INVALID, "query was prepared on another context");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  (void)hipStreamSynchronize(ctx->stream);  // nothing of the query may still be running when its buffers go back to the pool
  if (q->out) free_batch_storage(q->out);
  delete q;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
