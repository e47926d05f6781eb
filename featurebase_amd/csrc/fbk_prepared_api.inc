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
//
// Every kind has a plan struct in its own file, shared with the one-shot call: its *_prepare / *_enqueue / *_read are what the
// creators and the two switches below call.  Nothing is launched from this file.

enum FbkQueryKind : int32_t { kQCountMatrix = 1, kQFoldICount = 2, kQBsiSum = 3, kQBsiRange = 5, kQFold = 6, kQTopN = 7, kQCountMatrixSum = 8, kQExpr = 9, kQExprBsi = 10 };

struct fbk_query {
  fbk_ctx* ctx = nullptr;
  int32_t kind = 0;
  // count matrix: total [n_a * n_b]; folds, BSI Range, call tree: counts per group / shard; BSI Sum and the tree's aggregates: raw
  // words per shard; TopN: totals [n_a].  (GroupBy Sum: its plan's own {sums, counts}, result_bytes of them.)
  DevBuf result;
  uint64_t result_bytes = 0;
  // the kinds with a ROW result (BSI Range, materialised fold, call tree): an output batch of 8 KiB-strided cells the query owns and
  // every run rewrites (fbk_query_output lends it out until the next run / fbk_query_free), counts in `result`
  std::unique_ptr<fbk_batch, decltype(&free_batch_storage)> out{nullptr, free_batch_storage};
  bool ran = false;
  void* last_out = nullptr;  // where the last run wrote (result.p or the caller's buffer)
  // the kind's plan: exactly one of these
  std::unique_ptr<MatrixPlan> matrix;       // fbk_count_matrix_api.inc
  std::unique_ptr<MsumPlan> msum;           // fbk_matrix_sum_api.inc
  std::unique_ptr<FoldPlan> fold;           // fbk_fold_api.inc (both fold kinds)
  std::unique_ptr<BsiSumPlan> bsi_sum;      // fbk_bsi_api.inc (Sum and the one-pass Sum(Range))
  std::unique_ptr<BsiRangePlan> bsi_range;  // fbk_bsi_api.inc
  std::unique_ptr<TopnPlan> topn;           // fbk_topn_api.inc
  std::unique_ptr<ExprProgram> expr;        // fbk_expr_api.inc (both call-tree kinds; out == nullptr: FBK_EXPR_COUNT_ONLY)
};

namespace {

int32_t query_check(fbk_ctx* ctx, const fbk_query* q) {
  if (!ctx || !q) return fail(FBK_E_INVALID, "NULL argument");
  if (q->ctx != ctx) return fail(FBK_E_INVALID, "query was prepared on another context");
  return FBK_OK;
}

// A query from its `new` until finish() gives the handle to the caller.  Leaving a creator any other way — a failed step, an
// exception out of a std::vector — drains the context's stream (host vectors of the query may be the sources of queued copies)
// and deletes the query.  Declared under the context's lock and after set_device, so that the destructor runs under both.
// fbk_query_free deletes through it as well.
struct QueryGuard {
  fbk_ctx* ctx;
  fbk_query* q;
  QueryGuard(fbk_ctx* c, int32_t kind) : ctx(c), q(new (std::nothrow) fbk_query()) {
    if (q) q->ctx = c, q->kind = kind;
  }
  QueryGuard(fbk_ctx* c, fbk_query* owned) : ctx(c), q(owned) {}
  QueryGuard(const QueryGuard&) = delete;
  QueryGuard& operator=(const QueryGuard&) = delete;
  ~QueryGuard() {
    if (!q) return;
    (void)hipStreamSynchronize(ctx->stream);  // nothing of the query may still be running when its buffers go back to the pool
    delete q;
  }
  fbk_query* operator->() const { return q; }
  // the query's own result buffer
  int32_t alloc_result(uint64_t bytes) {
    q->result_bytes = bytes;
    const hipError_t e = q->result.alloc(ctx, bytes);
    return e == hipSuccess ? FBK_OK : fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  }
  // the output batch of a kind with a row result
  int32_t alloc_rows(uint64_t n_rows) {
    fbk_batch* o = nullptr;
    const int32_t rc = alloc_cell_batch(ctx, n_rows, &o);
    q->out.reset(o);
    return rc;
  }
  // rc of the creator's steps so far; FBK_OK: the uploads went through the context's pinned staging and must have landed before
  // the call returns, then the handle is the caller's
  int32_t finish(int32_t rc, fbk_query** out) {
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(FBK_E_HIP, std::string("query prepare: ") + hipGetErrorString(e));
    *out = q;
    q = nullptr;
    return FBK_OK;
  }
};

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
  QueryGuard q(ctx, kQCountMatrix);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->matrix.reset(new MatrixPlan());
  q->matrix->kept = true;
  int32_t rc = matrix_prepare(ctx, *q->matrix, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards, keep_per_shard != 0);
  if (!rc) rc = q.alloc_result(width * 8);
  return q.finish(rc, out_query);
} FBK_ABI_CATCH(ctx)

int32_t fbk_query_count_matrix_sum(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                                   uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, const fbk_batch* bsi, const uint32_t* base_rows,
                                   uint32_t bit_depth, uint32_t n_shards, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !out_query) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  const GroupFieldArgs args{a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards};
  if (int32_t rc = msum_args_ok(args)) return rc;
  if (n_shards == 0 || n_a == 0 || n_b == 0) return fail(FBK_E_INVALID, "query: empty count matrix");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  QueryGuard q(ctx, kQCountMatrixSum);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->result_bytes = uint64_t(n_a) * n_b * 16;  // (in the plan's own buffer)
  q->msum.reset(new MsumPlan());
  return q.finish(msum_prepare(ctx, *q->msum, args), out_query);
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
  QueryGuard q(ctx, kQFoldICount);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->fold.reset(new FoldPlan());
  int32_t rc = fold_prepare(ctx, *q->fold, op, batch, rows, n_groups, k, filter, rows_f);
  if (!rc) rc = q.alloc_result(n_groups * 8);
  return q.finish(rc, out_query);
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
  fbk::RangeSumPlan range{};
  if (op && !plan_range_sum(op, bit_depth, predicate, range))
    return fail(FBK_E_INVALID, "query: this predicate is not served by the one-pass Sum(Range) (a special form of the reference): use fbk_bsi_range_sum");
  QueryGuard q(ctx, kQBsiSum);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->bsi_sum.reset(new BsiSumPlan());
  int32_t rc = bsi_sum_prepare(ctx, *q->bsi_sum, batch, base_rows, n_shards, bit_depth, filter, rows_f, op ? &range : nullptr);
  if (!rc) rc = q.alloc_result(uint64_t(n_shards) * q->bsi_sum->words() * 8);
  return q.finish(rc, out_query);
} FBK_ABI_CATCH(ctx)

// Row(v op predicate) over a BSI field with the result ROWS kept on the device (fragment.rangeOp, fragment.go:937-1303):
// the plane program is generated and uploaded once, the output batch (one row of 8 KiB cells per shard) and the
// per-shard counts belong to the query; a run is memset + one launch.
int32_t fbk_query_bsi_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op, uint32_t bit_depth,
                            int64_t predicate, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_query || !base_rows) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (n_shards == 0) return fail(FBK_E_INVALID, "query: no shards");
  BsiProg prog;  // (before the guard: a queued copy reads it until the guard or finish() has drained the stream)
  if (!gen_range_op(prog, op, bit_depth, predicate)) return fail(FBK_E_INVALID, "invalid range operation");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  QueryGuard q(ctx, kQBsiRange);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->bsi_range.reset(new BsiRangePlan());
  int32_t rc = q.alloc_rows(n_shards);
  if (!rc) rc = bsi_range_prepare(ctx, *q->bsi_range, batch, base_rows, n_shards, bit_depth, prog, "query");
  if (!rc) rc = q.alloc_result(uint64_t(n_shards) * 8);
  return q.finish(rc, out_query);
} FBK_ABI_CATCH(ctx)

// The n-way Union / Xor / Difference of k rows per group MATERIALISED (executeUnionShard executor.go:5382, executeXorShard
// :5513, executeDifferenceShard :2950; Bitmap.Union roaring.go:1272-1284), with Container.optimize() in the kernel's
// epilogue when flags has FBK_SETOP_OPTIMIZE: group lists resident, the output batch and the per-group counts owned by the
// query; a run is memset + ONE launch.
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
  if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(batch))) return rc;
  QueryGuard q(ctx, kQFold);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->fold.reset(new FoldPlan());
  q->fold->encode = (flags & FBK_SETOP_OPTIMIZE) != 0;
  int32_t rc = q.alloc_rows(n_groups);
  if (!rc) rc = fold_prepare(ctx, *q->fold, op, batch, rows, n_groups, k, nullptr, nullptr);  // (validates the rows whose keys are read next)
  if (!rc) fold_output_keys(batch, rows, n_groups, k, q->out.get());
  if (!rc) rc = q.alloc_result(n_groups * 8);
  return q.finish(rc, out_query);
} FBK_ABI_CATCH(ctx)

// A whole bitmap call tree (fbk_expr_eval / fbk_expr_count) prepared: the row list of every leaf, the leaf table and the lowered
// program are validated and uploaded once, the output batch (one row of 8 KiB cells per shard; none with FBK_EXPR_COUNT_ONLY)
// and the per-shard counts belong to the query; a run is memset + ONE launch.
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
  QueryGuard q(ctx, kQExpr);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->expr.reset(new ExprProgram());
  q->expr->encode = (flags & FBK_SETOP_OPTIMIZE) != 0;
  int32_t rc = expr_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, *q->expr);
  if (!rc && n_shards == 0) rc = fail(FBK_E_INVALID, "query: no shards");
  if (!rc && !(flags & FBK_EXPR_COUNT_ONLY)) {
    rc = q.alloc_rows(n_shards);
    if (!rc) rc = expr_output_keys(leaves, *q->expr, q->out.get());
  }
  if (!rc) rc = q.alloc_result(uint64_t(n_shards) * 8);
  return q.finish(rc, out_query);
} FBK_ABI_CATCH(ctx)

// Sum / Min / Max of a BSI field over a whole call tree (fbk_expr_bsi_agg) prepared: row lists, leaf table, program and the field's
// base rows are validated and uploaded once; a run is memset + ONE launch into the raw per-shard words.
int32_t fbk_query_expr_bsi(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t n_shards,
                           uint32_t agg, const fbk_batch* batch, const uint32_t* base_rows, uint32_t bit_depth, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (int32_t rc = expr_args_ok(ctx, leaves, n_leaves, prog, n_prog)) return rc;
  if (!out_query) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (int32_t rc = expr_agg_args_ok(agg, batch, base_rows, bit_depth, n_shards)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  QueryGuard q(ctx, kQExprBsi);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->expr.reset(new ExprProgram());
  int32_t rc = expr_agg_prepare(ctx, leaves, n_leaves, prog, n_prog, n_shards, agg, batch, base_rows, bit_depth, *q->expr);
  if (!rc && n_shards == 0) rc = fail(FBK_E_INVALID, "query: no shards");
  if (!rc) rc = q.alloc_result(uint64_t(n_shards) * q->expr->agg_words() * 8);
  return q.finish(rc, out_query);
} FBK_ABI_CATCH(ctx)

// TopN / TopK with nothing left to the host (TopnPlan): a run leaves the ordered {counts, indexes, number of non-empty rows} on the
// device; fbk_query_read copies the first n.
int32_t fbk_query_topn(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f,
                       uint32_t n_shards, uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold, fbk_query** out_query) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !out_query || !rows_a || (filter && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  *out_query = nullptr;
  if (int32_t rc = topn_args_ok(n_a, tanimoto_threshold)) return rc;
  if (n_shards == 0 || n_a == 0) return fail(FBK_E_INVALID, "query: empty TopN");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  QueryGuard q(ctx, kQTopN);
  if (!q.q) return fail(FBK_E_NOMEM, "host allocation failed");
  q->topn.reset(new TopnPlan());
  int32_t rc = q.alloc_result(uint64_t(n_a) * 8);  // the totals
  if (!rc) rc = topn_prepare(ctx, *q->topn, a, rows_a, n_a, filter, rows_f, n_shards, n, min_threshold, tanimoto_threshold, q->result.as<u64>());
  return q.finish(rc, out_query);
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
  *out_batch = q->out.get();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

// Each case: the kind's rule on FBK_QUERY_ACCUMULATE and a caller's device_out, then its enqueue.
int32_t fbk_query_run(fbk_ctx* ctx, fbk_query* q, void* device_out, uint32_t flags) try {
  FBK_ENTER(ctx);
  if (int32_t rc = query_check(ctx, q)) return rc;
  if (flags & ~FBK_QUERY_ACCUMULATE) return fail(FBK_E_INVALID, "unknown flags");
  const bool acc = (flags & FBK_QUERY_ACCUMULATE) != 0;
  if (acc && q->kind == kQBsiSum) return fail(FBK_E_INVALID, "query: BSI results are per-shard records, not accumulable");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  void* out = device_out ? device_out : q->result.p;
  u64* out64 = static_cast<u64*>(out);
  int32_t rc = FBK_OK;
  switch (q->kind) {
    case kQCountMatrix:
      rc = matrix_enqueue(ctx, *q->matrix, out64, acc);
      break;
    case kQCountMatrixSum:
      if (acc || device_out) return fail(FBK_E_INVALID, "query: a GroupBy Sum writes its own two arrays (fbk_query_read), nothing to accumulate");
      rc = msum_enqueue(ctx, *q->msum);
      out = q->msum->result.p;
      break;
    case kQFoldICount:
      rc = fold_n_icount_launch(ctx, *q->fold, out64, acc, /*use_records=*/true);
      break;
    case kQBsiSum:
      rc = bsi_sum_enqueue(ctx, *q->bsi_sum, out64);
      break;
    case kQBsiRange:
      if (acc) return fail(FBK_E_INVALID, "query: a row result cannot be accumulated");
      rc = bsi_range_enqueue(ctx, *q->bsi_range, q->out.get(), out64);
      break;
    case kQFold:
      if (acc) return fail(FBK_E_INVALID, "query: a row result cannot be accumulated");
      rc = fold_enqueue(ctx, *q->fold, q->out.get(), out64);
      break;
    case kQExpr:
      if (q->out && (acc || device_out)) return fail(FBK_E_INVALID, "query: a row result cannot be accumulated or redirected (only the FBK_EXPR_COUNT_ONLY form)");
      rc = expr_enqueue(ctx, *q->expr, q->out.get(), out64, acc);
      break;
    case kQExprBsi:  // {psum, nsum, count} add up; the slot records of Min / Max do not
      if (q->expr->agg != FBK_AGG_SUM && (acc || device_out))
        return fail(FBK_E_INVALID, "query: Min / Max write per-slot records of their own (fbk_query_read), nothing to accumulate or redirect");
      rc = expr_agg_enqueue(ctx, *q->expr, out64, acc);
      break;
    case kQTopN:
      if (acc) return fail(FBK_E_INVALID, "query: TopN totals are ordered by the run, not accumulable");
      if (device_out) return fail(FBK_E_INVALID, "query: a TopN writes its own buffers (fbk_query_read)");
      rc = topn_enqueue(ctx, *q->topn);
      break;
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
    case kQExpr: {    // out0 = the per-shard cardinalities of the tree's result
      D2H back(ctx);
      if (out0) HIP_TRY(back.add(out0, q->last_out, q->result_bytes));
      HIP_TRY(back.finish());
      return FBK_OK;
    }
    case kQTopN:  // out0 = uint32 {number of results, then the row indexes}, out1 = uint64 counts of those rows
      return topn_read(ctx, *q->topn, static_cast<uint32_t*>(out0), static_cast<uint64_t*>(out1));
    case kQBsiSum:  // out0 = int64 sums [n_shards], out1 = uint64 counts [n_shards]
      return bsi_sum_read(ctx, *q->bsi_sum, q->last_out, static_cast<int64_t*>(out0), static_cast<uint64_t*>(out1));
    case kQExprBsi:  // out0 = int64 values [n_shards], out1 = uint64 counts [n_shards]
      return expr_agg_read(ctx, *q->expr, q->last_out, static_cast<int64_t*>(out0), static_cast<uint64_t*>(out1));
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
  QueryGuard drop(ctx, q);  // drains the stream, then deletes
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
