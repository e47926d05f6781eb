// fbk_fold_api.inc — host side of the n-way folds (included by fbk.hip after fbk_query_api.inc): fbk_fold_n / fbk_union_n, the fused
// counts fbk_fold_n_intersection_count / fbk_union_n_intersection_count, and FoldPlan, which these one-shot calls share with
// fbk_query_fold and fbk_query_fold_intersection_count (fbk_prepared_api.inc).

namespace {

template <int WRITE>  // 0 counts only, 1 bitmap cells (+ run counts), 2 Container.optimize() in the kernel's epilogue
void launch_fold(int32_t op, uint32_t blocks, hipStream_t st, const Slot* slots, const uint8_t* arena, const uint32_t* rows,
                 uint64_t n_groups, uint32_t k, const Slot* fslots, const uint8_t* farena, const uint32_t* frows,
                 uint8_t* arenaO, Slot* outSlots, uint32_t* outRuns, u64* out_counts, const Slot* recs = nullptr) {
#define FBK_FOLD(OPC)                                                                                               \
  hipLaunchKernelGGL((fbk::k_fold_n<OPC, WRITE>), dim3(blocks), dim3(256), 0, st, slots, arena, rows, n_groups, k, \
                     fslots, farena, frows, arenaO, outSlots, outRuns, out_counts)
#define FBK_SCATTER(OPC)                                                                                                  \
  hipLaunchKernelGGL((fbk::k_fold_scatter<OPC, WRITE>), dim3(blocks), dim3(256), 0, st, slots, arena, rows, n_groups, k, \
                     fslots, farena, frows, arenaO, outSlots, outRuns, out_counts, recs)
  // n-way Intersect accumulates in registers (k_fold_n); Union / Xor / Difference scatter into an LDS accumulator
  // (k_fold_scatter).  (Until round 5 option fold_register ran every op through k_fold_n as the A/B cross-check of the scatter kernels.)
  switch (op) {
    case FBK_OP_AND: FBK_FOLD(0); break;
    case FBK_OP_OR: FBK_SCATTER(1); break;
    case FBK_OP_XOR: FBK_SCATTER(2); break;
    default: FBK_SCATTER(3); break;
  }
#undef FBK_SCATTER
#undef FBK_FOLD
}

int32_t fold_args_ok(int32_t op, uint64_t n_groups, uint32_t k) {
  if (op < 0 || op > 3) return fail(FBK_E_INVALID, "unknown set operation");
  if (n_groups > (1ull << 26)) return fail(FBK_E_INVALID, "too many groups in one call");
  if ((op == FBK_OP_AND || op == FBK_OP_ANDNOT) && k == 0 && n_groups)
    return fail(FBK_E_INVALID, "Intersect / Difference need at least one row per group");  // executor.go:5363, 2956
  return FBK_OK;
}

// output keys of a fold: those of the group's first row (a row without containers: 0)
void fold_output_keys(const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k, fbk_batch* o) {
  for (uint64_t gi = 0; gi < n_groups && k; ++gi) {
    uint64_t high = 0;
    (void)row_key_high(batch, rows[gi * k], &high);
    set_row_keys(o, gi, high);
  }
}

// What a fold keeps on the device: the rows of every group and, for the count form, the filter's row of every group (one
// allocation, one copy).  A one-shot call has it for its own duration; a prepared query between its runs, with the resolved
// records of the rows.
struct FoldPlan {
  int32_t op = 0;
  uint32_t k = 0;
  uint64_t n_groups = 0;
  const fbk_batch *batch = nullptr, *filter = nullptr;
  DevBuf rows;
  const uint32_t* dr[2] = {nullptr, nullptr};  // group rows and filter rows on the device
  bool encode = false;  // a prepared materialising fold: FBK_SETOP_OPTIMIZE, the fold encodes in its epilogue
  RowRecords recs;      // a prepared fold: the resolved records of dr[0]
};

// validates and uploads the row lists
int32_t fold_prepare(fbk_ctx* ctx, FoldPlan& P, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k,
                     const fbk_batch* filter, const uint32_t* rows_f) {
  P.op = op;
  P.k = k;
  P.n_groups = n_groups;
  P.batch = batch;
  P.filter = filter;
  if (int32_t rc = check_rows(rows, n_groups * k, batch->n_rows, "fold_n")) return rc;
  return upload_rows_multi(ctx, {{rows, n_groups * k, UINT32_MAX}, {rows_f, filter ? n_groups : 0, filter ? filter->n_rows : UINT32_MAX}}, P.rows, P.dr);
}

// launch only: the fold of every group into the cells of `o`, its cardinality added to d_counts[g].  encode: the fold kernels
// apply optimize() in their epilogue (the register-accumulating kernel — n-way Intersect — from wave 0's fragment) and d_runs is
// not used; otherwise bitmap cells, with their run counts where d_runs is not NULL.
void fold_launch(fbk_ctx* ctx, const FoldPlan& P, fbk_batch* o, bool encode, uint32_t* d_runs, u64* d_counts, const Slot* recs) {
  KernelSpan span(ctx);
  const uint32_t blocks = uint32_t(P.n_groups * fbk::kSlots);
  const fbk_batch* b = P.batch;
  if (encode)
    launch_fold<2>(P.op, blocks, ctx->stream, b->d_slots, b->d_arena, P.dr[0], P.n_groups, P.k, nullptr, nullptr, nullptr, o->d_arena, o->d_slots, nullptr, d_counts, recs);
  else
    launch_fold<1>(P.op, blocks, ctx->stream, b->d_slots, b->d_arena, P.dr[0], P.n_groups, P.k, nullptr, nullptr, nullptr, o->d_arena, o->d_slots, d_runs, d_counts, recs);
}

// a run of the prepared materialising fold: memset + ONE launch into the query's output batch, the cardinalities into d_counts
int32_t fold_enqueue(fbk_ctx* ctx, FoldPlan& P, fbk_batch* o, u64* d_counts) {
  const Slot* recs = nullptr;
  if (P.op != FBK_OP_AND)  // (the scatter kernels)
    if (int32_t rc = query_row_records(ctx, P.recs, P.batch, P.dr[0], P.n_groups, P.k, &recs)) return rc;
  HIP_TRY(hipMemsetAsync(d_counts, 0, P.n_groups * 8, ctx->stream));
  fold_launch(ctx, P, o, P.encode, nullptr, d_counts, recs);
  HIP_TRY(hipGetLastError());
  slots_rewritten(o);
  return FBK_OK;
}

// launch only: d_counts[g] (+)= |fold of group g (∩ filter row)|.  use_records: a prepared query's run, the scatter kernels
// read the resolved records of the rows
int32_t fold_n_icount_launch(fbk_ctx* ctx, FoldPlan& P, u64* d_counts, bool accumulate, bool use_records) {
  const Slot* recs = nullptr;
  if (use_records && P.op != FBK_OP_AND)
    if (int32_t rc = query_row_records(ctx, P.recs, P.batch, P.dr[0], P.n_groups, P.k, &recs)) return rc;
  if (!accumulate) HIP_TRY(hipMemsetAsync(d_counts, 0, P.n_groups * 8, ctx->stream));
  const FilterArgs f(P.filter, P.dr[1]);
  {
    KernelSpan span(ctx);
    launch_fold<0>(P.op, uint32_t(P.n_groups * fbk::kSlots), ctx->stream, P.batch->d_slots, P.batch->d_arena, P.dr[0], P.n_groups, P.k, f.slots, f.arena, f.rows,
                   nullptr, nullptr, nullptr, d_counts, recs);
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_fold_n(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k,
                   uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_batch || (n_groups && k && !rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  if (int32_t rc = fold_args_ok(op, n_groups, k)) return rc;
  *out_batch = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(batch))) return rc;  // h_slots / h_keys of an asynchronously produced input
  FoldPlan P;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_groups, n_groups, "fold_n")) return rc;
  if (int32_t rc = fold_prepare(ctx, P, op, batch, rows, n_groups, k, nullptr, nullptr)) return rc;
  fbk_batch* o = out.batch();
  fold_output_keys(batch, rows, n_groups, k, o);
  if (n_groups) {
    const bool enc = (flags & FBK_SETOP_OPTIMIZE) != 0;  // optimize() asked for: always inside the fold kernels
    fold_launch(ctx, P, o, enc, out.runs(), out.counts(), nullptr);
    if (enc) o->dense = false;
    if (int32_t rc = out.finish(flags & ~uint32_t(FBK_SETOP_OPTIMIZE), n_groups, out_counts, enc)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_fold_n_intersection_count(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows,
                                      uint64_t n_groups, uint32_t k, const fbk_batch* filter, const uint32_t* rows_f,
                                      uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_counts || (n_groups && ((k && !rows) || (filter && !rows_f))))
    return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = fold_args_ok(op, n_groups, k)) return rc;
  if (n_groups == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  FoldPlan P;
  DevBuf dcnt;
  if (int32_t rc = fold_prepare(ctx, P, op, batch, rows, n_groups, k, filter, rows_f)) return rc;
  HIP_TRY(dcnt.alloc(ctx, n_groups * 8));
  if (int32_t rc = fold_n_icount_launch(ctx, P, dcnt.as<u64>(), false, false)) return rc;
  D2H back(ctx);
  HIP_TRY(back.add(out_counts, dcnt.p, n_groups * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_union_n(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k,
                    uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  return fbk_fold_n(ctx, FBK_OP_OR, batch, rows, n_groups, k, flags, out_batch, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_union_n_intersection_count(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups,
                                       uint32_t k, const fbk_batch* filter, const uint32_t* rows_f,
                                       uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  return fbk_fold_n_intersection_count(ctx, FBK_OP_OR, batch, rows, n_groups, k, filter, rows_f, out_counts);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
