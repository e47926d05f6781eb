// fbk_query_api.inc — host side of the query-level entry points (included by fbk.hip).
// n-way fold (and the resolved row records its prepared form shares with the count matrix and TopN), Rows, Flip, Shift, compaction,
// and the BSI calls: Range, Sum / Min / Max and the range sums (one frame: BsiShardOperands + download_words), Add, Distinct.  The
// output batch of the materialising ones is a CellOutput (fbk_output.inc).  The GroupBy count matrix: fbk_count_matrix_api.inc.
// TopK / TopN: fbk_topn_api.inc.

namespace {

int32_t check_rows(const uint32_t* rows, uint64_t n, uint32_t limit, const char* what) {
  for (uint64_t i = 0; i < n; ++i)
    if (rows[i] >= limit) return fail(FBK_E_INVALID, std::string(what) + ": row index out of range");
  return FBK_OK;
}

using namespace fbk_bsi;  // BsiProg and the plane-program generators: fbk_bsi_prog.h


// Sum(Row(v op k), field = v) in one pass (k_bsi_range_sum_slot): the per-plane actions of rangeLT / rangeGT and their
// unsigned scans (fragment.go:1024-1208), with the SAME predicate rewrites as gen_lt / gen_gt / gen_ltu / gen_gtu above.
// false = one of the reference's special forms (predicate 0, saturated predicates, EQ / NEQ): the caller takes the
// two-pass path (range, then sum with the result as the filter).
bool plan_range_sum(int32_t op, uint64_t depth, int64_t pred, fbk::RangeSumPlan& pl) {
  bool gt, eq;
  switch (op) {
    case FBK_BSI_LT: gt = false, eq = false; break;
    case FBK_BSI_LTE: gt = false, eq = true; break;
    case FBK_BSI_GT: gt = true, eq = false; break;
    case FBK_BSI_GTE: gt = true, eq = true; break;
    default: return false;
  }
  if (gt && pred == -1 && !eq) pred = 0, eq = true;   // rangeGT :1116-1118
  if (!gt && pred == 1 && !eq) pred = 0, eq = true;   // rangeLT :1025-1027
  if (pred == 0 || depth == 0) return false;
  uint64_t up = abs_int64(pred);
  bool scan_gt;
  if (gt) {
    pl.scan_positive = pred >= 0;  // v > k >= 0: positives above k; v > k, k < 0: every positive + the negatives below |k|
    pl.take_other = pred < 0;
    scan_gt = pred >= 0;
  } else {
    pl.scan_positive = pred > 0;   // v < k, k > 0: every negative + the positives below k; k < 0: the negatives above |k|
    pl.take_other = pred > 0;
    scan_gt = pred < 0;
  }
  pl.depth = uint32_t(depth);
  std::memset(pl.action, 0, sizeof(pl.action));
  std::memset(pl.vhi, 0, sizeof(pl.vhi));
  auto above = [](uint64_t v, int i) { return v & ~((2ull << unsigned(i)) - 1); };  // the bits of v above bit i (i = 63: none)
  if (!scan_gt) {  // gen_ltu
    const uint64_t all_ones = go_shl(1, depth) - 1;
    if (bits_len64(up) > depth || up == all_ones) return false;
    if (eq) up++;
    const uint64_t p0 = up;
    for (int i = int(depth) - 1; i >= 0 && up > 0; --i) {
      if ((up >> unsigned(i)) & 1) {
        pl.action[i] = 4;  // matched |= remaining \ plane: these columns have 0 where the predicate has 1
        pl.vhi[i] = above(p0, i);
        up &= ~(1ull << unsigned(i));
      } else {
        pl.action[i] = 2;  // remaining \= plane
      }
    }
  } else {  // gen_gtu
    for (;;) {
      if (up == 0) return false;
      if (!eq && bits_len64(up) > depth) return false;
      if (eq) {
        up--;
        eq = false;
        continue;
      }
      break;
    }
    const uint64_t p0 = up;
    uint64_t px = up | go_shl(~0ull, depth);
    for (int i = int(depth) - 1; i >= 0 && px < ~0ull; --i) {
      if ((px >> unsigned(i)) & 1) {
        pl.action[i] = 1;  // remaining &= plane
      } else {
        pl.action[i] = 3;  // matched |= remaining & plane: 1 where the predicate has 0
        pl.vhi[i] = above(p0, i) | (1ull << unsigned(i));
        px |= 1ull << unsigned(i);
      }
    }
  }
  return true;
}

// Sum over lo <= v <= hi of the same field in one pass (k_bsi_between_sum_half): the schedule of the two scan lanes, from
// the definition of the comparison on sign-magnitude values (BetweenSumPlan).  false = two passes (lo >= hi, bounds
// beyond the field, the reference's EQ forms).
bool plan_between_sum(uint64_t depth, int64_t lo, int64_t hi, fbk::BetweenSumPlan& pl) {
  if (depth == 0 || depth > 64 || lo >= hi) return false;
  std::memset(&pl, 0, sizeof(pl));
  pl.depth = uint32_t(depth);
  const uint64_t all_ones = go_shl(1, depth) - 1;  // depth 64: ~0
  auto above = [](uint64_t v, int i) { return v & ~((2ull << unsigned(i)) - 1); };
  // "magnitude <= bound" from the top plane, on lane l
  auto le_scan = [&](int l, uint64_t bound, int from) {
    for (int i = from; i >= 0; --i) {
      if ((bound >> unsigned(i)) & 1) {
        pl.action[l][i] = 4;  // bit 0 where the bound has 1: below it whatever follows
        pl.vhi[l][i] = above(bound, i);
      } else {
        pl.action[l][i] = 2;  // bit 1 where the bound has 0: above it
      }
    }
    pl.vfin[l] = bound;
  };
  const uint64_t ulo = abs_int64(lo), uhi = abs_int64(hi);
  if (lo < 0 && hi >= 0) {  // the positives up to hi, the negatives up to |lo|
    pl.class_pos[0] = 1, pl.class_pos[1] = 0, pl.init_b = 1;
    if (uhi >= all_ones) pl.whole[0] = 1;
    else le_scan(0, uhi, int(depth) - 1);
    if (ulo >= all_ones) pl.whole[1] = 1;
    else le_scan(1, ulo, int(depth) - 1);
    return true;
  }
  uint64_t mn, mx;
  if (lo >= 0) pl.class_pos[0] = pl.class_pos[1] = 1, mn = ulo, mx = uhi;
  else pl.class_pos[0] = pl.class_pos[1] = 0, mn = uhi, mx = ulo;  // both negative: magnitudes |hi| .. |lo|
  if (mn > all_ones) return false;
  if (mx > all_ones) mx = all_ones;
  if (mn >= mx) return false;
  const int t = int(bits_len64(mn ^ mx)) - 1;  // the highest plane where the bounds differ: mn has 0, mx has 1
  for (int i = int(depth) - 1; i > t; --i) pl.action[0][i] = ((mn >> unsigned(i)) & 1) ? 1 : 2;  // the common prefix
  pl.split[t] = 1;
  for (int i = t - 1; i >= 0; --i) {  // lane 0: bit t = 0, ">= mn" on the planes below
    if ((mn >> unsigned(i)) & 1) {
      pl.action[0][i] = 1;
    } else {
      pl.action[0][i] = 3;
      pl.vhi[0][i] = above(mn, i) | (1ull << unsigned(i));
    }
  }
  pl.vfin[0] = mn;
  le_scan(1, mx, t - 1);  // lane 1: bit t = 1, "<= mx" on the planes below
  return true;
}


// The filter operand of a launch: its descriptors, its arena and its row list on the device; no filter: all NULL.
struct FilterArgs {
  const Slot* slots = nullptr;
  const uint8_t* arena = nullptr;
  const uint32_t* rows = nullptr;
  FilterArgs(const fbk_batch* filter, const uint32_t* d_rows) {
    if (filter) slots = filter->d_slots, arena = filter->d_arena, rows = d_rows;
  }
};

// What a prepared fold, count matrix (TopK shape) or TopN keeps of its field's rows: the descriptors of every (group / shard, slot)
// side by side (k_resolve_rows), resolved on the first run and again whenever the batch's descriptors have been rewritten since
// (nothing above 1 GiB).
struct RowRecords {
  DevBuf buf;
  uint64_t version = ~0ull;
};

// The resolved records of rows d_rows [n_units][n_per] of `a` for this run (nullptr: not used).
int32_t query_row_records(fbk_ctx* ctx, RowRecords& r, const fbk_batch* a, const uint32_t* d_rows, uint64_t n_units, uint32_t n_per, const Slot** out) {
  *out = nullptr;
  const uint64_t n = n_units * fbk::kSlots * n_per;
  if (n == 0 || n * sizeof(Slot) > (1ull << 30)) return FBK_OK;
  if (!r.buf.p) {
    if (r.buf.alloc(ctx, n * sizeof(Slot)) != hipSuccess) {
      (void)hipGetLastError();
      return FBK_OK;  // (no memory for the records: the kernels gather the descriptors themselves)
    }
    r.version = ~0ull;
  }
  if (r.version != a->version) {
    hipLaunchKernelGGL(fbk::k_resolve_rows, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, a->d_slots, d_rows, n_units, n_per, r.buf.as<Slot>());
    HIP_TRY(hipGetLastError());
    r.version = a->version;
  }
  *out = r.buf.as<Slot>();
  return FBK_OK;
}

int32_t run_bsi_program(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint64_t n_shards,
                        uint64_t bit_depth, const BsiProg& prog, uint32_t flags, fbk_batch** out_batch,
                        uint64_t* out_counts) {
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  DevBuf dbase, dprog;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_shards, n_shards, "bsi range")) return rc;
  if (int32_t rc = upload_rows(ctx, base_rows, n_shards, batch->n_rows, dbase)) return rc;
  hipError_t e = dprog.alloc(ctx, std::max<size_t>(prog.v.size(), 1) * 4);
  if (e == hipSuccess && !prog.v.empty())
    e = hipMemcpyAsync(dprog.p, prog.v.data(), prog.v.size() * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? FBK_E_NOMEM : FBK_E_HIP, std::string("bsi range: ") + hipGetErrorString(e));
  }
  // optimize() asked for: applied by the kernel itself (option setop_direct_encode = 2; otherwise the separate re-encode pass)
  const bool enc = (flags & FBK_SETOP_OPTIMIZE) && ctx->opt.setop_direct_encode == 2;
  if (n_shards) {
    {
      KernelSpan span(ctx);
      // one wavefront per (shard, slot)
      hipLaunchKernelGGL(fbk::k_bsi_range_slot, dim3(uint32_t(n_shards * fbk::kSlots)), dim3(64), 0, ctx->stream,
                         batch->d_slots, batch->d_arena, dbase.as<uint32_t>(), uint32_t(n_shards), dprog.as<uint32_t>(),
                         uint32_t(prog.v.size()), uint32_t(bit_depth + 2), out.batch()->d_arena, out.batch()->d_slots, out.runs(), out.counts(), uint32_t(enc));
    }
    if (int32_t rc = out.finish(enc ? (flags & ~uint32_t(FBK_SETOP_OPTIMIZE)) : flags, n_shards, out_counts, enc)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
}

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

// The key rule of the materialising row operations: an output row's keys are (high | slot), high = the high key bits of the
// first non-nil container of its source row.  false: the row has no container.
bool row_key_high(const fbk_batch* batch, uint32_t row, uint64_t* high) {
  for (int s = 0; s < fbk::kSlots; ++s) {
    const uint64_t is = uint64_t(row) * fbk::kSlots + s;
    if (fbk::slot_type(batch->h_slots[is]) != fbk::kTypeNil) {
      *high = batch->h_keys[is] & ~15ull;
      return true;
    }
  }
  return false;
}
void set_row_keys(fbk_batch* o, uint64_t row, uint64_t high) {
  for (int s = 0; s < fbk::kSlots; ++s) o->h_keys[row * fbk::kSlots + s] = high | uint64_t(s);
}

// output keys of a fold: those of the group's first row (a row without containers: 0)
void fold_output_keys(const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k, fbk_batch* o) {
  for (uint64_t gi = 0; gi < n_groups && k; ++gi) {
    uint64_t high = 0;
    (void)row_key_high(batch, rows[gi * k], &high);
    set_row_keys(o, gi, high);
  }
}

int32_t fold_n_locked(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k,
                      uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts) {
  if (int32_t rc = check_rows(rows, n_groups * k, batch->n_rows, "fold_n")) return rc;
  if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(batch))) return rc;  // h_slots / h_keys of an asynchronously produced input
  DevBuf drows;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_groups, n_groups, "fold_n")) return rc;
  fbk_batch* o = out.batch();
  fold_output_keys(batch, rows, n_groups, k, o);
  if (int32_t rc = upload_rows(ctx, rows, n_groups * k, batch->n_rows, drows)) return rc;
  if (n_groups) {
    // optimize() asked for: the fold kernels encode in their epilogue (the register-accumulating kernel — n-way Intersect —
    // from wave 0's fragment)
    const bool enc = (flags & FBK_SETOP_OPTIMIZE) != 0;
    {
      KernelSpan span(ctx);
      if (enc) {
        launch_fold<2>(op, uint32_t(n_groups * fbk::kSlots), ctx->stream, batch->d_slots, batch->d_arena, drows.as<uint32_t>(), n_groups, k, nullptr, nullptr,
                       nullptr, o->d_arena, o->d_slots, nullptr, out.counts());
        flags &= ~uint32_t(FBK_SETOP_OPTIMIZE);
        o->dense = false;
      } else {
        launch_fold<1>(op, uint32_t(n_groups * fbk::kSlots), ctx->stream, batch->d_slots, batch->d_arena, drows.as<uint32_t>(), n_groups, k, nullptr, nullptr,
                       nullptr, o->d_arena, o->d_slots, out.runs(), out.counts());
      }
    }
    if (int32_t rc = out.finish(flags, n_groups, out_counts, enc)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
}

int32_t fold_n_icount_upload_rows(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k,
                                  const fbk_batch* filter, const uint32_t* rows_f, DevBuf& drows, const uint32_t** dr) {
  if (int32_t rc = check_rows(rows, n_groups * k, batch->n_rows, "fold_n")) return rc;
  return upload_rows_multi(ctx, {{rows, n_groups * k, UINT32_MAX}, {rows_f, filter ? n_groups : 0, filter ? filter->n_rows : UINT32_MAX}}, drows, dr);
}

// launch only: d_counts[g] (+)= |fold of group g (∩ filter row)|; dr = {group rows, filter rows} on the device
int32_t fold_n_icount_launch(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* const* dr, uint64_t n_groups, uint32_t k,
                             const fbk_batch* filter, u64* d_counts, bool accumulate, const Slot* recs = nullptr) {
  if (!accumulate) HIP_TRY(hipMemsetAsync(d_counts, 0, n_groups * 8, ctx->stream));
  const FilterArgs f(filter, dr[1]);
  {
    KernelSpan span(ctx);
    launch_fold<0>(op, uint32_t(n_groups * fbk::kSlots), ctx->stream, batch->d_slots, batch->d_arena, dr[0], n_groups, k,
                       f.slots, f.arena, f.rows, nullptr, nullptr, nullptr, d_counts, recs);
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

int32_t fold_n_icount_locked(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups,
                             uint32_t k, const fbk_batch* filter, const uint32_t* rows_f, uint64_t* out_counts) {
  DevBuf drows, dcnt;
  const uint32_t* dr[2] = {nullptr, nullptr};  // group rows and filter rows: one upload
  if (int32_t rc = fold_n_icount_upload_rows(ctx, batch, rows, n_groups, k, filter, rows_f, drows, dr)) return rc;
  HIP_TRY(dcnt.alloc(ctx, n_groups * 8));
  if (int32_t rc = fold_n_icount_launch(ctx, op, batch, dr, n_groups, k, filter, dcnt.as<u64>(), false)) return rc;
  D2H back(ctx);
  HIP_TRY(back.add(out_counts, dcnt.p, n_groups * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
}

int32_t fold_args_ok(int32_t op, uint64_t n_groups, uint32_t k) {
  if (op < 0 || op > 3) return fail(FBK_E_INVALID, "unknown set operation");
  if (n_groups > (1ull << 26)) return fail(FBK_E_INVALID, "too many groups in one call");
  if ((op == FBK_OP_AND || op == FBK_OP_ANDNOT) && k == 0 && n_groups)
    return fail(FBK_E_INVALID, "Intersect / Difference need at least one row per group");  // executor.go:5363, 2956
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
  return fold_n_locked(ctx, op, batch, rows, n_groups, k, flags, out_batch, out_counts);
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
  return fold_n_icount_locked(ctx, op, batch, rows, n_groups, k, filter, rows_f, out_counts);
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

int32_t fbk_batch_compact(fbk_ctx* ctx, fbk_batch* batch, uint64_t* out_arena_bytes) try {
  FBK_ENTER(ctx);
  if (!batch) return fail(FBK_E_INVALID, "batch is NULL");
  if (!ctx) ctx = batch->ctx;
  // (the new arena comes from ctx's pool and the copy runs on ctx's stream: another context's batch would leave stale pool entries
  // behind and race its owner's stream)
  if (ctx != batch->ctx) return fail(FBK_E_INVALID, "compact: the batch belongs to another context (compact it through its own)");
  if (batch->borrowed) return fail(FBK_E_INVALID, "compact: the batch is the output of a plan / prepared query (rewritten in place by its next run): compact a batch you own");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (!batch->dense) {
    if (int32_t rc = compact_cells(ctx, batch)) return rc;
  }
  if (out_arena_bytes) *out_arena_bytes = batch->arena_bytes;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_batch_memory(fbk_ctx* ctx, const fbk_batch* batch, uint64_t* out_arena_bytes, uint64_t* out_shadow_bytes, int32_t* out_shadow_state) try {
  FBK_ENTER(ctx);
  if (!batch) return fail(FBK_E_INVALID, "batch is NULL");
  std::lock_guard<std::mutex> g(batch->win_mu);
  if (out_arena_bytes) *out_arena_bytes = batch->arena_bytes;
  if (out_shadow_bytes) *out_shadow_bytes = batch->shadow_bytes;
  if (out_shadow_state) *out_shadow_state = batch->shadow_state;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_rows(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, const uint64_t* row_ids, uint64_t n_rows, uint64_t column,
                 uint64_t limit, uint32_t* out_idx, uint64_t cap, uint64_t* out_n) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_n || (n_rows && !rows) || (cap && !out_idx)) return fail(FBK_E_INVALID, "NULL argument");
  const bool need_ids = column != FBK_NO_COLUMN && limit != 0;  // the limit filter's count depends on which rows follow each other directly
  if (need_ids && n_rows && !row_ids) return fail(FBK_E_INVALID, "rows: a column together with a limit needs row_ids");
  if (row_ids)
    for (uint64_t i = 1; i < n_rows; ++i)
      if (row_ids[i - 1] >= row_ids[i]) return fail(FBK_E_INVALID, "rows: row_ids must be strictly ascending");
  if (column != FBK_NO_COLUMN && column >= (uint64_t(fbk::kSlots) << 16)) return fail(FBK_E_INVALID, "rows: column outside the shard (0 .. 2^20 - 1)");
  if (n_rows > (1ull << 31) - 1) return fail(FBK_E_INVALID, "too many rows in one call");
  *out_n = 0;
  if (n_rows == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = check_rows(rows, n_rows, batch->n_rows, "rows")) return rc;
  DevBuf drows, dids, dflags, drank, dkeep, dsel, dnum, dtmp;
  if (int32_t rc = upload_rows(ctx, rows, n_rows, UINT32_MAX, drows)) return rc;
  if (need_ids) {
    HIP_TRY(dids.alloc(ctx, n_rows * 8));
    HIP_TRY(hipMemcpyAsync(dids.p, row_ids, n_rows * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(dflags.alloc(ctx, n_rows));
  HIP_TRY(dkeep.alloc(ctx, n_rows));
  HIP_TRY(dsel.alloc(ctx, n_rows * 4));
  HIP_TRY(dnum.alloc(ctx, 8));
  const int n = int(n_rows);
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_rows_flags, dim3(uint32_t((n_rows * fbk::kSlots + 255) / 256)), dim3(256), 0, ctx->stream, batch->d_slots, batch->d_arena,
                       drows.as<uint32_t>(), n_rows, column, dflags.as<uint8_t>());
  }
  size_t t1 = 0, t2 = 0;
  hipcub::CountingInputIterator<uint32_t> iota(0);
  hipcub::TransformInputIterator<uint32_t, fbk::RowCounted, hipcub::CountingInputIterator<uint32_t>> ne(
      iota, fbk::RowCounted{dflags.as<uint8_t>(), need_ids ? dids.as<uint64_t>() : (const uint64_t*)nullptr});
  if (limit) {
    HIP_TRY(drank.alloc(ctx, n_rows * 4));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, ne, drank.as<uint32_t>(), n, ctx->stream));
  }
  HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, t2, iota, dkeep.as<uint8_t>(), dsel.as<uint32_t>(), dnum.as<uint32_t>(), n, ctx->stream));
  HIP_TRY(dtmp.alloc(ctx, std::max<size_t>(std::max(t1, t2), 16)));
  if (limit) {
    size_t tb = std::max(t1, t2);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(dtmp.p, tb, ne, drank.as<uint32_t>(), n, ctx->stream));
  }
  hipLaunchKernelGGL(fbk::k_rows_select, dim3(uint32_t((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, dflags.as<uint8_t>(),
                     limit ? drank.as<uint32_t>() : (const uint32_t*)nullptr, n_rows, limit, dkeep.as<uint8_t>());
  {
    size_t tb = std::max(t1, t2);
    HIP_TRY(hipcub::DeviceSelect::Flagged(dtmp.p, tb, iota, dkeep.as<uint8_t>(), dsel.as<uint32_t>(), dnum.as<uint32_t>(), n, ctx->stream));
  }
  HIP_TRY(hipGetLastError());
  uint32_t n_sel = 0;
  HIP_TRY(hipMemcpyAsync(&n_sel, dnum.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *out_n = n_sel;
  if (n_sel > cap) return fail(FBK_E_CAPACITY, "rows: " + std::to_string(n_sel) + " rows match, buffer holds " + std::to_string(cap));
  if (n_sel) {
    HIP_TRY(hipMemcpyAsync(out_idx, dsel.p, uint64_t(n_sel) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_flip(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n_rows, uint64_t start, uint64_t end, uint32_t flags,
                 fbk_batch** out_batch, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_batch || (n_rows && !rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  const uint64_t width = uint64_t(fbk::kSlots) << 16;
  if (start > end || end >= width) return fail(FBK_E_INVALID, "flip: need 0 <= start <= end < 2^20");  // roaring.go:2771 panics on start > end
  if (n_rows > (1ull << 27)) return fail(FBK_E_INVALID, "too many rows in one call");
  *out_batch = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_batch* bb = const_cast<fbk_batch*>(batch);
  if (int32_t rc = refresh_slots(bb)) return rc;
  if (int32_t rc = check_rows(rows, n_rows, batch->n_rows, "flip")) return rc;
  DevBuf drows;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_rows, n_rows, "flip")) return rc;
  fbk_batch* o = out.batch();
  for (uint64_t i = 0; i < n_rows; ++i) {  // keys: those of the flipped row (a row without containers: row ordinal << 4)
    uint64_t high = i << 4;
    (void)row_key_high(batch, rows[i], &high);
    set_row_keys(o, i, high);
  }
  if (int32_t rc = upload_rows(ctx, rows, n_rows, UINT32_MAX, drows)) return rc;
  const bool enc = (flags & FBK_SETOP_OPTIMIZE) && ctx->opt.setop_direct_encode == 2;  // optimize() inside the kernel
  if (n_rows) {
    hipLaunchKernelGGL(fbk::k_flip, dim3(uint32_t((n_rows * fbk::kSlots + 3) / 4)), dim3(256), 0, ctx->stream, batch->d_slots, batch->d_arena,
                       drows.as<uint32_t>(), n_rows, uint32_t(start), uint32_t(end), o->d_arena, o->d_slots, out.runs(), out.counts(), uint32_t(enc));
    if (int32_t rc = out.finish(enc ? (flags & ~uint32_t(FBK_SETOP_OPTIMIZE)) : flags, n_rows, out_counts, enc)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"

namespace {

// ---- the per-shard BSI aggregates (Sum, Min / Max, the range sums): one frame ------------------------------------------
// check the arguments, take the lock, upload the operands (BsiShardOperands), launch into W words per shard, download them
// (download_words), fold them on the host.

// pointers and depth; the outputs may be NULL only without shards (then the call returns FBK_OK right after this)
int32_t bsi_aggregate_args_ok(const fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                              const fbk_batch* filter, const uint32_t* rows_f, const void* out_a, const void* out_b) {
  if (!ctx || !batch || (n_shards && (!base_rows || !out_a || !out_b)) || (filter && n_shards && !rows_f))
    return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  return FBK_OK;
}

// base_rows and the filter's rows on the device (two copies, in this order).  The caller holds ctx->mu and has set the device.
struct BsiShardOperands {
  DevBuf dbase, drf;
  int32_t upload(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth, const fbk_batch* filter,
                 const uint32_t* rows_f) {
    if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
    if (int32_t rc = upload_rows(ctx, base_rows, n_shards, batch->n_rows, dbase)) return rc;
    if (filter)
      if (int32_t rc = upload_rows(ctx, rows_f, n_shards, filter->n_rows, drf)) return rc;
    return FBK_OK;
  }
  const uint32_t* base() { return dbase.as<uint32_t>(); }
  const uint32_t* filter_rows() { return drf.as<uint32_t>(); }  // NULL without a filter
};

// the words a launch left in `d`, on the host once this returns (one synchronisation)
int32_t download_words(fbk_ctx* ctx, DevBuf& d, uint64_t n_words, std::vector<u64>& h) {
  h.resize(n_words);
  D2H back(ctx);
  HIP_TRY(back.add(h.data(), d.p, n_words * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
}

// The two-pass form of a range sum, the reference's own two steps: the range as a Row (`rng`, owned from here on: freed on every
// path), then fragment.sum with that Row (∩ the caller's filter) as the filter.  Called WITHOUT the context's lock: the public
// entry points used here take it themselves.
int32_t bsi_sum_over_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth, fbk_batch* rng,
                           const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums, uint64_t* out_counts) {
  struct Owned {
    fbk_ctx* ctx;
    fbk_batch* b;
    ~Owned() { (void)fbk_batch_free(ctx, b); }
  } row{ctx, rng};
  std::vector<uint32_t> ident(n_shards);
  for (uint32_t s = 0; s < n_shards; ++s) ident[s] = s;
  if (filter) {
    fbk_batch* both = nullptr;
    const int32_t rc = fbk_setop(ctx, FBK_OP_AND, row.b, ident.data(), filter, rows_f, n_shards, 0, &both, nullptr);
    (void)fbk_batch_free(ctx, row.b);
    row.b = both;  // (NULL after a failure)
    if (rc) return rc;
  }
  return fbk_bsi_sum(ctx, batch, base_rows, n_shards, bit_depth, row.b, ident.data(), out_sums, out_counts);
}

// launch only: d3[s] = {psum, nsum, count} of shard s (zeroed here)
int32_t bsi_sum_launch(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* d_base, uint32_t n_shards, uint32_t bit_depth, const fbk_batch* filter,
                       const uint32_t* d_rf, u64* d3) {
  HIP_TRY(hipMemsetAsync(d3, 0, uint64_t(n_shards) * 24, ctx->stream));
  const FilterArgs f(filter, d_rf);
  {
    KernelSpan span(ctx);
    // one wavefront per (shard, slot)
    hipLaunchKernelGGL(fbk::k_bsi_sum_slot, dim3(uint32_t(uint64_t(n_shards) * fbk::kSlots)), dim3(64), 0, ctx->stream,
                       batch->d_slots, batch->d_arena, d_base, n_shards, bit_depth, f.slots, f.arena, d_rf, d3);
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// launch only: d4[s] = {scanned class magnitudes, other class magnitudes, count scanned, count other} (zeroed here);
// d_plan = the RangeSumPlan on the device
int32_t bsi_range_sum_launch(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* d_base, uint32_t n_shards, const fbk::RangeSumPlan& pl,
                             const fbk::RangeSumPlan* d_plan, const fbk_batch* filter, const uint32_t* d_rf, u64* d4) {
  HIP_TRY(hipMemsetAsync(d4, 0, uint64_t(n_shards) * 32, ctx->stream));
  const FilterArgs f(filter, d_rf);
  {
    KernelSpan span(ctx);
    if (batch->dense) {  // half a container per wavefront, three planes in flight (four measured equal in round 3 and were dropped in round 5)
      auto kern = pl.take_other ? fbk::k_bsi_range_sum_half<true, 3> : fbk::k_bsi_range_sum_half<false, 3>;
      hipLaunchKernelGGL(kern, dim3(uint32_t(uint64_t(n_shards) * fbk::kSlots * 2)), dim3(64), 0, ctx->stream, batch->d_arena, d_base, n_shards, d_plan,
                         f.slots, f.arena, d_rf, d4);
    } else {
      auto kern = pl.take_other ? fbk::k_bsi_range_sum_slot<true> : fbk::k_bsi_range_sum_slot<false>;
      hipLaunchKernelGGL(kern, dim3(uint32_t(uint64_t(n_shards) * fbk::kSlots)), dim3(64), 0, ctx->stream, batch->d_slots, batch->d_arena, d_base,
                         n_shards, d_plan, f.slots, f.arena, d_rf, d4);
    }
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_bsi_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums,
                    uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_sums, out_counts)) return rc;
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  BsiShardOperands ops;
  if (int32_t rc = ops.upload(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f)) return rc;
  DevBuf d3;
  HIP_TRY(d3.alloc(ctx, uint64_t(n_shards) * 24));
  if (int32_t rc = bsi_sum_launch(ctx, batch, ops.base(), n_shards, bit_depth, filter, ops.filter_rows(), d3.as<u64>())) return rc;
  std::vector<u64> h3;
  if (int32_t rc = download_words(ctx, d3, uint64_t(n_shards) * 3, h3)) return rc;
  for (uint32_t s = 0; s < n_shards; ++s) {
    // Total(): int64(psum) - int64(nsum) (roaring/filter.go:1106-1108)
    out_sums[s] = int64_t(uint64_t(h3[s * 3 + 0]) - uint64_t(h3[s * 3 + 1]));
    out_counts[s] = h3[s * 3 + 2];
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

// The host fold of k_bsi_minmax_slot's records (also k_expr_agg_slot's): h2[(s * 16 + slot) * 2] = {magnitude, count | scan flag}
// -> Min (mode 0) / Max (mode 1) of shard s and the number of columns that hold it; (0, 0) where nothing qualifies.
static void bsi_minmax_fold(const u64* h2, uint32_t n_shards, uint32_t mode, int64_t* out_vals, uint64_t* out_counts) {
  for (uint32_t s = 0; s < n_shards; ++s) {
    // fragment.min (fragment.go:754-779): negatives present => -(maxUnsigned over them), else
    // minUnsigned over everything considered; fragment.max (:803-830) with positives.  "present" is
    // the OR over the slots; maxUnsigned / minUnsigned over the row = max / min of the slots' values.
    bool decided = false;  // some slot holds columns of the deciding sign
    for (int sl = 0; sl < fbk::kSlots; ++sl)
      if (h2[(uint64_t(s) * fbk::kSlots + sl) * 2 + 1] >> 63) decided = true;
    uint64_t mag = 0, cnt = 0;
    for (int sl = 0; sl < fbk::kSlots; ++sl) {
      const uint64_t v = h2[(uint64_t(s) * fbk::kSlots + sl) * 2];
      const uint64_t cw = h2[(uint64_t(s) * fbk::kSlots + sl) * 2 + 1];
      const uint64_t c = cw & ~(1ull << 63);
      if (c == 0 || bool(cw >> 63) != decided) continue;  // empty slot / a slot without columns of the deciding sign
      if (cnt == 0 || (decided ? v > mag : v < mag)) {
        mag = v;
        cnt = c;
      } else if (v == mag) {
        cnt += c;
      }
    }
    const bool negate = decided ? (mode == 0) : (mode == 1);
    const int64_t best = int64_t(negate ? (0ull - mag) : mag);
    out_vals[s] = cnt ? best : 0;
    out_counts[s] = cnt;
  }
}

// Min (mode 0) / Max (mode 1) per shard.  The caller holds ctx->mu, has set the device and checked the pointers; n_shards != 0.
// Also fbk_bsi_distinct_rows' window when arithmetic does not bound it.
static int32_t bsi_minmax_locked(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                                 uint32_t bit_depth, uint32_t mode, const fbk_batch* filter, const uint32_t* rows_f,
                                 int64_t* out_vals, uint64_t* out_counts) {
  BsiShardOperands ops;
  if (int32_t rc = ops.upload(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f)) return rc;
  // one wavefront per (shard, slot), folded per shard on the host: min over a shard = the smallest of
  // its slots' minima, its count = the sum over the slots that reach it (max alike)
  const uint64_t n_out = uint64_t(n_shards) * fbk::kSlots;
  DevBuf d2;
  HIP_TRY(d2.alloc(ctx, n_out * 16));
  const FilterArgs f(filter, ops.filter_rows());
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_bsi_minmax_slot, dim3(uint32_t(n_out)), dim3(64), 0, ctx->stream, batch->d_slots, batch->d_arena,
                       ops.base(), n_shards, bit_depth, mode, f.slots, f.arena, f.rows, d2.as<u64>());
  }
  HIP_TRY(hipGetLastError());
  std::vector<u64> h2;
  if (int32_t rc = download_words(ctx, d2, n_out * 2, h2)) return rc;
  bsi_minmax_fold(h2.data(), n_shards, mode, out_vals, out_counts);
  return FBK_OK;
}

static int32_t bsi_minmax(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                          uint32_t bit_depth, uint32_t mode, const fbk_batch* filter, const uint32_t* rows_f,
                          int64_t* out_vals, uint64_t* out_counts) {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_vals, out_counts)) return rc;
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return bsi_minmax_locked(ctx, batch, base_rows, n_shards, bit_depth, mode, filter, rows_f, out_vals, out_counts);
}

int32_t fbk_bsi_min(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_vals,
                    uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  return bsi_minmax(ctx, batch, base_rows, n_shards, bit_depth, 0, filter, rows_f, out_vals, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_max(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_vals,
                    uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  return bsi_minmax(ctx, batch, base_rows, n_shards, bit_depth, 1, filter, rows_f, out_vals, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_add(fbk_ctx* ctx, const fbk_batch* x, const uint32_t* rows_x, uint32_t depth_x, const fbk_batch* y,
                    const uint32_t* rows_y, uint32_t depth_y, uint64_t n_groups, uint32_t flags, fbk_batch** out_batch) try {
  FBK_ENTER(ctx);
  if (!ctx || !x || !y || !out_batch || (n_groups && ((depth_x && !rows_x) || (depth_y && !rows_y))))
    return fail(FBK_E_INVALID, "NULL argument");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  if (depth_x > 64 || depth_y > 64) return fail(FBK_E_INVALID, "bsi_add: at most 64 planes per operand");
  *out_batch = nullptr;
  const uint32_t D = std::max(depth_x, depth_y);
  if (n_groups * (D + 1) > (1ull << 27)) return fail(FBK_E_INVALID, "too many groups in one call");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  DevBuf drx, dry;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_groups * (D + 1), 0, "bsi_add")) return rc;
  if (int32_t rc = upload_rows(ctx, rows_x, n_groups * depth_x, x->n_rows, drx)) return rc;
  if (int32_t rc = upload_rows(ctx, rows_y, n_groups * depth_y, y->n_rows, dry)) return rc;
  if (n_groups) {
    hipLaunchKernelGGL(fbk::k_bsi_add, dim3(uint32_t(n_groups * fbk::kSlots)), dim3(256), 0, ctx->stream, x->d_slots, x->d_arena,
                       drx.as<uint32_t>(), depth_x, y->d_slots, y->d_arena, dry.as<uint32_t>(), depth_y, n_groups, out.batch()->d_arena,
                       out.batch()->d_slots, out.runs());
    if (int32_t rc = out.finish(flags, 0, nullptr)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_shift(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, const uint32_t* carry_rows, uint64_t n_rows,
                  uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_batch || (n_rows && !rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  if (n_rows > (1ull << 27)) return fail(FBK_E_INVALID, "too many rows in one call");
  *out_batch = nullptr;
  for (uint64_t i = 0; i < n_rows; ++i) {
    if (rows[i] != FBK_NO_ROW && rows[i] >= batch->n_rows) return fail(FBK_E_INVALID, "shift: row index out of range");
    if (carry_rows && carry_rows[i] != FBK_NO_ROW && carry_rows[i] >= batch->n_rows)
      return fail(FBK_E_INVALID, "shift: carry row index out of range");
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_batch* bb = const_cast<fbk_batch*>(batch);
  if (int32_t rc = refresh_slots(bb)) return rc;
  DevBuf drows, dcarry;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_rows, n_rows, "shift")) return rc;
  fbk_batch* o = out.batch();
  // output keys: the keys of the shifted row (of the carry row's successor shard for a row that
  // exists only because a bit was carried into it)
  for (uint64_t i = 0; i < n_rows; ++i) {
    uint64_t high = 0;
    if (rows[i] == FBK_NO_ROW || !row_key_high(batch, rows[i], &high)) {
      if (carry_rows && carry_rows[i] != FBK_NO_ROW && row_key_high(batch, carry_rows[i], &high)) high += 16;
    }
    set_row_keys(o, i, high);
  }
  if (int32_t rc = upload_rows(ctx, rows, n_rows, UINT32_MAX, drows)) return rc;  // validated above (FBK_NO_ROW is legal here)
  if (carry_rows)
    if (int32_t rc = upload_rows(ctx, carry_rows, n_rows, UINT32_MAX, dcarry)) return rc;
  const bool enc = (flags & FBK_SETOP_OPTIMIZE) && ctx->opt.setop_direct_encode == 2;  // optimize() inside the kernel
  if (n_rows) {
    hipLaunchKernelGGL(fbk::k_shift, dim3(uint32_t((n_rows * fbk::kSlots + 3) / 4)), dim3(256), 0, ctx->stream, batch->d_slots,
                       batch->d_arena, drows.as<uint32_t>(), carry_rows ? dcarry.as<uint32_t>() : (const uint32_t*)nullptr, n_rows,
                       o->d_arena, o->d_slots, out.runs(), out.counts(), uint32_t(enc));
    if (int32_t rc = out.finish(enc ? (flags & ~uint32_t(FBK_SETOP_OPTIMIZE)) : flags, n_rows, out_counts, enc)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

// blocks per (shard, slot) of k_bsi_values: enough of them for ~8 blocks per CU (each covers 16 / split rounds of 1024 columns per wave)
static uint32_t bsi_values_split(uint32_t n_shards) {
  uint32_t split = 1;
  while (split < 16 && uint64_t(n_shards) * fbk::kSlots * split < 2048) split <<= 1;
  return split;
}

// The device half of fbk_bsi_distinct: the sorted distinct values of exists ∩ filter over the shards, left on the device in `duniq`
// (n_unique of them).  Also the first stage of fbk_count_matrix_distinct.  The caller holds ctx->mu and has checked the pointers.
static int32_t bsi_distinct_device(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                                   const fbk_batch* filter, const uint32_t* rows_f, DevBuf& duniq, u64& n_unique) {
  n_unique = 0;
  fbk_batch* bb = const_cast<fbk_batch*>(batch);
  if (int32_t rc = refresh_slots(bb)) return rc;
  uint64_t upper = 0;  // at most one value per existing column
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  for (uint32_t s = 0; s < n_shards; ++s)
    for (int sl = 0; sl < fbk::kSlots; ++sl) upper += fbk::slot_n(batch->h_slots[uint64_t(base_rows[s]) * fbk::kSlots + sl]);
  if (filter)
    if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "bsi_distinct filter")) return rc;
  if (upper == 0) return FBK_OK;
  if (upper >= (1ull << 31)) return fail(FBK_E_INVALID, "bsi_distinct: more than 2^31 values in one call (split the shard list)");
  DevBuf dvals, dsorted, dcur, dtmp, dbase, dcounts;
  HIP_TRY(dvals.alloc(ctx, upper * 8));
  HIP_TRY(dcur.alloc(ctx, 32));  // [0] the running total of values (k_bsi_cell_scan's carry), [1] the number of distinct values, [2] (uint32) the count-mismatch flag
  HIP_TRY(hipMemsetAsync(dcur.p, 0, 32, ctx->stream));
  HIP_TRY(dbase.alloc(ctx, (uint64_t(n_shards) * fbk::kSlots + 1) * 8));
  if (filter) HIP_TRY(dcounts.alloc(ctx, uint64_t(n_shards) * fbk::kSlots * 4));
  uint32_t* d_flag = reinterpret_cast<uint32_t*>(dcur.as<u64>() + 2);
  // Array / run containers among the planes or in the filter: both are densified, a chunk of shards at a time (<= ~4 GiB).
  const bool densify = !batch->dense || (filter && !filter->dense);
  const uint32_t rps = bit_depth + 2;  // rows per shard
  const uint32_t chunk = densify ? uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(n_shards, (4ull << 30) / ((rps + 1) * kDenseRowBytes)))) : n_shards;
  DenseOperands ops;
  const int kS = ops.add(batch, base_rows, rps, true, densify), kF = ops.add(filter, rows_f, 1, false, densify);
  if (int32_t rc = ops.upload(ctx, n_shards, chunk)) return rc;
  // Where a cell's values go is known before the transpose runs (k_bsi_cell_scan): without a filter the stored cardinalities of the
  // exists row are the counts, with one a count pass over exists ∩ filter comes first.
  for (uint32_t s0 = 0; s0 < n_shards; s0 += chunk) {
    const uint32_t ns = std::min(chunk, n_shards - s0);
    ops.densify(ctx, s0, ns);
    const DenseView S = ops.view(kS, s0), F = ops.view(kF, s0);
    u64* cb = dbase.as<u64>() + uint64_t(s0) * fbk::kSlots;  // (the chunk's last entry is the next chunk's first: the same number)
    if (filter)
      hipLaunchKernelGGL(fbk::k_bsi_cell_counts, dim3((ns * fbk::kSlots + 3) / 4), dim3(256), 0, ctx->stream, S.arena, S.rows, ns, F.arena, F.rows,
                         dcounts.as<uint32_t>());
    hipLaunchKernelGGL(fbk::k_bsi_cell_scan, dim3(1), dim3(1024), 0, ctx->stream, batch->d_slots, ops.rows(kS, s0),
                       filter ? dcounts.as<uint32_t>() : (const uint32_t*)nullptr, ns * fbk::kSlots, cb, dcur.as<u64>());
    hipLaunchKernelGGL(fbk::k_bsi_values, dim3(ns * fbk::kSlots * bsi_values_split(ns)), dim3(256), 0, ctx->stream, S.arena, S.rows, ns, bit_depth, F.arena, F.rows,
                       dvals.as<long long>(), u64(upper), cb, d_flag, bsi_values_split(ns));
  }
  HIP_TRY(hipGetLastError());
  u64 h_cur[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h_cur, dcur.p, 24, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const u64 n_emit = h_cur[0];
  if (uint32_t(h_cur[2]) != 0)
    return fail(FBK_E_INVALID, "bsi_distinct: an exists row holds another number of columns than its stored cardinality says");
  if (n_emit == 0) return FBK_OK;
  if (n_emit > upper)
    return fail(FBK_E_INVALID, "bsi_distinct: the exists rows hold more columns than their stored cardinalities say (" +
                                   std::to_string(n_emit) + " > " + std::to_string(upper) + ")");
  // sort + unique (SignedRow.Union over shards is a set union of the values, executor.go:1196)
  HIP_TRY(dsorted.alloc(ctx, n_emit * 8));
  HIP_TRY(duniq.alloc(ctx, n_emit * 8));
  size_t t1 = 0, t2 = 0;
  u64* d_nu = dcur.as<u64>() + 1;
  HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, t1, dvals.as<long long>(), dsorted.as<long long>(), int(n_emit), 0, 64, ctx->stream));
  HIP_TRY(hipcub::DeviceSelect::Unique(nullptr, t2, dsorted.as<long long>(), duniq.as<long long>(), d_nu, int(n_emit), ctx->stream));
  HIP_TRY(dtmp.alloc(ctx, std::max<size_t>(std::max(t1, t2), 16)));
  size_t tb = std::max(t1, t2);
  HIP_TRY(hipcub::DeviceRadixSort::SortKeys(dtmp.p, tb, dvals.as<long long>(), dsorted.as<long long>(), int(n_emit), 0, 64, ctx->stream));
  tb = std::max(t1, t2);
  HIP_TRY(hipcub::DeviceSelect::Unique(dtmp.p, tb, dsorted.as<long long>(), duniq.as<long long>(), d_nu, int(n_emit), ctx->stream));
  HIP_TRY(hipMemcpyAsync(&n_unique, d_nu, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return FBK_OK;
}

int32_t fbk_bsi_distinct(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                         uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_values,
                         uint64_t cap, uint64_t* out_n) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_n || (n_shards && !base_rows) || (filter && n_shards && !rows_f) || (cap && !out_values))
    return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  *out_n = 0;
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  DevBuf duniq;
  u64 n_unique = 0;
  if (int32_t rc = bsi_distinct_device(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, duniq, n_unique)) return rc;
  *out_n = n_unique;
  if (n_unique == 0) return FBK_OK;
  if (n_unique > cap) return fail(FBK_E_CAPACITY, "bsi_distinct: " + std::to_string(n_unique) + " distinct values, buffer holds " + std::to_string(cap));
  HIP_TRY(hipMemcpyAsync(out_values, duniq.p, n_unique * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op,
                      uint32_t bit_depth, int64_t predicate, uint32_t flags, fbk_batch** out_batch,
                      uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_batch || (n_shards && !base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  *out_batch = nullptr;
  BsiProg prog;
  if (!gen_range_op(prog, op, bit_depth, predicate)) return fail(FBK_E_INVALID, "invalid range operation");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return run_bsi_program(ctx, batch, base_rows, n_shards, bit_depth, prog, flags, out_batch, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op,
                          uint32_t bit_depth, int64_t predicate, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums,
                          uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_sums, out_counts)) return rc;
  if (op < FBK_BSI_EQ || op > FBK_BSI_GTE) return fail(FBK_E_INVALID, "invalid range operation");
  if (n_shards == 0) return FBK_OK;
  fbk::RangeSumPlan pl;
  if (!plan_range_sum(op, bit_depth, predicate, pl)) {
    fbk_batch* rng = nullptr;
    if (int32_t rc = fbk_bsi_range(ctx, batch, base_rows, n_shards, op, bit_depth, predicate, 0, &rng, nullptr)) return rc;
    return bsi_sum_over_range(ctx, batch, base_rows, n_shards, bit_depth, rng, filter, rows_f, out_sums, out_counts);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  BsiShardOperands ops;
  if (int32_t rc = ops.upload(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f)) return rc;
  DevBuf d4, dplan;
  HIP_TRY(d4.alloc(ctx, uint64_t(n_shards) * 32));
  HIP_TRY(dplan.alloc(ctx, sizeof(pl)));
  HIP_TRY(hipMemcpyAsync(dplan.p, &pl, sizeof(pl), hipMemcpyHostToDevice, ctx->stream));
  if (int32_t rc = bsi_range_sum_launch(ctx, batch, ops.base(), n_shards, pl, dplan.as<fbk::RangeSumPlan>(), filter, ops.filter_rows(), d4.as<u64>()))
    return rc;
  std::vector<u64> h4;
  if (int32_t rc = download_words(ctx, d4, uint64_t(n_shards) * 4, h4)) return rc;
  for (uint32_t s = 0; s < n_shards; ++s) {
    // the scanned class's magnitudes and the other class's: which of them is positive decides the signs (Total():
    // int64(psum) - int64(nsum), roaring/filter.go:1106-1108)
    const uint64_t sm = h4[s * 4 + 0], so = h4[s * 4 + 1];
    out_sums[s] = int64_t(pl.scan_positive ? sm - so : so - sm);
    out_counts[s] = h4[s * 4 + 2] + h4[s * 4 + 3];
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range_sum_plan(int32_t op, uint32_t bit_depth, int64_t predicate, uint8_t* out_actions, uint64_t* out_vhi,
                               uint32_t* out_scan_positive, uint32_t* out_take_other) try {
  if (!out_actions || !out_vhi || !out_scan_positive || !out_take_other) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (op < FBK_BSI_EQ || op > FBK_BSI_GTE) return fail(FBK_E_INVALID, "invalid range operation");
  fbk::RangeSumPlan pl;
  if (!plan_range_sum(op, bit_depth, predicate, pl)) return 1;  // the two-pass path
  std::memcpy(out_actions, pl.action, 64);
  std::memcpy(out_vhi, pl.vhi, 64 * 8);
  *out_scan_positive = pl.scan_positive;
  *out_take_other = pl.take_other;
  return FBK_OK;
} FBK_ABI_CATCH(nullptr)

int32_t fbk_bsi_between_sum_plan(uint32_t bit_depth, int64_t lo, int64_t hi, uint8_t* out_actions, uint64_t* out_vhi, uint8_t* out_split,
                                 uint64_t* out_vfin, uint32_t* out_flags) try {
  if (!out_actions || !out_vhi || !out_split || !out_vfin || !out_flags) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  fbk::BetweenSumPlan pl;
  if (!plan_between_sum(bit_depth, lo, hi, pl)) return 1;  // the two-pass path
  std::memcpy(out_actions, pl.action, 128);
  std::memcpy(out_vhi, pl.vhi, 128 * 8);
  std::memcpy(out_split, pl.split, 64);
  out_vfin[0] = pl.vfin[0], out_vfin[1] = pl.vfin[1];
  out_flags[0] = pl.class_pos[0], out_flags[1] = pl.class_pos[1], out_flags[2] = pl.init_b, out_flags[3] = pl.whole[0], out_flags[4] = pl.whole[1];
  return FBK_OK;
} FBK_ABI_CATCH(nullptr)

int32_t fbk_bsi_range_between_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                                  int64_t lo, int64_t hi, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_sums, out_counts)) return rc;
  if (n_shards == 0) return FBK_OK;
  fbk::BetweenSumPlan pl;
  // the one-pass kernel keeps four fragments per wavefront: dense batches only (half a container per wavefront)
  if (!batch->dense || !plan_between_sum(bit_depth, lo, hi, pl)) {
    fbk_batch* rng = nullptr;
    if (int32_t rc = fbk_bsi_range_between(ctx, batch, base_rows, n_shards, bit_depth, lo, hi, 0, &rng, nullptr)) return rc;
    return bsi_sum_over_range(ctx, batch, base_rows, n_shards, bit_depth, rng, filter, rows_f, out_sums, out_counts);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  BsiShardOperands ops;
  if (int32_t rc = ops.upload(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f)) return rc;
  DevBuf d4, dplan;
  HIP_TRY(d4.alloc(ctx, uint64_t(n_shards) * 32));
  HIP_TRY(hipMemsetAsync(d4.p, 0, uint64_t(n_shards) * 32, ctx->stream));
  HIP_TRY(dplan.alloc(ctx, sizeof(pl)));
  HIP_TRY(hipMemcpyAsync(dplan.p, &pl, sizeof(pl), hipMemcpyHostToDevice, ctx->stream));
  const FilterArgs f(filter, ops.filter_rows());
  {
    KernelSpan span(ctx);
    // half a container per wavefront, bsi_planes_ahead planes in flight (the quarter-container form of round 3 was removed
    // again: slower once the planes in flight were counted by hand, and two of its instantiations failed the in-flight check)
    auto kern = fbk::k_bsi_between_sum_part<8, 3>;
    hipLaunchKernelGGL(kern, dim3(uint32_t(uint64_t(n_shards) * fbk::kSlots * 2)), dim3(64), 0, ctx->stream, batch->d_arena, ops.base(), n_shards,
                       dplan.as<fbk::BetweenSumPlan>(), f.slots, f.arena, f.rows, d4.as<u64>());
  }
  HIP_TRY(hipGetLastError());
  std::vector<u64> h4;
  if (int32_t rc = download_words(ctx, d4, uint64_t(n_shards) * 4, h4)) return rc;
  for (uint32_t s = 0; s < n_shards; ++s) {
    const uint64_t s0 = h4[s * 4 + 0], s1 = h4[s * 4 + 1];
    out_sums[s] = int64_t((pl.class_pos[0] ? s0 : 0ull - s0) + (pl.class_pos[1] ? s1 : 0ull - s1));
    out_counts[s] = h4[s * 4 + 2] + h4[s * 4 + 3];
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range_between(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                              uint32_t bit_depth, int64_t lo, int64_t hi, uint32_t flags, fbk_batch** out_batch,
                              uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_batch || (n_shards && !base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  *out_batch = nullptr;
  BsiProg prog;
  gen_between(prog, bit_depth, lo, hi);
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return run_bsi_program(ctx, batch, base_rows, n_shards, bit_depth, prog, flags, out_batch, out_counts);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
