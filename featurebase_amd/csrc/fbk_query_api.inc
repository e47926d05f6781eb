// fbk_query_api.inc — host side of the query-level entry points (included by fbk.hip): what they share — check_rows, FilterArgs, the
// resolved row records of the prepared folds, count matrix and TopN (RowRecords), the key rule of the materialising row operations —
// and Rows, Flip, Shift, compaction.  The folds: fbk_fold_api.inc.  The BSI calls: fbk_bsi_api.inc.  The output batch of the
// materialising ones is a CellOutput (fbk_output.inc).  The GroupBy count matrix: fbk_count_matrix_api.inc.  TopK / TopN: fbk_topn_api.inc.

namespace {

int32_t check_rows(const uint32_t* rows, uint64_t n, uint32_t limit, const char* what) {
  for (uint64_t i = 0; i < n; ++i)
    if (rows[i] >= limit) return fail(FBK_E_INVALID, std::string(what) + ": row index out of range");
  return FBK_OK;
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

}  // namespace

extern "C" {

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
  if (n_rows) {
    hipLaunchKernelGGL(fbk::k_flip, dim3(uint32_t((n_rows * fbk::kSlots + 3) / 4)), dim3(256), 0, ctx->stream, batch->d_slots, batch->d_arena,
                       drows.as<uint32_t>(), n_rows, uint32_t(start), uint32_t(end), o->d_arena, o->d_slots, out.runs(), out.counts(), uint32_t(out.kernel_encodes(flags)));
    if (int32_t rc = out.finish(n_rows, out_counts)) return rc;
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
  if (n_rows) {
    hipLaunchKernelGGL(fbk::k_shift, dim3(uint32_t((n_rows * fbk::kSlots + 3) / 4)), dim3(256), 0, ctx->stream, batch->d_slots,
                       batch->d_arena, drows.as<uint32_t>(), carry_rows ? dcarry.as<uint32_t>() : (const uint32_t*)nullptr, n_rows,
                       o->d_arena, o->d_slots, out.runs(), out.counts(), uint32_t(out.kernel_encodes(flags)));
    if (int32_t rc = out.finish(n_rows, out_counts)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
