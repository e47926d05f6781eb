// fbk_extract_api.inc — fbk_extract_*: Extract(filter, Rows(f1), Rows(f2), …) (fbk_extract.hip.h).  Included by fbk.hip after
// fbk_matrix_distinct_api.inc.
//
// fbk_extract_open fixes the selected columns: the filter's set bits in shard order, ranks [lo, hi) after offset / limit.  It
// counts the filter's WORDS (k_extract_scan over every shard, never a stored cardinality), reads the shards' prefix back — the
// one synchronisation — and keeps, for the span of shards [s_first, s_first + span) that hold a selected column:
//   sel   [span][16384] u64   the filter's words with the selected columns only         2^17 bytes per shard of the span
//   upre  [span * 1024 + 1]   u32 rank (relative to lo) of every unit's first column    2^12 bytes per shard of the span
//   ids   [n_shards] u64      the shard ids
// The per-field calls walk the span only.  Rows of batches that are not dense are densified a chunk of shards at a time
// (fbk_dense_operands.inc) under kExtractScratch; a set field with more rows per shard than that holds (fbk_extract_rows, n_a >
// 2048) goes one shard per launch and a block of 2048 rows of it.  (fbk.h documents the arithmetic: the tests rely on it.)

namespace {

using fbk_select_plan::kExtractScratch, fbk_select_plan::densify_chunk;  // shared with Sort, the quantiles and Distinct rows

uint32_t extract_grid(uint64_t units) { return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((units + 3) / 4, 8192))); }

}  // namespace

struct fbk_extract {
  fbk_ctx* ctx = nullptr;
  const fbk_batch* filter = nullptr;
  uint32_t n_shards = 0;
  uint64_t n = 0;                      // selected columns (< 2^31)
  uint32_t s_first = 0, span = 0;      // the shards that hold them: [s_first, s_first + span); span == 0 iff n == 0
  DevBuf sel, upre, ids;
};

namespace {

int32_t extract_handle_ok(fbk_ctx* ctx, const fbk_extract* h) {
  if (!ctx || !h) return fail(FBK_E_INVALID, "NULL argument");
  if (h->ctx != ctx) return fail(FBK_E_INVALID, "extract: the handle belongs to another context");
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_extract_open(fbk_ctx* ctx, const fbk_batch* filter, const uint32_t* rows_f, const uint64_t* shard_ids, uint32_t n_shards,
                         uint64_t offset, uint64_t limit, fbk_extract** out, uint64_t* out_n) try {
  FBK_ENTER(ctx);
  if (!out || !out_n || (n_shards && (!rows_f || !shard_ids))) return fail(FBK_E_INVALID, "NULL argument");
  *out = nullptr, *out_n = 0;
  if (int32_t rc = shard_ids_ok(shard_ids, n_shards, "extract")) return rc;
  if (!ctx || !filter) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "extract filter")) return rc;
  std::unique_ptr<fbk_extract> h(new fbk_extract);
  h->ctx = ctx, h->filter = filter, h->n_shards = n_shards;
  if (n_shards == 0 || limit == 0) {
    *out = h.release();
    return FBK_OK;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  DenseOperands ops;
  const int kF = ops.add(filter, rows_f, 1);
  const uint32_t chunk = densify_chunk(n_shards, ops.densified_rows());
  DevBuf unit_pre, shard_tot, shard_base, carry;
  if (int32_t rc = ops.upload(ctx, n_shards, chunk)) return rc;
  HIP_TRY(h->ids.alloc(ctx, uint64_t(n_shards) * 8));
  {
    const void* src = shard_ids;
    if (uint8_t* st = stage_alloc(ctx, uint64_t(n_shards) * 8)) {
      std::memcpy(st, shard_ids, uint64_t(n_shards) * 8);
      src = st;
    }
    HIP_TRY(hipMemcpyAsync(h->ids.p, src, uint64_t(n_shards) * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(unit_pre.alloc(ctx, uint64_t(n_shards) * fbk::kExtractUnits * 4));
  HIP_TRY(shard_tot.alloc(ctx, uint64_t(n_shards) * 4));
  HIP_TRY(shard_base.alloc(ctx, (uint64_t(n_shards) + 1) * 8));
  HIP_TRY(carry.alloc(ctx, 8));
  HIP_TRY(hipMemsetAsync(carry.p, 0, 8, ctx->stream));
  // the filter's columns per unit and per shard, from its words
  ops.for_each_chunk(ctx, true, DenseOperands::Densify::together, [&](uint32_t s0, uint32_t ns) {
    const DenseView F = ops.view(kF, s0);
    hipLaunchKernelGGL(fbk::k_extract_scan, dim3(ns), dim3(1024), 0, ctx->stream, F.arena, F.rows, unit_pre.as<uint32_t>() + uint64_t(s0) * fbk::kExtractUnits,
                       shard_tot.as<uint32_t>() + s0);
  });
  exclusive_scan_u32(ctx, shard_tot.as<uint32_t>(), n_shards, shard_base.as<u64>(), carry.as<u64>());
  HIP_TRY(hipGetLastError());
  std::vector<uint64_t> base(uint64_t(n_shards) + 1);
  {
    D2H back(ctx);
    HIP_TRY(back.add(base.data(), shard_base.p, base.size() * 8));
    HIP_TRY(back.finish());
  }
  const uint64_t total = base[n_shards], lo = std::min(offset, total), n = std::min(limit, total - lo), hi = lo + n;
  if (n >= (1ull << 31))
    return fail(FBK_E_INVALID, "extract: " + std::to_string(n) + " columns selected; one handle takes fewer than 2^31: use a limit");
  *out_n = n;
  if (n == 0) {
    *out = h.release();
    return FBK_OK;
  }
  // the span: the first shard with a column of rank >= lo, the last with one of rank < hi
  const uint32_t s_first = uint32_t(std::upper_bound(base.begin(), base.end(), lo) - base.begin() - 1);
  const uint32_t s_last = uint32_t(std::lower_bound(base.begin(), base.end(), hi) - base.begin() - 1);
  const uint32_t span = s_last - s_first + 1;
  h->n = n, h->s_first = s_first, h->span = span;
  const uint64_t su_end = uint64_t(span) * fbk::kExtractUnits;
  HIP_TRY(h->sel.alloc(ctx, su_end * fbk::kExtractWords * 8));
  HIP_TRY(h->upre.alloc(ctx, (su_end + 1) * 4));
  for (uint32_t s0 = 0; s0 < span; s0 += chunk) {  // (not for_each_chunk: a sub-span, walked with the first pass's chunk, scratch and lists)
    const uint32_t ns = std::min(chunk, span - s0);
    ops.densify(ctx, s_first + s0, ns);
    const DenseView F = ops.view(kF, s_first + s0);
    hipLaunchKernelGGL(fbk::k_extract_select, dim3(extract_grid(uint64_t(ns) * fbk::kExtractUnits)), dim3(256), 0, ctx->stream, F.arena, F.rows, ns,
                       unit_pre.as<uint32_t>(), shard_base.as<u64>(), s_first + s0, s0, u64(lo), u64(hi), u64(su_end), h->sel.as<u64>(), h->upre.as<uint32_t>());
  }
  HIP_TRY(hipGetLastError());
  *out = h.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_extract_span(fbk_ctx* ctx, const fbk_extract* h, uint32_t* out_first, uint32_t* out_count) try {
  FBK_ENTER(ctx);
  if (int32_t rc = extract_handle_ok(ctx, h)) return rc;
  if (!out_first || !out_count) return fail(FBK_E_INVALID, "NULL argument");
  *out_first = h->s_first, *out_count = h->span;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_extract_columns(fbk_ctx* ctx, fbk_extract* h, uint64_t* out_columns) try {
  FBK_ENTER(ctx);
  if (int32_t rc = extract_handle_ok(ctx, h)) return rc;
  if (h->n == 0) return FBK_OK;
  if (!out_columns) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  DevBuf cols;
  HIP_TRY(cols.alloc(ctx, h->n * 8));
  const uint64_t units = uint64_t(h->span) * fbk::kExtractUnits;
  hipLaunchKernelGGL(fbk::k_extract_columns, dim3(extract_grid(units)), dim3(256), 0, ctx->stream, h->sel.as<u64>(), h->upre.as<uint32_t>(),
                     h->ids.as<u64>() + h->s_first, u64(units), u64(h->n), cols.as<u64>());
  HIP_TRY(hipGetLastError());
  D2H back(ctx);
  HIP_TRY(back.add(out_columns, cols.p, h->n * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_extract_bsi(fbk_ctx* ctx, fbk_extract* h, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth,
                        int64_t* out_values, uint8_t* out_present) try {
  FBK_ENTER(ctx);
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (int32_t rc = extract_handle_ok(ctx, h)) return rc;
  if (!bsi || (h->n_shards && !base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = bsi_rows_ok(base_rows, h->n_shards, bit_depth, bsi->n_rows)) return rc;
  if (h->n == 0) return FBK_OK;
  if (!out_values || !out_present) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  const uint32_t span = h->span;
  DenseOperands ops;
  const int kS = ops.add(bsi, base_rows + h->s_first, bit_depth + 2, true);
  const uint32_t chunk = densify_chunk(span, ops.densified_rows());
  DevBuf vals, pres;
  if (int32_t rc = ops.upload(ctx, span, chunk)) return rc;
  HIP_TRY(vals.alloc(ctx, h->n * 8));
  HIP_TRY(pres.alloc(ctx, h->n));
  ops.for_each_chunk(ctx, true, DenseOperands::Densify::together, [&](uint32_t s0, uint32_t ns) {
    const DenseView S = ops.view(kS, s0);
    hipLaunchKernelGGL(fbk::k_extract_bsi, dim3(extract_grid(uint64_t(ns) * fbk::kExtractUnits)), dim3(256), 0, ctx->stream, S.arena, S.rows, ns, s0, bit_depth,
                       h->sel.as<u64>(), h->upre.as<uint32_t>(), u64(h->n), vals.as<long long>(), pres.as<uint8_t>());
  });
  HIP_TRY(hipGetLastError());
  D2H back(ctx);
  HIP_TRY(back.add(out_values, vals.p, h->n * 8));
  HIP_TRY(back.add(out_present, pres.p, h->n));
  HIP_TRY(back.finish());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_extract_rows(fbk_ctx* ctx, fbk_extract* h, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, uint64_t* out_offsets,
                         uint32_t* out_items, uint64_t cap, uint64_t* out_n_items) try {
  FBK_ENTER(ctx);
  if (n_a > 4096) return fail(FBK_E_INVALID, "extract_rows: at most 4096 rows per call");
  if (int32_t rc = extract_handle_ok(ctx, h)) return rc;
  if (!a || !out_offsets || !out_n_items || (h->n_shards && n_a && !rows_a) || (cap && !out_items)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = check_rows(rows_a, uint64_t(h->n_shards) * n_a, a->n_rows, "extract_rows")) return rc;
  *out_n_items = 0;
  const uint64_t n = h->n;
  if (n == 0 || n_a == 0) {
    std::memset(out_offsets, 0, (n + 1) * 8);
    return FBK_OK;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  const uint32_t span = h->span;
  DenseOperands ops;
  const int kA = ops.add(a, rows_a + uint64_t(h->s_first) * n_a, n_a);
  // a chunk of shards and all their rows per launch, or (one shard's rows exceed the scratch) one shard and a block of its rows
  const uint64_t per_shard = kDenseRowBytes * ops.densified_rows();
  const bool blocks = per_shard > kExtractScratch;
  const uint32_t chunk = blocks ? 1 : even_chunk(span, kExtractScratch, per_shard), block = blocks ? uint32_t(kExtractScratch / kDenseRowBytes) : n_a;
  DevBuf counts, tsum, tbase, carry, offs, items;
  if (int32_t rc = ops.upload(ctx, span, chunk, block)) return rc;
  const uint64_t n_tiles = (n + 1 + fbk::kExtractTile - 1) / fbk::kExtractTile, padded = n_tiles * fbk::kExtractTile;  // n + 1: offs[n] is the total
  HIP_TRY(counts.alloc(ctx, padded * 4));
  HIP_TRY(tsum.alloc(ctx, n_tiles * 4));
  HIP_TRY(tbase.alloc(ctx, (n_tiles + 1) * 8));
  HIP_TRY(carry.alloc(ctx, 8));
  HIP_TRY(offs.alloc(ctx, (n + 1) * 8));
  // one walk over the span, a chunk of shards and a block of rows per launch: counts (fill == false), then the items
  auto walk = [&](bool fill, u64 m) {
    for (uint32_t s0 = 0; s0 < span; s0 += chunk) {  // (not for_each_chunk: a block of rows is densified inside the chunk)
      const uint32_t ns = std::min(chunk, span - s0);
      for (uint32_t i0 = 0; i0 < n_a; i0 += block) {
        const uint32_t nr = std::min(block, n_a - i0);
        ops.densify_one(ctx, kA, s0, ns, i0, nr);
        const DenseView A = ops.view(kA, s0, i0);
        const dim3 grid(extract_grid(uint64_t(ns) * fbk::kExtractUnits));
        if (fill)
          hipLaunchKernelGGL(fbk::k_extract_rows<true>, grid, dim3(256), 0, ctx->stream, A.arena, A.rows, A.stride, nr, i0, ns, s0, h->sel.as<u64>(),
                             h->upre.as<uint32_t>(), u64(n), counts.as<uint32_t>(), offs.as<u64>(), items.as<uint32_t>(), m);
        else
          hipLaunchKernelGGL(fbk::k_extract_rows<false>, grid, dim3(256), 0, ctx->stream, A.arena, A.rows, A.stride, nr, i0, ns, s0, h->sel.as<u64>(),
                             h->upre.as<uint32_t>(), u64(n), counts.as<uint32_t>(), static_cast<const u64*>(nullptr), static_cast<uint32_t*>(nullptr), m);
      }
    }
  };
  HIP_TRY(hipMemsetAsync(counts.p, 0, padded * 4, ctx->stream));
  HIP_TRY(hipMemsetAsync(carry.p, 0, 8, ctx->stream));
  walk(false, 0);
  hipLaunchKernelGGL(fbk::k_extract_tile_sums, dim3(uint32_t(n_tiles)), dim3(1024), 0, ctx->stream, counts.as<uint32_t>(), tsum.as<uint32_t>());
  exclusive_scan_u32(ctx, tsum.as<uint32_t>(), uint32_t(n_tiles), tbase.as<u64>(), carry.as<u64>());
  hipLaunchKernelGGL(fbk::k_extract_offsets, dim3(uint32_t(n_tiles)), dim3(1024), 0, ctx->stream, counts.as<uint32_t>(), tbase.as<u64>(), u64(n + 1),
                     offs.as<u64>());
  HIP_TRY(hipGetLastError());
  D2H back(ctx);
  HIP_TRY(back.add(out_offsets, offs.p, (n + 1) * 8));
  HIP_TRY(back.finish());
  const uint64_t m = out_offsets[n];
  *out_n_items = m;
  if (m > cap) return fail(FBK_E_CAPACITY, "extract_rows: " + std::to_string(m) + " items, capacity " + std::to_string(cap));
  if (m == 0) return FBK_OK;
  ctx->h_stage_used = 0;  // (the offsets have left the staging area)
  HIP_TRY(items.alloc(ctx, m * 4));
  HIP_TRY(hipMemsetAsync(counts.p, 0, padded * 4, ctx->stream));
  walk(true, m);
  HIP_TRY(hipGetLastError());
  HIP_TRY(back.add(out_items, items.p, m * 4));
  HIP_TRY(back.finish());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_extract_free(fbk_ctx* ctx, fbk_extract* h) try {
  FBK_ENTER(ctx);
  if (!h) return FBK_OK;
  if (int32_t rc = extract_handle_ok(ctx, h)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  delete h;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
