// fbk_extract_api.inc — fbk_extract_*: Extract(filter, Rows(f1), Rows(f2), …) (fbk_extract.hip.h).  Included by fbk.hip after
// fbk_matrix_distinct_api.inc.
//
// fbk_extract_open fixes the selected columns: the filter's set bits in shard order, ranks [lo, hi) after offset / limit.  It
// counts the filter's WORDS (k_extract_scan over every shard, never a stored cardinality), reads the shards' prefix back — the
// one synchronisation — and keeps, for the span of shards [s_first, s_first + span) that hold a selected column:
//   sel   [span][16384] u64   the filter's words with the selected columns only         2^17 bytes per shard of the span
//   upre  [span * 1024 + 1]   u32 rank (relative to lo) of every unit's first column    2^12 bytes per shard of the span
//   ids   [n_shards] u64      the shard ids
// The per-field calls walk the span only.  Rows of batches that are not dense are densified a chunk at a time (fbk.h documents the
// arithmetic: the tests rely on it):
//   per_shard = 2^17 * R, R = the rows densified per shard (filter 1, BSI bit_depth + 2, set field n_a);
//   per_shard <= kExtractScratch: most = max(1, min(shards, kExtractScratch / per_shard)), chunk = ceil(shards / ceil(shards / most))
//     shards per launch, all their rows;  else one shard per launch and blocks of kExtractScratch / 2^17 (2048) rows of it.

namespace {

constexpr uint64_t kExtractScratch = 1ull << 28;
constexpr uint64_t kExtractRowBytes = uint64_t(fbk::kSlots) * 8192;

struct ExtractChunks {
  uint32_t shards = 0;  // shards per launch
  uint32_t rows = 0;    // rows of a shard per launch
};

ExtractChunks extract_chunks(uint32_t shards, uint32_t rows_per_shard) {
  ExtractChunks c;
  const uint64_t per_shard = kExtractRowBytes * rows_per_shard;
  if (per_shard <= kExtractScratch) {
    const uint64_t most = std::max<uint64_t>(1, std::min<uint64_t>(shards, per_shard ? kExtractScratch / per_shard : shards));
    const uint64_t passes = (shards + most - 1) / most;
    c.shards = uint32_t((shards + passes - 1) / passes), c.rows = rows_per_shard;
  } else {
    c.shards = 1, c.rows = uint32_t(kExtractScratch / kExtractRowBytes);
  }
  return c;
}

uint32_t extract_grid(uint64_t units) { return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((units + 3) / 4, 8192))); }

void extract_densify(fbk_ctx* ctx, const fbk_batch* b, const uint32_t* d_rows, uint64_t n_rows, uint8_t* out) {
  fbk::DensifyArgs dargs{};
  dargs.src[0] = {b->d_slots, b->d_arena, d_rows, n_rows, out};
  hipLaunchKernelGGL(fbk::k_densify_rows, dim3(uint32_t((n_rows * fbk::kSlots + 3) / 4)), dim3(256), 0, ctx->stream, dargs);
}

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
  for (uint32_t s = 0; s < n_shards; ++s) {
    if (shard_ids[s] >= (1ull << 44)) return fail(FBK_E_INVALID, "extract: shard id >= 2^44 (column ids are shard * 2^20 + position)");
    if (s && shard_ids[s] <= shard_ids[s - 1]) return fail(FBK_E_INVALID, "extract: shard_ids must be strictly ascending");
  }
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
  const bool df = !filter->dense;
  const ExtractChunks ck = extract_chunks(n_shards, 1);
  std::vector<uint32_t> iota(df ? ck.shards : 0);
  for (uint32_t i = 0; i < iota.size(); ++i) iota[i] = i;
  DevBuf rows, unit_pre, shard_tot, shard_base, carry, dense;
  const uint32_t* d[2];
  if (int32_t rc = upload_rows_multi(ctx, {{rows_f, n_shards, UINT32_MAX}, {iota.data(), iota.size(), UINT32_MAX}}, rows, d)) return rc;
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
  if (df) HIP_TRY(dense.alloc(ctx, uint64_t(ck.shards) * kExtractRowBytes));
  // the filter's columns per unit and per shard, from its words
  for (uint32_t s0 = 0; s0 < n_shards; s0 += ck.shards) {
    const uint32_t ns = df ? std::min(ck.shards, n_shards - s0) : n_shards;
    if (df) extract_densify(ctx, filter, d[0] + s0, ns, dense.as<uint8_t>());
    hipLaunchKernelGGL(fbk::k_extract_scan, dim3(ns), dim3(1024), 0, ctx->stream, df ? dense.as<uint8_t>() : filter->d_arena, df ? d[1] : d[0],
                       unit_pre.as<uint32_t>() + uint64_t(s0) * fbk::kExtractUnits, shard_tot.as<uint32_t>() + s0);
    if (!df) break;
  }
  hipLaunchKernelGGL(fbk::k_bsi_cell_scan, dim3(1), dim3(1024), 0, ctx->stream, static_cast<const Slot*>(nullptr), static_cast<const uint32_t*>(nullptr),
                     shard_tot.as<uint32_t>(), n_shards, shard_base.as<u64>(), carry.as<u64>());
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
  for (uint32_t s0 = 0; s0 < span; s0 += ck.shards) {  // (the chunk of the first pass: its buffer and index list)
    const uint32_t ns = df ? std::min(ck.shards, span - s0) : span;
    if (df) extract_densify(ctx, filter, d[0] + s_first + s0, ns, dense.as<uint8_t>());
    hipLaunchKernelGGL(fbk::k_extract_select, dim3(extract_grid(uint64_t(ns) * fbk::kExtractUnits)), dim3(256), 0, ctx->stream,
                       df ? dense.as<uint8_t>() : filter->d_arena, df ? d[1] : d[0] + s_first + s0, ns, unit_pre.as<uint32_t>(), shard_base.as<u64>(),
                       s_first + s0, s0, u64(lo), u64(hi), u64(su_end), h->sel.as<u64>(), h->upre.as<uint32_t>());
    if (!df) break;
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
  const uint64_t rps = uint64_t(bit_depth) + 2;
  for (uint32_t s = 0; s < h->n_shards; ++s)
    if (uint64_t(base_rows[s]) + rps > bsi->n_rows) return fail(FBK_E_INVALID, "bsi: fragment rows (exists, sign, bit planes) exceed the batch");
  if (h->n == 0) return FBK_OK;
  if (!out_values || !out_present) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  const bool dd = !bsi->dense;
  const uint32_t span = h->span;
  const uint32_t* base = base_rows + h->s_first;
  const ExtractChunks ck = extract_chunks(span, uint32_t(rps));
  std::vector<uint32_t> all(dd ? uint64_t(span) * rps : 0), ibase(dd ? ck.shards : 0);
  for (uint32_t s = 0; s < span && dd; ++s)
    for (uint64_t r = 0; r < rps; ++r) all[uint64_t(s) * rps + r] = uint32_t(base[s] + r);
  for (uint64_t i = 0; i < ibase.size(); ++i) ibase[i] = uint32_t(i * rps);
  DevBuf rows, dense, vals, pres;
  const uint32_t* d[3];
  if (int32_t rc = upload_rows_multi(ctx, {{base, span, UINT32_MAX}, {all.data(), all.size(), UINT32_MAX}, {ibase.data(), ibase.size(), UINT32_MAX}}, rows, d))
    return rc;
  if (dd) HIP_TRY(dense.alloc(ctx, uint64_t(ck.shards) * rps * kExtractRowBytes));
  HIP_TRY(vals.alloc(ctx, h->n * 8));
  HIP_TRY(pres.alloc(ctx, h->n));
  for (uint32_t s0 = 0; s0 < span; s0 += ck.shards) {
    const uint32_t ns = dd ? std::min(ck.shards, span - s0) : span;
    if (dd) extract_densify(ctx, bsi, d[1] + uint64_t(s0) * rps, uint64_t(ns) * rps, dense.as<uint8_t>());
    hipLaunchKernelGGL(fbk::k_extract_bsi, dim3(extract_grid(uint64_t(ns) * fbk::kExtractUnits)), dim3(256), 0, ctx->stream,
                       dd ? dense.as<uint8_t>() : bsi->d_arena, dd ? d[2] : d[0], ns, s0, bit_depth, h->sel.as<u64>(), h->upre.as<uint32_t>(), u64(h->n),
                       vals.as<long long>(), pres.as<uint8_t>());
    if (!dd) break;
  }
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
  const bool da = !a->dense;
  const uint32_t span = h->span;
  const uint32_t* ra = rows_a + uint64_t(h->s_first) * n_a;
  const ExtractChunks ck = extract_chunks(span, n_a);
  std::vector<uint32_t> iota(da ? uint64_t(ck.shards) * ck.rows : 0);
  for (uint64_t i = 0; i < iota.size(); ++i) iota[i] = uint32_t(i);
  DevBuf rows, dense, counts, tsum, tbase, carry, offs, items;
  const uint32_t* d[2];
  if (int32_t rc = upload_rows_multi(ctx, {{ra, uint64_t(span) * n_a, UINT32_MAX}, {iota.data(), iota.size(), UINT32_MAX}}, rows, d)) return rc;
  if (da) HIP_TRY(dense.alloc(ctx, uint64_t(ck.shards) * ck.rows * kExtractRowBytes));
  const uint64_t n_tiles = (n + 1 + fbk::kExtractTile - 1) / fbk::kExtractTile, padded = n_tiles * fbk::kExtractTile;  // n + 1: offs[n] is the total
  HIP_TRY(counts.alloc(ctx, padded * 4));
  HIP_TRY(tsum.alloc(ctx, n_tiles * 4));
  HIP_TRY(tbase.alloc(ctx, (n_tiles + 1) * 8));
  HIP_TRY(carry.alloc(ctx, 8));
  HIP_TRY(offs.alloc(ctx, (n + 1) * 8));
  // one walk over the span, a chunk of shards and a block of rows per launch: counts (fill == false), then the items
  auto walk = [&](bool fill, u64 m) {
    for (uint32_t s0 = 0; s0 < span; s0 += ck.shards) {
      const uint32_t ns = da ? std::min(ck.shards, span - s0) : span;
      for (uint32_t i0 = 0; i0 < n_a; i0 += ck.rows) {
        const uint32_t nr = da ? std::min(ck.rows, n_a - i0) : n_a;
        // (row blocks only with one shard per launch: its rows [i0, i0 + nr) are consecutive in the list)
        if (da) extract_densify(ctx, a, d[0] + uint64_t(s0) * n_a + i0, uint64_t(ns) * nr, dense.as<uint8_t>());
        const uint8_t* arena = da ? dense.as<uint8_t>() : a->d_arena;
        const uint32_t* rr = da ? d[1] : d[0];
        const dim3 grid(extract_grid(uint64_t(ns) * fbk::kExtractUnits));
        if (fill)
          hipLaunchKernelGGL(fbk::k_extract_rows<true>, grid, dim3(256), 0, ctx->stream, arena, rr, da ? nr : n_a, nr, i0, ns, s0, h->sel.as<u64>(),
                             h->upre.as<uint32_t>(), u64(n), counts.as<uint32_t>(), offs.as<u64>(), items.as<uint32_t>(), m);
        else
          hipLaunchKernelGGL(fbk::k_extract_rows<false>, grid, dim3(256), 0, ctx->stream, arena, rr, da ? nr : n_a, nr, i0, ns, s0, h->sel.as<u64>(),
                             h->upre.as<uint32_t>(), u64(n), counts.as<uint32_t>(), static_cast<const u64*>(nullptr), static_cast<uint32_t*>(nullptr), m);
        if (!da) break;
      }
      if (!da) break;
    }
  };
  HIP_TRY(hipMemsetAsync(counts.p, 0, padded * 4, ctx->stream));
  HIP_TRY(hipMemsetAsync(carry.p, 0, 8, ctx->stream));
  walk(false, 0);
  hipLaunchKernelGGL(fbk::k_extract_tile_sums, dim3(uint32_t(n_tiles)), dim3(1024), 0, ctx->stream, counts.as<uint32_t>(), tsum.as<uint32_t>());
  hipLaunchKernelGGL(fbk::k_bsi_cell_scan, dim3(1), dim3(1024), 0, ctx->stream, static_cast<const Slot*>(nullptr), static_cast<const uint32_t*>(nullptr),
                     tsum.as<uint32_t>(), uint32_t(n_tiles), tbase.as<u64>(), carry.as<u64>());
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
