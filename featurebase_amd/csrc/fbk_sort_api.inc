// fbk_sort_api.inc — fbk_bsi_sort (Sort() by an int field) and fbk_extract_open_columns (an extract handle from a column list):
// fbk_sort.hip.h.  Included by fbk.hip after fbk_extract_api.inc.
//
// fbk_bsi_sort walks the shards a few times (a radix-select pass per 11 key bits, a count pass, a collect pass).  Its key, its cut
// and the digit descent are fbk_select_plan.h's; its operands and its walk are FieldOperands below, which fbk_bsi_quantiles and
// fbk_bsi_distinct_rows share.  Device scratch (fbk.h documents it):
//   2^14 + 2^23 (histogram, the blocks' partial histograms) + 2^15 per shard (counts and prefixes of its 1024 units, key < T and
//   key == T) + the densify chunk (<= 2^28) + 16 K (candidates) + 16 n_less + the radix sort's temporary storage (sorted pairs)
//   + 16 n (the records) + the row lists.

namespace {

namespace sp = fbk_select_plan;

// The operand arguments of a call over one int field and a filter row per shard, in the order these calls reject them
int32_t field_args_ok(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                      uint32_t n_shards, uint32_t max_shards, const char* cap_text, const char* filter_text) {
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (n_shards > max_shards) return fail(FBK_E_INVALID, cap_text);
  if (!ctx || !bsi || (n_shards && !base_rows) || (filter && n_shards && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, bsi->n_rows)) return rc;
  return filter ? check_rows(rows_f, n_shards, filter->n_rows, filter_text) : FBK_OK;
}

// A filter row and one int field fragment per shard, the single-field sibling of GroupFieldOperands (fbk_group_field.inc): what
// the kernels on sort_walk_unit read.  A walk densifies under kExtractScratch, the filter's rows and the field's in a launch each.
struct FieldOperands {
  DenseOperands ops;
  int F = 0, S = 0;  // the operands' numbers in ops
  uint32_t n_shards = 0;
  // depth_read: the planes the kernels read (the fragment's exists and sign rows come with them)
  void add(const fbk_batch* bsi, const uint32_t* base_rows, uint32_t depth_read, const fbk_batch* filter, const uint32_t* rows_f, uint32_t shards) {
    n_shards = shards;
    F = ops.add(filter, rows_f, 1), S = ops.add(bsi, base_rows, depth_read + 2, true);
  }
  int32_t upload(fbk_ctx* ctx) { return ops.upload(ctx, n_shards, sp::densify_chunk(n_shards, ops.densified_rows())); }

  // fn(S, F, s0, ns, grid) for every chunk [s0, s0 + ns): the field's and the filter's views, a block per four units.  Every walk
  // densifies again, a single chunk too: skipping the repeat (DenseOperands::for_each_chunk's first_walk) changes the launches.
  template <class Fn>
  void for_each_chunk(fbk_ctx* ctx, Fn fn) {
    ops.for_each_chunk(ctx, true, DenseOperands::Densify::each, [&](uint32_t s0, uint32_t ns) {
      fn(ops.view(S, s0), ops.view(F, s0), s0, ns, dim3(extract_grid(uint64_t(ns) * fbk::kExtractUnits)));
    });
  }
};

}  // namespace

extern "C" {

int32_t fbk_bsi_sort(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                     const uint64_t* shard_ids, uint32_t n_shards, uint32_t flags, uint64_t offset, uint64_t limit, uint64_t* out_columns,
                     int64_t* out_values, uint64_t cap, uint64_t* out_n, uint64_t* out_total) try {
  FBK_ENTER(ctx);
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (!out_n || (n_shards && (!base_rows || !shard_ids)) || (cap && (!out_columns || !out_values))) return fail(FBK_E_INVALID, "NULL argument");
  *out_n = 0;
  if (out_total) *out_total = 0;
  if (flags & ~uint32_t(FBK_SORT_DESC | FBK_SORT_KEEP_ZERO)) return fail(FBK_E_INVALID, "sort: unknown flag");
  if (int32_t rc = shard_ids_ok(shard_ids, n_shards, "sort")) return rc;
  if (int32_t rc = field_args_ok(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards, 1u << 20, "sort: at most 2^20 shards per call", "sort filter")) return rc;
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;

  const fbk::SortKey sk = fbk::select_key(bit_depth, flags & FBK_SORT_DESC, flags & FBK_SORT_KEEP_ZERO);
  const uint32_t nbits = fbk::key_bits(bit_depth), passes = fbk::passes(bit_depth, fbk::kSortDigitBits);

  FieldOperands fo;
  fo.add(bsi, base_rows, bit_depth, filter, rows_f, n_shards);
  DevBuf ids, hist, part, n_lt, n_eq, p_lt, p_eq, keys, cols, skeys, scols, tmp, ocols, ovals;
  if (int32_t rc = fo.upload(ctx)) return rc;
  HIP_TRY(ids.alloc(ctx, uint64_t(n_shards) * 8));
  HIP_TRY(hipMemcpyAsync(ids.p, shard_ids, uint64_t(n_shards) * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hist.alloc(ctx, fbk::kSortBins * 8));
  HIP_TRY(part.alloc(ctx, uint64_t(fbk::kSortHistBlocks) * fbk::kSortBins * 4));

  // radix select: total, then the K-th smallest key T, the columns below it and the ties to take
  std::vector<uint64_t> hh(fbk::kSortBins);
  uint64_t total = 0, K = 0, T = 0, n_less = 0, want = 0;
  bool take_all = false;
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t shift = fbk::kSortDigitBits * (passes - 1 - p);
    HIP_TRY(hipMemsetAsync(hist.p, 0, fbk::kSortBins * 8, ctx->stream));
    fo.for_each_chunk(ctx, [&](const DenseView& S, const DenseView& F, uint32_t, uint32_t ns, dim3 grid) {
      const uint32_t nb = std::min(grid.x, fbk::kSortHistBlocks);
      hipLaunchKernelGGL(fbk::k_sort_hist, dim3(nb), dim3(256), 0, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, bit_depth, sk, shift, u64(T),
                         p ? 1u : 0u, part.as<uint32_t>());
      hipLaunchKernelGGL(fbk::k_sort_hist_sum, dim3(fbk::kSortBins / 256, 32), dim3(256), 0, ctx->stream, part.as<uint32_t>(), nb, hist.as<u64>());
    });
    HIP_TRY(hipGetLastError());
    {
      D2H back(ctx);
      HIP_TRY(back.add(hh.data(), hist.p, fbk::kSortBins * 8));
      HIP_TRY(back.finish());
      ctx->h_stage_used = 0;  // (row lists and histogram have left the staging area)
    }
    if (p == 0) {
      for (uint64_t c : hh) total += c;
      if (out_total) *out_total = total;
      const sp::SortCut cut = sp::sort_cut(total, offset, limit);
      K = cut.K;
      if (K >= (1ull << 31))
        return fail(FBK_E_INVALID, "sort: " + std::to_string(K) + " records to order (offset + limit, or every column without a limit); one call takes fewer than 2^31: use a limit");
      *out_n = K - cut.lo;
      if (*out_n > cap) return fail(FBK_E_CAPACITY, "sort: " + std::to_string(*out_n) + " records, capacity " + std::to_string(cap));
      if (*out_n == 0) return FBK_OK;
      want = K, take_all = K == total;
      if (take_all) break;
    }
    const sp::Descent d = sp::descend(hh.data(), fbk::kSortBins, want - 1);
    n_less += d.before, want -= d.before, T = (T << fbk::kSortDigitBits) | d.bin;
  }
  const uint64_t r = take_all ? 0 : want;
  if (take_all) n_less = K;

  // ranks of the candidates, then the candidates
  const uint64_t n_units = uint64_t(n_shards) * fbk::kExtractUnits;
  HIP_TRY(n_lt.alloc(ctx, (n_units + 1) * 8));
  HIP_TRY(n_eq.alloc(ctx, (n_units + 1) * 8));
  HIP_TRY(p_lt.alloc(ctx, (n_units + 1) * 8));
  HIP_TRY(p_eq.alloc(ctx, (n_units + 1) * 8));
  HIP_TRY(hipMemsetAsync(n_lt.as<u64>() + n_units, 0, 8, ctx->stream));
  HIP_TRY(hipMemsetAsync(n_eq.as<u64>() + n_units, 0, 8, ctx->stream));
  fo.for_each_chunk(ctx, [&](const DenseView& S, const DenseView& F, uint32_t s0, uint32_t ns, dim3 grid) {
    hipLaunchKernelGGL(fbk::k_sort_count, grid, dim3(256), 0, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, s0, bit_depth, sk, u64(T),
                       take_all ? 1u : 0u, n_lt.as<u64>(), n_eq.as<u64>());
  });
  size_t t_scan = 0, t_sort = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, n_lt.as<u64>(), p_lt.as<u64>(), int(n_units + 1), ctx->stream));
  if (n_less)
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, static_cast<const u64*>(nullptr), static_cast<u64*>(nullptr), static_cast<const u64*>(nullptr),
                                               static_cast<u64*>(nullptr), int(n_less), 0, int(nbits), ctx->stream));
  HIP_TRY(tmp.alloc(ctx, std::max<size_t>(std::max(t_scan, t_sort), 16)));
  size_t tb = t_scan;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, n_lt.as<u64>(), p_lt.as<u64>(), int(n_units + 1), ctx->stream));
  tb = t_scan;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, n_eq.as<u64>(), p_eq.as<u64>(), int(n_units + 1), ctx->stream));
  HIP_TRY(keys.alloc(ctx, K * 8));
  HIP_TRY(cols.alloc(ctx, K * 8));
  fo.for_each_chunk(ctx, [&](const DenseView& S, const DenseView& F, uint32_t s0, uint32_t ns, dim3 grid) {
    hipLaunchKernelGGL(fbk::k_sort_collect, grid, dim3(256), 0, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, s0, bit_depth, sk, u64(T),
                       take_all ? 1u : 0u, p_lt.as<u64>(), p_eq.as<u64>(), ids.as<u64>(), u64(n_less), u64(r), keys.as<u64>(), cols.as<u64>());
  });
  HIP_TRY(hipGetLastError());

  // order the columns below T (stable: equal keys stay in ascending column order), cut, download
  const uint64_t n = *out_n, lo = K - n;
  if (n_less) {
    HIP_TRY(skeys.alloc(ctx, n_less * 8));
    HIP_TRY(scols.alloc(ctx, n_less * 8));
    tb = t_sort;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, keys.as<u64>(), skeys.as<u64>(), cols.as<u64>(), scols.as<u64>(), int(n_less), 0, int(nbits), ctx->stream));
  }
  HIP_TRY(ocols.alloc(ctx, n * 8));
  HIP_TRY(ovals.alloc(ctx, n * 8));
  hipLaunchKernelGGL(fbk::k_sort_emit, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, skeys.as<u64>(), scols.as<u64>(), keys.as<u64>(),
                     cols.as<u64>(), u64(n_less), u64(lo), u64(n), sk, ocols.as<u64>(), ovals.as<long long>());
  HIP_TRY(hipGetLastError());
  D2H back(ctx);
  HIP_TRY(back.add(out_columns, ocols.p, n * 8));
  HIP_TRY(back.add(out_values, ovals.p, n * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_extract_open_columns(fbk_ctx* ctx, const uint64_t* columns, uint64_t n, const uint64_t* shard_ids, uint32_t n_shards, fbk_extract** out,
                                 uint32_t* out_rank) try {
  FBK_ENTER(ctx);
  if (!out || (n && (!columns || !out_rank)) || (n_shards && !shard_ids)) return fail(FBK_E_INVALID, "NULL argument");
  *out = nullptr;
  if (n >= (1ull << 31)) return fail(FBK_E_INVALID, "extract: " + std::to_string(n) + " columns; one handle takes fewer than 2^31");
  if (int32_t rc = shard_ids_ok(shard_ids, n_shards, "extract")) return rc;
  if (!ctx) return fail(FBK_E_INVALID, "NULL argument");
  // the slot of every column in ascending order; duplicates and foreign shards are errors
  std::vector<uint32_t> order(n);
  for (uint64_t k = 0; k < n; ++k) order[k] = uint32_t(k);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return columns[a] < columns[b]; });
  for (uint64_t k = 1; k < n; ++k)
    if (columns[order[k]] == columns[order[k - 1]]) return fail(FBK_E_INVALID, "extract: column " + std::to_string(columns[order[k]]) + " is listed twice");
  std::vector<uint64_t> bitpos(n);
  uint32_t s_first = 0;
  {
    const uint64_t* cur = shard_ids;
    for (uint64_t k = 0; k < n; ++k) {
      const uint64_t c = columns[order[k]], sh = c >> 20;
      cur = std::lower_bound(cur, shard_ids + n_shards, sh);
      if (cur == shard_ids + n_shards || *cur != sh) return fail(FBK_E_INVALID, "extract: column " + std::to_string(c) + " lies in a shard that is not in shard_ids");
      if (k == 0) s_first = uint32_t(cur - shard_ids);
      bitpos[k] = (uint64_t(cur - shard_ids) - s_first) << 20 | (c & 0xFFFFF);
      out_rank[order[k]] = uint32_t(k);
    }
  }
  std::unique_ptr<fbk_extract> h(new fbk_extract);
  h->ctx = ctx, h->n_shards = n_shards;
  if (n == 0) {
    *out = h.release();
    return FBK_OK;
  }
  const uint32_t span = uint32_t(bitpos[n - 1] >> 20) + 1;
  h->n = n, h->s_first = s_first, h->span = span;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  const uint64_t su_end = uint64_t(span) * fbk::kExtractUnits, n_words = su_end * fbk::kExtractWords;
  std::vector<uint32_t> iota(span);
  for (uint32_t i = 0; i < span; ++i) iota[i] = i;
  DevBuf rows, dpos, unit_pre, shard_tot, shard_base, carry;
  HIP_TRY(h->ids.alloc(ctx, uint64_t(n_shards) * 8));
  HIP_TRY(hipMemcpyAsync(h->ids.p, shard_ids, uint64_t(n_shards) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (int32_t rc = upload_rows(ctx, iota.data(), span, UINT32_MAX, rows)) return rc;
  HIP_TRY(dpos.alloc(ctx, n * 8));
  HIP_TRY(hipMemcpyAsync(dpos.p, bitpos.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(h->sel.alloc(ctx, n_words * 8));
  HIP_TRY(h->upre.alloc(ctx, (su_end + 1) * 4));
  HIP_TRY(unit_pre.alloc(ctx, su_end * 4));
  HIP_TRY(shard_tot.alloc(ctx, uint64_t(span) * 4));
  HIP_TRY(shard_base.alloc(ctx, (uint64_t(span) + 1) * 8));
  HIP_TRY(carry.alloc(ctx, 8));
  HIP_TRY(hipMemsetAsync(carry.p, 0, 8, ctx->stream));
  HIP_TRY(hipMemsetAsync(h->sel.p, 0, n_words * 8, ctx->stream));
  hipLaunchKernelGGL(fbk::k_extract_scatter, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, dpos.as<u64>(), u64(n), u64(n_words), h->sel.as<u64>());
  hipLaunchKernelGGL(fbk::k_extract_scan, dim3(span), dim3(1024), 0, ctx->stream, h->sel.as<uint8_t>(), rows.as<uint32_t>(), unit_pre.as<uint32_t>(),
                     shard_tot.as<uint32_t>());
  exclusive_scan_u32(ctx, shard_tot.as<uint32_t>(), span, shard_base.as<u64>(), carry.as<u64>());
  hipLaunchKernelGGL(fbk::k_extract_upre, dim3(uint32_t((su_end + 1 + 255) / 256)), dim3(256), 0, ctx->stream, unit_pre.as<uint32_t>(), shard_base.as<u64>(),
                     u64(su_end), u64(n), h->upre.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host lists above are the sources of the copies)
  *out = h.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
