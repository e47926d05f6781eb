// fbk_group_select_api.inc — GroupBy's having / sort / offset / limit on the device: fbk_count_matrix_select, fbk_count_cube_select,
// fbk_count_matrix_sum_select (the selection between the full calls' *_enqueue and *_read) and fbk_select_groups (the stage alone):
// fbk_group_select.hip.h, rules in fbk_group_select_plan.h.  Included by fbk.hip after fbk_count_cube_api.inc.
//
// Device scratch of the stage (fbk.h documents it), U = ceil(n / 512) units, W the cells that are sorted, n_out the records:
//   16 (U + 1) (unit counts and their scan) + the scan's temporary storage + 20 n_out (the records), and with a sort
//   4 matched (the matched cells) + 4 W + 16 W (sorted cells, keys in and out) + the radix sort's temporary storage
//   + (K < matched) 4 K (the winners) + 1 KiB (histogram) + 32 (state).

namespace {

// the checks every selecting call makes before any launch; *out_n = *out_matched = 0
int32_t group_select_args_ok(const fbk_groupby_select* sel, bool has_agg, const uint32_t* out_cells, const uint64_t* out_counts, const int64_t* out_aggs,
                             uint64_t cap, uint64_t* out_n, uint64_t* out_matched) {
  if (!sel || !out_n || !out_matched || (cap && (!out_cells || !out_counts || (has_agg && !out_aggs)))) return fail(FBK_E_INVALID, "NULL argument");
  *out_n = 0, *out_matched = 0;
  if (const char* what = fbk_group_select::check(sel, has_agg)) return fail(FBK_E_INVALID, std::string("groupby select: ") + what);
  return FBK_OK;
}

int32_t group_select_capacity_ok(uint64_t want, uint64_t cap, uint64_t* out_n) {
  *out_n = want;
  if (want > cap) return fail(FBK_E_CAPACITY, "groupby select: " + std::to_string(want) + " records, capacity " + std::to_string(cap));
  return FBK_OK;
}

// The host path: the totals come down, fbk_group_select::select orders them.
int32_t group_select_host(const uint64_t* counts, const int64_t* aggs, uint64_t n, const fbk_groupby_select& sel, uint32_t* out_cells, uint64_t* out_counts,
                          int64_t* out_aggs, uint64_t cap, uint64_t* out_n, uint64_t* out_matched) {
  std::vector<uint32_t> cells;
  *out_matched = fbk_group_select::select(counts, aggs, n, sel, cells);
  if (int32_t rc = group_select_capacity_ok(cells.size(), cap, out_n)) return rc;
  for (size_t k = 0; k < cells.size(); ++k) {
    out_cells[k] = cells[k];
    out_counts[k] = counts[cells[k]];
    if (aggs && out_aggs) out_aggs[k] = aggs[cells[k]];
  }
  return FBK_OK;
}

// The buffers of the ordered compactions of one call (fbk_group_select.hip.h): unit counts, their exclusive scan, the scan's scratch.
// cnt / pre hold 2 * (units + 1) words each: {class A counts, 0, class B counts, 0}, so that ONE scan gives both classes' ranks and totals.
struct GsScan {
  DevBuf cnt, pre, tmp;
  size_t tmp_bytes = 0;
  hipError_t alloc(fbk_ctx* ctx, uint32_t units) {
    const uint64_t words = 2 * (uint64_t(units) + 1);
    hipError_t e = cnt.alloc(ctx, words * 4);
    if (e == hipSuccess) e = pre.alloc(ctx, words * 4);
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt.as<uint32_t>(), pre.as<uint32_t>(), int(words), ctx->stream);
    if (e == hipSuccess) e = tmp.alloc(ctx, std::max<size_t>(tmp_bytes, 16));
    return e;
  }
};

template <fbk::GsMode MODE>
int32_t group_select_count_scan(fbk_ctx* ctx, GsScan& s, const u64* counts, const long long* aggs, const uint32_t* list, uint32_t n, const fbk::GsRules& r,
                                const fbk::GsState* state) {
  const uint32_t units = (n + fbk::kGsUnit - 1) / fbk::kGsUnit;
  const uint32_t words = (MODE == fbk::kGsBelow ? 2 : 1) * (units + 1);
  HIP_TRY(hipMemsetAsync(s.cnt.p, 0, uint64_t(words) * 4, ctx->stream));  // (the zero behind each class's counts: its total lands there)
  hipLaunchKernelGGL((fbk::k_gs_count<MODE>), dim3((units + 3) / 4), dim3(256), 0, ctx->stream, counts, aggs, list, n, r, state, units, s.cnt.as<uint32_t>());
  size_t tb = s.tmp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.tmp.p, tb, s.cnt.as<uint32_t>(), s.pre.as<uint32_t>(), int(words), ctx->stream));
  return FBK_OK;
}

template <fbk::GsMode MODE>
void group_select_emit(fbk_ctx* ctx, GsScan& s, const u64* counts, const long long* aggs, const uint32_t* list, uint32_t n, const fbk::GsRules& r,
                       const fbk::GsState* state, uint32_t lo, uint32_t end, uint32_t cap, uint32_t* out) {
  const uint32_t units = (n + fbk::kGsUnit - 1) / fbk::kGsUnit;
  hipLaunchKernelGGL((fbk::k_gs_emit<MODE>), dim3((units + 3) / 4), dim3(256), 0, ctx->stream, counts, aggs, list, n, r, state, units, s.pre.as<uint32_t>(), lo, end,
                     cap, out);
}

// The stage over totals on the device (this context's stream; the caller holds ctx->mu): d_counts[n], d_aggs[n] or nullptr,
// 0 < n <= 2^24, `sel` checked.  Synchronises the stream.
int32_t group_select_locked(fbk_ctx* ctx, const u64* d_counts, const long long* d_aggs, uint64_t n64, const fbk_groupby_select& sel, uint32_t* out_cells,
                            uint64_t* out_counts, int64_t* out_aggs, uint64_t cap, uint64_t* out_n, uint64_t* out_matched) {
  bool device = n64 > fbk_group_select::kHostCells;
  if (sel.flags & FBK_GROUPSEL_DEVICE) device = true;
  if (sel.flags & FBK_GROUPSEL_HOST) device = false;
  if (!device) {
    std::vector<uint64_t> hc(n64);
    std::vector<int64_t> ha(d_aggs ? n64 : 0);
    D2H back(ctx);
    HIP_TRY(back.add(hc.data(), d_counts, n64 * 8));
    if (d_aggs) HIP_TRY(back.add(ha.data(), d_aggs, n64 * 8));
    HIP_TRY(back.finish());
    return group_select_host(hc.data(), d_aggs ? ha.data() : nullptr, n64, sel, out_cells, out_counts, out_aggs, cap, out_n, out_matched);
  }
  const uint32_t n = uint32_t(n64);
  const fbk::GsRules r = fbk_group_select::rules_of(sel);
  const uint32_t units = (n + fbk::kGsUnit - 1) / fbk::kGsUnit;
  GsScan scan;
  HIP_TRY(scan.alloc(ctx, units));

  // the groups: counted, then — once the window is known — written in ascending cell order
  if (int32_t rc = group_select_count_scan<fbk::kGsMatched>(ctx, scan, d_counts, d_aggs, nullptr, n, r, nullptr)) return rc;
  HIP_TRY(hipGetLastError());
  uint32_t matched = 0;
  HIP_TRY(hipMemcpyAsync(&matched, scan.pre.as<uint32_t>() + units, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *out_matched = matched;
  const fbk_group_select::Window w = fbk_group_select::window(matched, sel.offset, sel.limit);
  if (int32_t rc = group_select_capacity_ok(w.n(), cap, out_n)) return rc;
  if (w.n() == 0) return FBK_OK;
  const uint32_t lo = uint32_t(w.lo), K = uint32_t(w.end), n_out = K - lo;

  DevBuf cells, winners, sorted, kin, kout, tmp, state, hist, ocounts, oaggs;
  const uint32_t* result = nullptr;  // the cells of the result, in order, on the device
  if (r.n_sort == 0) {
    HIP_TRY(cells.alloc(ctx, uint64_t(n_out) * 4));
    group_select_emit<fbk::kGsMatched>(ctx, scan, d_counts, d_aggs, nullptr, n, r, nullptr, lo, K, n_out, cells.as<uint32_t>());
    result = cells.as<uint32_t>();
  } else {
    HIP_TRY(cells.alloc(ctx, uint64_t(matched) * 4));
    group_select_emit<fbk::kGsMatched>(ctx, scan, d_counts, d_aggs, nullptr, n, r, nullptr, 0, matched, matched, cells.as<uint32_t>());
    uint32_t* order = cells.as<uint32_t>();  // what is sorted: W cells, ties in ascending cell order
    uint32_t W = matched;
    if (K < matched) {
      // the key T of rank K among the matched cells, MSB first; then the cells below it and the first ties
      HIP_TRY(state.alloc(ctx, sizeof(fbk::GsState)));
      HIP_TRY(hist.alloc(ctx, fbk::kGsBins * 4));
      fbk::GsState* st = state.as<fbk::GsState>();
      const fbk::GsState st0{{0, 0}, K, 0};
      HIP_TRY(hipMemcpyAsync(st, &st0, sizeof st0, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(hipMemsetAsync(hist.p, 0, fbk::kGsBins * 4, ctx->stream));
      const uint32_t hb = std::min<uint32_t>((matched + 255) / 256, fbk::kGsHistBlocks);
      for (uint32_t word = 0; word < r.n_sort; ++word)
        for (int shift = 56; shift >= 0; shift -= 8) {
          hipLaunchKernelGGL(fbk::k_gs_hist, dim3(hb), dim3(256), 0, ctx->stream, d_counts, d_aggs, order, matched, r, st, word, uint32_t(shift), hist.as<uint32_t>());
          hipLaunchKernelGGL(fbk::k_gs_pick, dim3(1), dim3(256), 0, ctx->stream, hist.as<uint32_t>(), st, word, uint32_t(shift));
        }
      HIP_TRY(hipStreamSynchronize(ctx->stream));  // (st0 is the source of a copy)
      HIP_TRY(winners.alloc(ctx, uint64_t(K) * 4));
      if (int32_t rc = group_select_count_scan<fbk::kGsBelow>(ctx, scan, d_counts, d_aggs, order, matched, r, st)) return rc;
      group_select_emit<fbk::kGsBelow>(ctx, scan, d_counts, d_aggs, order, matched, r, st, 0, K, K, winners.as<uint32_t>());
      order = winners.as<uint32_t>(), W = K;
    }
    // stable radix sorts, the last term first: equal keys keep the order they came in
    size_t t_sort = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, static_cast<const u64*>(nullptr), static_cast<u64*>(nullptr), static_cast<const uint32_t*>(nullptr),
                                               static_cast<uint32_t*>(nullptr), int(W), 0, 64, ctx->stream));
    HIP_TRY(tmp.alloc(ctx, std::max<size_t>(t_sort, 16)));
    HIP_TRY(sorted.alloc(ctx, uint64_t(W) * 4));
    HIP_TRY(kin.alloc(ctx, uint64_t(W) * 8));
    HIP_TRY(kout.alloc(ctx, uint64_t(W) * 8));
    uint32_t *from = order, *to = sorted.as<uint32_t>();
    for (uint32_t t = r.n_sort; t-- > 0;) {
      hipLaunchKernelGGL(fbk::k_gs_keys, dim3((W + 255) / 256), dim3(256), 0, ctx->stream, d_counts, d_aggs, from, W, r, t, kin.as<u64>());
      size_t tb = t_sort;
      HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, kin.as<u64>(), kout.as<u64>(), from, to, int(W), 0, 64, ctx->stream));
      std::swap(from, to);
    }
    result = from + lo;
  }
  HIP_TRY(ocounts.alloc(ctx, uint64_t(n_out) * 8));
  if (d_aggs) HIP_TRY(oaggs.alloc(ctx, uint64_t(n_out) * 8));
  hipLaunchKernelGGL(fbk::k_gs_records, dim3((n_out + 255) / 256), dim3(256), 0, ctx->stream, d_counts, d_aggs, result, n_out, ocounts.as<u64>(),
                     oaggs.as<long long>());
  HIP_TRY(hipGetLastError());
  D2H back(ctx);
  HIP_TRY(back.add(out_cells, result, uint64_t(n_out) * 4));
  HIP_TRY(back.add(out_counts, ocounts.p, uint64_t(n_out) * 8));
  if (d_aggs && out_aggs) HIP_TRY(back.add(out_aggs, oaggs.p, uint64_t(n_out) * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_count_matrix_select(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b,
                                const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, const fbk_groupby_select* sel, uint32_t* out_cells,
                                uint64_t* out_counts, uint64_t cap, uint64_t* out_n, uint64_t* out_matched) try {
  FBK_ENTER(ctx);
  if (!ctx) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = group_select_args_ok(sel, false, out_cells, out_counts, nullptr, cap, out_n, out_matched)) return rc;
  if (int32_t rc = count_matrix_args_ok(a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  const uint64_t width = uint64_t(n_a) * n_b;
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  MatrixPlan p;
  DevBuf dtot;
  HIP_TRY(dtot.alloc(ctx, width * 8));
  if (int32_t rc = matrix_prepare(ctx, p, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards, false)) return rc;
  if (int32_t rc = matrix_enqueue(ctx, p, dtot.as<u64>(), false)) return rc;
  return group_select_locked(ctx, dtot.as<u64>(), nullptr, width, *sel, out_cells, out_counts, nullptr, cap, out_n, out_matched);
} FBK_ABI_CATCH(ctx)

int32_t fbk_count_cube_select(fbk_ctx* ctx, const fbk_batch* p, const uint32_t* rows_p, uint32_t n_p, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a,
                              const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards,
                              const fbk_groupby_select* sel, uint32_t* out_cells, uint64_t* out_counts, uint64_t cap, uint64_t* out_n,
                              uint64_t* out_matched) try {
  FBK_ENTER(ctx);
  if (!ctx) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = group_select_args_ok(sel, false, out_cells, out_counts, nullptr, cap, out_n, out_matched)) return rc;
  if (int32_t rc = cube_args_ok(p, rows_p, n_p, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  const uint64_t cells = uint64_t(n_p) * n_a * n_b;
  if (n_shards == 0 || cells == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  CubePlan c;
  if (int32_t rc = cube_prepare(ctx, c, p, rows_p, n_p, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  if (int32_t rc = cube_enqueue(ctx, c)) return rc;
  return group_select_locked(ctx, c.result.as<u64>(), nullptr, cells, *sel, out_cells, out_counts, nullptr, cap, out_n, out_matched);
} FBK_ABI_CATCH(ctx)

int32_t fbk_count_matrix_sum_select(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                                    uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, const fbk_batch* bsi, const uint32_t* base_rows,
                                    uint32_t bit_depth, uint32_t n_shards, const fbk_groupby_select* sel, uint32_t* out_cells, uint64_t* out_counts,
                                    int64_t* out_aggs, uint64_t cap, uint64_t* out_n, uint64_t* out_matched) try {
  FBK_ENTER(ctx);
  if (!ctx || !a) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = group_select_args_ok(sel, true, out_cells, out_counts, out_aggs, cap, out_n, out_matched)) return rc;
  const GroupFieldArgs args{a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards};
  if (int32_t rc = msum_args_ok(args)) return rc;
  const uint64_t width = args.width();
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  MsumPlan p;
  if (int32_t rc = msum_prepare(ctx, p, args)) return rc;
  if (int32_t rc = msum_enqueue(ctx, p)) return rc;
  // p.result = {sums [width], counts [width]}
  return group_select_locked(ctx, p.result.as<u64>() + width, p.result.as<long long>(), width, *sel, out_cells, out_counts, out_aggs, cap, out_n, out_matched);
} FBK_ABI_CATCH(ctx)

int32_t fbk_select_groups(fbk_ctx* ctx, const uint64_t* counts, const int64_t* aggs, uint64_t n, const fbk_groupby_select* sel, uint32_t* out_cells,
                          uint64_t* out_counts, int64_t* out_aggs, uint64_t cap, uint64_t* out_n, uint64_t* out_matched) try {
  FBK_ENTER(ctx);
  if (!ctx || (n && !counts)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = group_select_args_ok(sel, aggs != nullptr, out_cells, out_counts, out_aggs, cap, out_n, out_matched)) return rc;
  if (n > fbk_group_select::kMaxCells) return fail(FBK_E_INVALID, "select_groups: at most 2^24 cells per call");
  if (n == 0) return FBK_OK;
  const bool device = (sel->flags & FBK_GROUPSEL_DEVICE) || (!(sel->flags & FBK_GROUPSEL_HOST) && n > fbk_group_select::kHostCells);
  if (!device) return group_select_host(counts, aggs, n, *sel, out_cells, out_counts, out_aggs, cap, out_n, out_matched);  // (nothing to upload)
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  DevBuf dc, da;
  HIP_TRY(dc.alloc(ctx, n * 8));
  HIP_TRY(hipMemcpyAsync(dc.p, counts, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (aggs) {
    HIP_TRY(da.alloc(ctx, n * 8));
    HIP_TRY(hipMemcpyAsync(da.p, aggs, n * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  return group_select_locked(ctx, dc.as<u64>(), aggs ? da.as<long long>() : nullptr, n, *sel, out_cells, out_counts, out_aggs, cap, out_n, out_matched);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
