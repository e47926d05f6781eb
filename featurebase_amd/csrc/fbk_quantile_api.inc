// fbk_quantile_api.inc — fbk_bsi_quantiles (the values at several ranks of an int field over exists ∩ filter) and
// fbk_bsi_percentile (Percentile(field=, nth=, filter=) replayed from such values): fbk_quantile.hip.h.  Included by fbk.hip after
// fbk_sort_api.inc.
//
// Both calls run ONE engine (quant_select): pass 0 of the radix select with no prefix gives the total N; a resolver turns what the
// caller asked for into absolute ascending ranks below N; the remaining passes carry every rank's prefix forward.  A walk densifies
// what is not dense a chunk of shards at a time, exactly as fbk_bsi_sort's.  Device scratch (fbk.h documents it):
//   2^17 (histograms) + 2^26 (the blocks' partial histograms) + the densify chunk (<= 2^28) + the row lists.

namespace {

// The ranks a call wants, known once N is: fills `ranks` (each < N, any order, repeats allowed).
using QuantResolve = std::function<int32_t(uint64_t N, std::vector<uint64_t>& ranks)>;

// vals[i] / cnts[i] = the stored value at ascending rank ranks[i] and the columns holding exactly it.  want_ranks == false: the
// count alone (one walk over exists and filter, no plane read, the resolver is not called).  Arguments are checked by the caller.
int32_t quant_select(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                     uint32_t n_shards, bool want_ranks, const QuantResolve& resolve, uint64_t* out_total, std::vector<uint64_t>& ranks,
                     std::vector<int64_t>& vals, std::vector<uint64_t>& cnts) {
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  const uint32_t depth = want_ranks ? bit_depth : 0;  // the count alone: the key of every column is the bias

  // the key (fbk_sort.hip.h): ascending, stored zeros take part
  fbk::SortKey sk{};
  const bool wide = depth >= 63;
  const uint32_t nbits = wide ? 64 : depth + 1;
  sk.flip = wide ? 1ull << 63 : 0, sk.bias = wide ? 0 : 1ull << depth;
  sk.desc = 0, sk.keep_zero = 1;
  const uint32_t passes = (nbits + fbk::kSortDigitBits - 1) / fbk::kSortDigitBits;
  constexpr uint32_t P = fbk::kQuantPrefixes, B = fbk::kSortBins;

  DenseOperands ops;
  const int kF = ops.add(filter, rows_f, 1), kS = ops.add(bsi, base_rows, depth + 2, true);
  const uint32_t chunk = even_chunk(n_shards, kExtractScratch, kDenseRowBytes * ops.densified_rows());
  DevBuf hist, part;
  if (int32_t rc = ops.upload(ctx, n_shards, chunk)) return rc;
  HIP_TRY(hist.alloc(ctx, uint64_t(P) * B * 8));
  HIP_TRY(part.alloc(ctx, uint64_t(fbk::kQuantHistBlocks) * P * B * 4));
  std::vector<uint64_t> hh(uint64_t(P) * B);

  // one walk over the shards for the prefixes pre[0 .. n_pre) (n_pre == 0: none yet); hh[j * 2048 + d] = the counts
  auto walk = [&](uint32_t shift, const fbk::QuantPrefixes& pre, uint32_t n_pre) -> int32_t {
    const uint32_t n_bins = (n_pre ? n_pre : 1) * B;
    HIP_TRY(hipMemsetAsync(hist.p, 0, uint64_t(n_bins) * 8, ctx->stream));
    for (uint32_t s0 = 0; s0 < n_shards; s0 += chunk) {
      const uint32_t ns = std::min(chunk, n_shards - s0);
      ops.densify_one(ctx, kF, s0, ns);  // (a launch each: the filter's rows, then the field's)
      ops.densify_one(ctx, kS, s0, ns);
      const DenseView S = ops.view(kS, s0), F = ops.view(kF, s0);
      const uint32_t nb = std::min(extract_grid(uint64_t(ns) * fbk::kExtractUnits), fbk::kQuantHistBlocks);
      hipLaunchKernelGGL(fbk::k_quant_hist, dim3(nb), dim3(256), n_bins * 4, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, depth, sk, shift, pre, n_pre,
                         part.as<uint32_t>());
      hipLaunchKernelGGL(fbk::k_quant_hist_sum, dim3(n_bins / 256, 32), dim3(256), 0, ctx->stream, part.as<uint32_t>(), nb, n_bins, hist.as<u64>());
    }
    HIP_TRY(hipGetLastError());
    D2H back(ctx);
    HIP_TRY(back.add(hh.data(), hist.p, uint64_t(n_bins) * 8));
    HIP_TRY(back.finish());
    ctx->h_stage_used = 0;  // (row lists and histograms have left the staging area)
    return FBK_OK;
  };

  // a distinct rank on its way down the digits
  struct Target {
    uint64_t want;    // its rank among the columns of its prefix
    uint64_t prefix;  // the key's digits so far
    uint64_t count;   // columns in its bin of the last pass
  };
  std::vector<Target> tg;
  std::vector<uint32_t> of;  // ranks[i] is target of[i]
  // the bin of histogram h that holds rank t.want; rank and prefix move on
  auto descend = [&](Target& t, const uint64_t* h) {
    uint64_t before = 0;
    uint32_t b = 0;
    while (b + 1 < B && before + h[b] <= t.want) before += h[b++];
    t.want -= before, t.prefix = (t.prefix << fbk::kSortDigitBits) | b, t.count = h[b];
  };

  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t shift = fbk::kSortDigitBits * (passes - 1 - p);
    if (p == 0) {
      if (int32_t rc = walk(shift, fbk::QuantPrefixes{}, 0)) return rc;
      uint64_t total = 0;
      for (uint32_t d = 0; d < B; ++d) total += hh[d];
      *out_total = total;
      if (!want_ranks || total == 0) return FBK_OK;
      if (int32_t rc = resolve(total, ranks)) return rc;
      // the distinct ranks, ascending
      std::vector<uint64_t> uniq(ranks);
      std::sort(uniq.begin(), uniq.end());
      uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
      of.resize(ranks.size());
      for (size_t i = 0; i < ranks.size(); ++i) of[i] = uint32_t(std::lower_bound(uniq.begin(), uniq.end(), ranks[i]) - uniq.begin());
      tg.reserve(uniq.size());
      for (uint64_t r : uniq) tg.push_back({r, 0, 0});
      if (tg.empty()) return FBK_OK;
      for (Target& t : tg) descend(t, hh.data());
      continue;
    }
    // ascending ranks keep ascending prefixes: the distinct ones are runs of tg
    for (size_t a = 0; a < tg.size();) {
      fbk::QuantPrefixes pre{};
      uint32_t n_pre = 0;
      size_t e = a;
      while (e < tg.size() && (n_pre < P || tg[e].prefix == pre.p[n_pre - 1])) {
        if (n_pre == 0 || tg[e].prefix != pre.p[n_pre - 1]) pre.p[n_pre++] = tg[e].prefix;
        ++e;
      }
      if (int32_t rc = walk(shift, pre, n_pre)) return rc;
      uint32_t j = 0;
      for (size_t k = a; k < e; ++k) {
        while (pre.p[j] != tg[k].prefix) ++j;
        descend(tg[k], hh.data() + uint64_t(j) * B);
      }
      a = e;
    }
  }
  vals.resize(ranks.size());
  cnts.resize(ranks.size());
  for (size_t i = 0; i < ranks.size(); ++i) {
    const Target& t = tg[of[i]];
    vals[i] = int64_t((t.prefix - sk.bias) ^ sk.flip);  // sort_value with desc = 0
    cnts[i] = t.count;
  }
  return FBK_OK;
}

// the argument checks the two calls share (fbk_bsi_sort's conventions)
int32_t quant_args_ok(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                      uint32_t n_shards) {
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (n_shards > (1u << 20)) return fail(FBK_E_INVALID, "quantiles: at most 2^20 shards per call");
  if (!ctx || !bsi || (n_shards && !base_rows) || (filter && n_shards && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, bsi->n_rows)) return rc;
  if (filter)
    if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "quantiles filter")) return rc;
  return FBK_OK;
}

// Percentile of the value + base order statistics: executor.go:1411-1585 with "leftCount > desiredLess" restated as s[L] < guess and
// "rightCount > desiredGreater" as s[N-1-G] > guess.  has_a / has_b: L / G is below N (else the count can never exceed it).
void percentile_replay(int64_t mn, uint64_t mn_count, int64_t mx, uint64_t mx_count, bool has_a, int64_t a, bool has_b, int64_t b, uint64_t L, uint64_t G,
                       int64_t* out_value, uint64_t* out_count) {
  if (G != 0 && L == 0) {
    *out_value = mn, *out_count = mn_count;
    return;
  }
  if (G == 0) {
    *out_value = mx, *out_count = mx_count;
    return;
  }
  int64_t lo = mn, hi = mx, guess = mn;
  while (lo < hi) {
    guess = (lo / 2) + (hi / 2) + (((lo % 2) + (hi % 2)) / 2);  // average without overflow (:1497-1501)
    if (has_a && a < guess) {
      hi = guess - 1;
      continue;
    }
    if (has_b && b > guess) {
      lo = guess + 1;
      continue;
    }
    break;
  }
  *out_value = guess, *out_count = 1;
}

}  // namespace

extern "C" {

int32_t fbk_bsi_quantiles(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                          uint32_t n_shards, const uint64_t* ranks, uint32_t n_ranks, int64_t* out_values, uint64_t* out_counts, uint64_t* out_total) try {
  FBK_ENTER(ctx);
  if (!out_total || (n_ranks && (!ranks || !out_values || !out_counts))) return fail(FBK_E_INVALID, "NULL argument");
  *out_total = 0;
  if (n_ranks > 1024) return fail(FBK_E_INVALID, "quantiles: at most 1024 ranks per call");
  if (int32_t rc = quant_args_ok(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards)) return rc;
  for (uint32_t i = 0; i < n_ranks; ++i) out_values[i] = 0, out_counts[i] = 0;
  if (n_shards == 0) return FBK_OK;
  std::vector<uint32_t> slot;  // the rank list's entry i is output slot[i]
  std::vector<uint64_t> abs;
  std::vector<int64_t> vals;
  std::vector<uint64_t> cnts;
  const QuantResolve resolve = [&](uint64_t N, std::vector<uint64_t>& out) {
    for (uint32_t i = 0; i < n_ranks; ++i) {
      const uint64_t k = ranks[i] & ~uint64_t(FBK_RANK_FROM_TOP);
      if (k >= N) continue;  // no such rank: (0, 0)
      out.push_back((ranks[i] & FBK_RANK_FROM_TOP) ? N - 1 - k : k);
      slot.push_back(i);
    }
    return FBK_OK;
  };
  if (int32_t rc = quant_select(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards, n_ranks != 0, resolve, out_total, abs, vals, cnts)) return rc;
  for (size_t i = 0; i < vals.size(); ++i) out_values[slot[i]] = vals[i], out_counts[slot[i]] = cnts[i];
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_percentile(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                           uint32_t n_shards, int64_t base, const double* nth, uint32_t n_nth, int64_t* out_values, uint64_t* out_counts,
                           uint64_t* out_total) try {
  FBK_ENTER(ctx);
  if (!out_total || (n_nth && (!nth || !out_values || !out_counts))) return fail(FBK_E_INVALID, "NULL argument");
  *out_total = 0;
  if (n_nth > 256) return fail(FBK_E_INVALID, "percentile: at most 256 nth values per call");
  for (uint32_t i = 0; i < n_nth; ++i)
    if (!(nth[i] >= 0.0 && nth[i] <= 100.0))  // (NaN fails both)
      return fail(FBK_E_INVALID, "Percentile(): invalid nth value, should be a number between 0 and 100 inclusive");
  if (int32_t rc = quant_args_ok(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards)) return rc;
  for (uint32_t i = 0; i < n_nth; ++i) out_values[i] = 0, out_counts[i] = 0;
  if (n_shards == 0) return FBK_OK;
  // ranks 0 and N - 1, then per nth that reaches the loop L and N - 1 - G where they exist
  struct Need {
    uint64_t L, G;
    int32_t a = -1, b = -1;  // their places in the rank list
  };
  std::vector<Need> need(n_nth);
  std::vector<uint64_t> abs;
  std::vector<int64_t> vals;
  std::vector<uint64_t> cnts;
  const QuantResolve resolve = [&](uint64_t N, std::vector<uint64_t>& out) {
    out.push_back(0);
    out.push_back(N - 1);
    for (uint32_t i = 0; i < n_nth; ++i) {
      // the two IEEE operations of executor.go:1408-1409 each, in statements of their own (a product then a quotient: nothing
      // a compiler could contract)
      double less = double(N) * nth[i];
      less = less / 100.0;
      double more = double(N) * (100 - nth[i]);
      more = more / 100.0;
      Need& nd = need[i];
      nd.L = uint64_t(less), nd.G = uint64_t(more);
      if (nd.G == 0 || nd.L == 0) continue;  // the maximum, or the minimum
      if (nd.L < N) nd.a = int32_t(out.size()), out.push_back(nd.L);
      if (nd.G < N) nd.b = int32_t(out.size()), out.push_back(N - 1 - nd.G);
    }
    return FBK_OK;
  };
  if (int32_t rc = quant_select(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards, n_nth != 0, resolve, out_total, abs, vals, cnts)) return rc;
  if (vals.empty()) return FBK_OK;  // N == 0 (the median of nothing is NULL), or nothing asked
  int64_t mn, mx;
  if (__builtin_add_overflow(vals[0], base, &mn) || __builtin_add_overflow(vals[1], base, &mx))
    return fail(FBK_E_INVALID, "percentile: minimum + base or maximum + base is outside int64");
  for (uint32_t i = 0; i < n_nth; ++i) {
    const Need& nd = need[i];
    percentile_replay(mn, cnts[0], mx, cnts[1], nd.a >= 0, nd.a >= 0 ? vals[nd.a] + base : 0, nd.b >= 0, nd.b >= 0 ? vals[nd.b] + base : 0, nd.L, nd.G,
                      &out_values[i], &out_counts[i]);
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
