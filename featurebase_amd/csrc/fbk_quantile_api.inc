// fbk_quantile_api.inc — fbk_bsi_quantiles (the values at several ranks of an int field over exists ∩ filter) and
// fbk_bsi_percentile (Percentile(field=, nth=, filter=) replayed from such values): fbk_quantile.hip.h.  Included by fbk.hip after
// fbk_sort_api.inc.
//
// Both calls run ONE engine (quant_select): pass 0 of the radix select with no prefix gives the total N; a resolver turns what the
// caller asked for into absolute ascending ranks below N; the remaining passes carry every rank's prefix forward.  The host's rules
// are fbk_select_plan.h's, the operands and the walk fbk_bsi_sort's FieldOperands.  Device scratch (fbk.h documents it):
//   2^17 (histograms) + 2^26 (the blocks' partial histograms) + the densify chunk (<= 2^28) + the row lists.

namespace {

// The ranks a call wants, known once N is: fills `ranks` (each < N, any order, repeats allowed).
using QuantResolve = std::function<void(uint64_t N, std::vector<uint64_t>& ranks)>;

// vals[i] / cnts[i] = the stored value at ascending rank ranks[i] and the columns holding exactly it.  want_ranks == false: the
// count alone (one walk over exists and filter, no plane read, the resolver is not called).  Arguments are checked by the caller.
int32_t quant_select(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                     uint32_t n_shards, bool want_ranks, const QuantResolve& resolve, uint64_t* out_total, std::vector<uint64_t>& ranks,
                     std::vector<int64_t>& vals, std::vector<uint64_t>& cnts) {
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  const uint32_t depth = want_ranks ? bit_depth : 0;  // the count alone: the key of every column is the bias

  const fbk::SortKey sk = fbk::select_key(depth, false, true);  // ascending, stored zeros take part
  const uint32_t passes = fbk::passes(depth, fbk::kSortDigitBits);
  constexpr uint32_t P = fbk::kQuantPrefixes, B = fbk::kSortBins;

  FieldOperands fo;
  fo.add(bsi, base_rows, depth, filter, rows_f, n_shards);
  DevBuf hist, part;
  if (int32_t rc = fo.upload(ctx)) return rc;
  HIP_TRY(hist.alloc(ctx, uint64_t(P) * B * 8));
  HIP_TRY(part.alloc(ctx, uint64_t(fbk::kQuantHistBlocks) * P * B * 4));
  std::vector<uint64_t> hh(uint64_t(P) * B);

  // one walk over the shards for the prefixes pre[0 .. n_pre) (n_pre == 0: none yet); hh[j * 2048 + d] = the counts
  auto walk = [&](uint32_t shift, const fbk::QuantPrefixes& pre, uint32_t n_pre) -> int32_t {
    const uint32_t n_bins = (n_pre ? n_pre : 1) * B;
    HIP_TRY(hipMemsetAsync(hist.p, 0, uint64_t(n_bins) * 8, ctx->stream));
    fo.for_each_chunk(ctx, [&](const DenseView& S, const DenseView& F, uint32_t, uint32_t ns, dim3 grid) {
      const uint32_t nb = std::min(grid.x, fbk::kQuantHistBlocks);
      hipLaunchKernelGGL(fbk::k_quant_hist, dim3(nb), dim3(256), n_bins * 4, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, depth, sk, shift, pre, n_pre,
                         part.as<uint32_t>());
      hipLaunchKernelGGL(fbk::k_quant_hist_sum, dim3(n_bins / 256, 32), dim3(256), 0, ctx->stream, part.as<uint32_t>(), nb, n_bins, hist.as<u64>());
    });
    HIP_TRY(hipGetLastError());
    D2H back(ctx);
    HIP_TRY(back.add(hh.data(), hist.p, uint64_t(n_bins) * 8));
    HIP_TRY(back.finish());
    ctx->h_stage_used = 0;  // (row lists and histograms have left the staging area)
    return FBK_OK;
  };

  std::vector<sp::Target> tg;  // the distinct ranks on their way down the digits (fbk_select_plan.h)
  std::vector<uint32_t> of;    // ranks[i] is target of[i]
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t shift = fbk::kSortDigitBits * (passes - 1 - p);
    if (p == 0) {
      if (int32_t rc = walk(shift, fbk::QuantPrefixes{}, 0)) return rc;
      uint64_t total = 0;
      for (uint32_t d = 0; d < B; ++d) total += hh[d];
      *out_total = total;
      if (!want_ranks || total == 0) return FBK_OK;
      resolve(total, ranks);
      tg = sp::rank_table(ranks, of);
      if (tg.empty()) return FBK_OK;
      for (sp::Target& t : tg) sp::step(t, hh.data());
      continue;
    }
    for (size_t a = 0; a < tg.size();) {
      fbk::QuantPrefixes pre{};
      uint32_t n_pre = 0;
      const size_t e = sp::prefix_group(tg, a, pre, n_pre);
      if (int32_t rc = walk(shift, pre, n_pre)) return rc;
      uint32_t j = 0;
      for (size_t k = a; k < e; ++k) {
        while (pre.p[j] != tg[k].prefix) ++j;
        sp::step(tg[k], hh.data() + uint64_t(j) * B);
      }
      a = e;
    }
  }
  for (uint32_t o : of) vals.push_back(fbk::sort_value(tg[o].prefix, sk)), cnts.push_back(tg[o].count);
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_bsi_quantiles(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f,
                          uint32_t n_shards, const uint64_t* ranks, uint32_t n_ranks, int64_t* out_values, uint64_t* out_counts, uint64_t* out_total) try {
  FBK_ENTER(ctx);
  if (!out_total || (n_ranks && (!ranks || !out_values || !out_counts))) return fail(FBK_E_INVALID, "NULL argument");
  *out_total = 0;
  if (n_ranks > 1024) return fail(FBK_E_INVALID, "quantiles: at most 1024 ranks per call");
  if (int32_t rc = field_args_ok(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards, 1u << 20, "quantiles: at most 2^20 shards per call", "quantiles filter")) return rc;
  for (uint32_t i = 0; i < n_ranks; ++i) out_values[i] = 0, out_counts[i] = 0;
  if (n_shards == 0) return FBK_OK;
  std::vector<uint32_t> slot;  // the rank list's entry i is output slot[i]
  std::vector<uint64_t> abs, cnts;
  std::vector<int64_t> vals;
  const QuantResolve resolve = [&](uint64_t N, std::vector<uint64_t>& out) {
    for (uint32_t i = 0; i < n_ranks; ++i) {
      const uint64_t k = ranks[i] & ~uint64_t(FBK_RANK_FROM_TOP);
      if (k >= N) continue;  // no such rank: (0, 0)
      out.push_back((ranks[i] & FBK_RANK_FROM_TOP) ? N - 1 - k : k);
      slot.push_back(i);
    }
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
  if (int32_t rc = field_args_ok(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards, 1u << 20, "quantiles: at most 2^20 shards per call", "quantiles filter")) return rc;
  for (uint32_t i = 0; i < n_nth; ++i) out_values[i] = 0, out_counts[i] = 0;
  if (n_shards == 0) return FBK_OK;
  std::vector<sp::PctNeed> need;
  std::vector<uint64_t> abs, cnts;
  std::vector<int64_t> vals;
  const QuantResolve resolve = [&](uint64_t N, std::vector<uint64_t>& out) { sp::percentile_ranks(N, nth, n_nth, need, out); };
  if (int32_t rc = quant_select(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards, n_nth != 0, resolve, out_total, abs, vals, cnts)) return rc;
  if (vals.empty()) return FBK_OK;  // N == 0 (the median of nothing is NULL), or nothing asked
  if (!sp::percentile_finish(need, vals, cnts, base, out_values, out_counts))
    return fail(FBK_E_INVALID, "percentile: minimum + base or maximum + base is outside int64");
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
