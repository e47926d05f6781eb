// fbk_group_quantile_api.inc — fbk_count_matrix_quantiles: GroupBy with a percentile of an int field for all (A row, B row) groups in
// one call (fbk_group_quantile.hip.h).  Included by fbk.hip after fbk_quantile_api.inc; the argument checks of the operands are
// fbk_count_matrix_sum's (msum_args_ok).
//
// The kernels read dense rows through GroupFieldOperands (fbk_group_field.inc), a chunk of shards at a time; the path, the digits, the passes, the scratch
// bound and the chunk are fbk_group_quantile_plan.h's rules.  (fbk.h documents the arithmetic: the tests rely on it.)  A pass is a
// memset of the histograms, one histogram launch per chunk and k_gquant_resolve; nothing comes back to the host between the passes:
// the call synchronises once.  With more than one chunk every pass densifies every chunk again.

#include "fbk_group_quantile_plan.h"

extern "C" {

int32_t fbk_count_matrix_quantiles(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                   const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                   const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                                   const uint32_t* q_num, const uint32_t* q_den, uint32_t n_q, uint32_t flags, int64_t* out_values,
                                   uint64_t* out_counts, uint64_t* out_totals) try {
  FBK_ENTER(ctx);
  namespace gp = fbk_gquant_plan;
  // (what the values alone decide comes first: a caller without a device gets the message of its mistake)
  if (n_q > gp::kMaxRequests) return fail(FBK_E_INVALID, "count_matrix_quantiles: at most 16 requests per call");
  if (n_q && (!q_num || !q_den || !out_values || !out_counts)) return fail(FBK_E_INVALID, "NULL argument");
  for (uint32_t q = 0; q < n_q; ++q)
    if (q_den[q] == 0 || q_den[q] > gp::kMaxDen || q_num[q] > q_den[q])
      return fail(FBK_E_INVALID, "count_matrix_quantiles: a request is num / den with 1 <= den <= 2^20 and num <= den");
  if (flags > FBK_GQUANT_GLOBAL) return fail(FBK_E_INVALID, "count_matrix_quantiles: unknown flags");
  if (!ctx || !a || !out_totals) return fail(FBK_E_INVALID, "NULL argument");
  const GroupFieldArgs args{a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards};
  if (int32_t rc = msum_args_ok(args)) return rc;
  if (n_shards > (1u << 20)) return fail(FBK_E_INVALID, "count_matrix_quantiles: at most 2^20 shards per call");
  const uint32_t path = gp::path(n_a, n_b, n_q, flags);
  if (!path)
    return fail(FBK_E_INVALID, "count_matrix_quantiles: FBK_GQUANT_LDS takes at most " + std::to_string(gp::lds_pairs_cap()) + " histograms (n_a * n_b * max(1, n_q))");
  const uint32_t dbits = gp::digit_bits(path), bins = 1u << dbits;
  if (gp::scratch_bytes(n_a, n_b, n_q, dbits) > gp::kScratchBound)
    return fail(FBK_E_INVALID, "count_matrix_quantiles: the histograms of n_a * n_b * max(1, n_q) = " + std::to_string(gp::pairs_of(n_a, n_b, n_q)) +
                                   " (group, request) pairs exceed 2^30 bytes: block the leading field (fewer A rows per call)");
  const uint64_t width = uint64_t(n_a) * n_b, nq1 = std::max<uint32_t>(1, n_q), pairs = width * nq1, answers = width * n_q;
  std::memset(out_totals, 0, width * 8);
  if (n_q) std::memset(out_values, 0, answers * 8), std::memset(out_counts, 0, answers * 8);
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;

  const uint32_t depth = n_q ? bit_depth : 0;  // n_q == 0: the totals alone, no plane is read (the kernels build the key from the depth)
  const uint32_t passes = gp::passes(depth, dbits);

  GroupFieldOperands gf;
  gf.add(args, depth);
  const uint32_t chunk = gp::densify_chunk(n_shards, gf.ops.densified_rows());
  if (int32_t rc = gf.upload(ctx, chunk)) return rc;
  DevBuf hist, slots, result, reqs, part;  // result: totals [width], values [answers], counts [answers]
  HIP_TRY(hist.alloc(ctx, pairs * bins * 8));
  HIP_TRY(slots.alloc(ctx, pairs * sizeof(fbk::GquantSlot)));
  HIP_TRY(result.alloc(ctx, (width + 2 * answers) * 8));
  u64* d_totals = result.as<u64>();
  long long* d_values = reinterpret_cast<long long*>(d_totals + width);
  u64* d_counts = d_totals + width + answers;
  const uint32_t* d_req[2] = {nullptr, nullptr};
  if (n_q)
    if (int32_t rc = upload_rows_multi(ctx, {{q_num, n_q, UINT32_MAX}, {q_den, n_q, UINT32_MAX}}, reqs, d_req)) return rc;
  const auto lds_grid = [&](uint32_t ns) { return std::min(gf.walk_grid(ns), gp::kLdsBlocks); };
  if (path == gp::kLds) HIP_TRY(part.alloc(ctx, uint64_t(lds_grid(chunk)) * pairs * bins * 4));
  {
    KernelSpan span(ctx);
    for (uint32_t p = 0; p < passes; ++p) {
      const uint32_t shift = gp::pass_low(depth, dbits, p), wbits = gp::pass_width(depth, dbits, p), n_h = p ? n_q : 0;
      const uint64_t n_bins = (p ? pairs : width) * bins;  // (the LDS path: at most 64 KiB / 4)
      HIP_TRY(hipMemsetAsync(hist.p, 0, n_bins * 8, ctx->stream));
      gf.for_each_chunk(ctx, p == 0, [&](const GroupFieldViews& v, uint32_t, uint32_t ns) {
        if (path == gp::kLds) {
          const uint32_t nb = lds_grid(ns);
          gf.launch(fbk::k_gquant_hist_lds, nb, n_bins * 4, ctx, v, ns, shift, wbits, dbits, n_h, slots.as<fbk::GquantSlot>(), uint32_t(n_bins), part.as<uint32_t>());
          hipLaunchKernelGGL(fbk::k_quant_hist_sum, dim3(uint32_t(n_bins / 256), 32), dim3(256), 0, ctx->stream, part.as<uint32_t>(), nb, uint32_t(n_bins),
                             hist.as<u64>());
        } else {
          gf.launch(fbk::k_gquant_hist_global, gf.walk_grid(ns), 0, ctx, v, ns, shift, wbits, dbits, n_h, slots.as<fbk::GquantSlot>(), hist.as<u64>());
        }
      });
      hipLaunchKernelGGL(fbk::k_gquant_resolve, dim3(uint32_t((pairs + 3) / 4)), dim3(256), 0, ctx->stream, hist.as<u64>(), uint32_t(width), n_q, dbits, wbits, int(p == 0),
                         int(p + 1 == passes), d_req[0], d_req[1], depth, slots.as<fbk::GquantSlot>(), d_totals, d_values, d_counts);
    }
  }
  HIP_TRY(hipGetLastError());
  D2H back(ctx);
  HIP_TRY(back.add(out_totals, d_totals, width * 8));
  if (n_q) {
    HIP_TRY(back.add(out_values, d_values, answers * 8));
    HIP_TRY(back.add(out_counts, d_counts, answers * 8));
  }
  HIP_TRY(back.finish());  // the call's one synchronisation
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
