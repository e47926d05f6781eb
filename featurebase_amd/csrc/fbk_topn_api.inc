// fbk_topn_api.inc — host side of the TopK / TopN family (included by fbk.hip after fbk_expr_api.inc: a call tree may be the filter): fbk_topk,
// fbk_topn, fbk_topn_partials, fbk_topk_bsi and the TopnPlan of fbk_query_topn here; fbk_group_topn (fbk_group_api.inc) and fbk_expr_row_counts /
// _topk / _topn (fbk_expr_topk_api.inc) are built from the same pieces: topn_args_ok (the limits), TopnSource (the filter), TopnBuffers (the device
// vectors, sized by fbk_topn_plan.h), topn_totals_enqueue (the passes: ONE body), TopnSort / topn_radix_enqueue / topn_order_locked (the ordering).
#include "fbk_topn_plan.h"

namespace {

int32_t topn_args_ok(uint32_t n_a, uint64_t tanimoto_threshold) {
  if (n_a > (1u << 22)) return fail(FBK_E_INVALID, "topk: at most 2^22 rows");
  if (tanimoto_threshold > 100) return fail(FBK_E_INVALID, "topn: Tanimoto threshold is a percentage (0..100)");
  return FBK_OK;
}

// The n of fragment.top's candidate pass for a TopN of n over n_a rows under the context's semantics (0: no candidate pass —
// n = 0 asks for every row, n >= n_a cannot fill any shard's heap before its rows run out, topn_semantics = 0 is exact).
inline uint32_t topn_cand_n(const fbk_ctx* ctx, uint32_t n, uint32_t n_a, bool reference_operator) {
  return (reference_operator && ctx->opt.topn_semantics == 1 && n > 0 && n < n_a) ? n : 0;
}

// The filter of the counts: none (all nullptr), a row per shard, or a call tree.
struct TopnSource {
  const fbk_batch* filter = nullptr;  // shard s of the call reads row d_rf[s] (device) of `filter`
  const uint32_t* d_rf = nullptr;
  const Slot* recs = nullptr;   // with `filter`: the FIELD's resolved records of a prepared query (query_row_records) or nullptr
  ExprProgram* tree = nullptr;  // an uploaded tree the counting kernel evaluates itself
  fbk_topn_plan::Source kind() const { return tree ? fbk_topn_plan::kTreeSource : filter ? fbk_topn_plan::kRowSource : fbk_topn_plan::kNoSource; }
};

inline fbk_topn_plan::Sizes topn_plan(const fbk_ctx* ctx, uint32_t n_a, uint32_t n_shards, const TopnSource& S, uint64_t min_threshold, uint64_t tanimoto_threshold,
                                      uint32_t cand_n, bool keep_per_shard = false, bool keep_src = false) {
  return fbk_topn_plan::plan({n_a, n_shards, S.kind(), min_threshold, tanimoto_threshold, cand_n, uint64_t(ctx->opt.matrix_pass_kb), keep_per_shard, keep_src});
}

// The device vectors of one call (of a prepared query: of every run).  The totals [n_a] and the candidate flags [n_a] are its own unless the
// caller has a place for them (a prepared query's result, a group member's reduce buffer).
struct TopnBuffers {
  fbk_topn_plan::Sizes sz;
  DevBuf shard, cards, src, tot, cand;
  u64 *d_total = nullptr, *d_cand = nullptr;
  hipError_t alloc(fbk_ctx* ctx, const fbk_topn_plan::Sizes& s, u64* ext_total = nullptr, u64* ext_cand = nullptr) {
    sz = s;
    hipError_t e = ext_total ? hipSuccess : tot.alloc(ctx, uint64_t(s.req.n_a) * 8);
    if (e == hipSuccess) e = shard.alloc(ctx, s.shard_words * 8);
    if (e == hipSuccess && s.cards_words) e = cards.alloc(ctx, s.cards_words * 8);
    if (e == hipSuccess && s.src_words) e = src.alloc(ctx, s.src_words * 8);
    if (e == hipSuccess && s.cand_words && !ext_cand) e = cand.alloc(ctx, s.cand_words * 8);
    d_total = ext_total ? ext_total : tot.as<u64>();
    d_cand = !s.cand_words ? nullptr : ext_cand ? ext_cand : cand.as<u64>();
    return e;
  }
};

// the counting launch of one pass over a call tree: shards [p0, p0 + pn) of the call, d_ra = their rows of the field, dshard [pn][n_a] zeroed by
// the caller, dsrc [pn] (zeroed) or nullptr
int32_t expr_rows_launch(fbk_ctx* ctx, ExprProgram& P, const fbk_batch* a, const uint32_t* d_ra, uint32_t n_a, uint32_t p0, uint32_t pn, u64* dshard, u64* dsrc) {
  if (int32_t rc = expr_patch_leaves(ctx, P)) return rc;
  const uint32_t rpb = fbk_expr::rows_per_block(n_a, pn, fbk_expr::operand_reads(P.plan.ins));
  const uint32_t chunks = (n_a + rpb - 1) / rpb;
  const uint32_t stack_bytes = P.plan.slots * 8192u;
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_expr_rows_vs_filter, dim3(pn * 16 * chunks), dim3(256), stack_bytes, ctx->stream, P.d_leaves(), P.d_prog(), uint32_t(P.plan.ins.size()),
                       P.plan.slots, p0, a->d_slots, a->d_arena, d_ra, n_a, pn, rpb, dshard, dsrc);
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// totals[i] = sum over the shards of the count of row i that QUALIFIES in that shard (fragment.top's rules, k_topn_filter): |row ∩ source_s| with
// a source, the stored cardinality without.  Launch only: d_ra [n_shards][n_a] is on the device, B was allocated from the plan of this call (B.sz).
// The shards go in passes of B.sz.pass_shards (executeTopKShard's per-shard counts, merged by AddBSI / Pairs.Add in the reference's reduce).  A pass:
// the counts by source; cardinalities and source counts where the rules need them (a tree's counting launch writes its own source counts);
// k_topn_candidates with cand_n > 0 (the reference's TopN with 0 < n < n_a, option topn_semantics = 1: B.d_cand [n_a] gets 1 for every row some
// shard's fragment.top(N = cand_n) would return, pass 1 of executeTopN); k_topn_filter with thresholds; k_reduce_shards into B.d_total.  Without a
// source the counts ARE the cardinalities, there is no source count and no Tanimoto rule: the same sequence.
// mask: zero the totals of the non-candidates at the end (k_topn_mask); off where the flags are reduced over several members first.
int32_t topn_totals_enqueue(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* d_ra, const TopnSource& S, TopnBuffers& B, bool mask) {
  const fbk_topn_plan::Sizes& z = B.sz;
  const uint32_t n_a = z.req.n_a, n_shards = z.req.n_shards, cand_n = z.req.cand_n;
  const u64 min_threshold = z.req.min_threshold, tanimoto = z.tanimoto;
  const bool sourced = S.tree || S.filter;
  u64* dshard = B.shard.as<u64>();
  const u64* dcards = sourced ? B.cards.as<u64>() : dshard;
  if (z.cands) HIP_TRY(hipMemsetAsync(B.d_cand, 0, uint64_t(n_a) * 8, ctx->stream));
  HIP_TRY(hipMemsetAsync(B.d_total, 0, uint64_t(n_a) * 8, ctx->stream));
  if (S.tree && z.src_words) HIP_TRY(hipMemsetAsync(B.src.p, 0, z.src_words * 8, ctx->stream));
  for (uint64_t p0 = 0; p0 < n_shards; p0 += z.pass_shards) {
    const uint32_t pn = uint32_t(std::min<uint64_t>(z.pass_shards, n_shards - p0));
    const uint32_t* ra = d_ra + p0 * n_a;
    const uint64_t n = uint64_t(pn) * n_a;
    u64* src = z.src_words ? B.src.as<u64>() + p0 : nullptr;
    if (sourced) HIP_TRY(hipMemsetAsync(dshard, 0, n * 8, ctx->stream));
    if (S.tree) {
      if (int32_t rc = expr_rows_launch(ctx, *S.tree, a, ra, n_a, uint32_t(p0), pn, dshard, src)) return rc;
    } else if (S.filter) {
      KernelSpan span(ctx);
      launch_rows_vs_filter(ctx, a, ra, n_a, S.filter, S.d_rf + p0, pn, dshard, S.recs ? S.recs + p0 * fbk::kSlots * n_a : (const Slot*)nullptr);
    } else {
      hipLaunchKernelGGL(fbk::k_row_cardinality, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, a->d_slots, ra, n, dshard);
    }
    if (z.cards_words) hipLaunchKernelGGL(fbk::k_row_cardinality, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, a->d_slots, ra, n, B.cards.as<u64>());
    if (S.filter && src) hipLaunchKernelGGL(fbk::k_row_cardinality, dim3(uint32_t((pn + 255) / 256)), dim3(256), 0, ctx->stream, S.filter->d_slots, S.d_rf + p0, uint64_t(pn), src);
    if (z.cands)  // (no source: the first cand_n rows of the rank order that reach MinThreshold, fragment.go:1398-1401)
      hipLaunchKernelGGL(fbk::k_topn_candidates, dim3(pn), dim3(256), 0, ctx->stream, dshard, dcards, src, n_a, cand_n, min_threshold, tanimoto, sourced ? 1 : 0, B.d_cand);
    if (z.thresholds)  // (no source: count == cardinality, the rule is count >= MinThreshold)
      hipLaunchKernelGGL(fbk::k_topn_filter, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, dshard, dcards, src, n, n_a, min_threshold, tanimoto);
    hipLaunchKernelGGL(fbk::k_reduce_shards, dim3(uint32_t((uint64_t(n_a) + 255) / 256), std::min<uint32_t>(pn, 64)), dim3(256), 0, ctx->stream, dshard, pn,
                       uint64_t(n_a), B.d_total);
  }
  if (mask && z.cands) hipLaunchKernelGGL(fbk::k_topn_mask, dim3((n_a + 255) / 256), dim3(256), 0, ctx->stream, B.d_total, B.d_cand, n_a);
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// the one-shot form: validates and uploads the row lists, allocates B from the plan, enqueues.  ext_total / ext_cand: TopnBuffers
int32_t topn_totals_locked(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards,
                           uint64_t min_threshold, uint64_t tanimoto_threshold, uint32_t cand_n, TopnBuffers& B, bool mask, u64* ext_total = nullptr,
                           u64* ext_cand = nullptr) {
  if (int32_t rc = check_rows(rows_a, uint64_t(n_shards) * n_a, a->n_rows, "topk rows")) return rc;
  if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(a))) return rc;
  DevBuf drows;
  const uint32_t* dr[2] = {nullptr, nullptr};  // field rows and filter rows: one upload
  const uint64_t n_f = filter ? n_shards : 0;
  if (int32_t rc = upload_rows_multi(ctx, {{rows_a, uint64_t(n_shards) * n_a, UINT32_MAX}, {rows_f, n_f, filter ? filter->n_rows : UINT32_MAX}}, drows, dr)) return rc;
  const TopnSource S{filter, dr[1]};
  HIP_TRY(B.alloc(ctx, topn_plan(ctx, n_a, n_shards, S, min_threshold, tanimoto_threshold, cand_n), ext_total, ext_cand));
  return topn_totals_enqueue(ctx, a, dr[0], S, B, mask);
}

// *out_n = want; an error when the caller's buffers hold fewer
int32_t topn_capacity_ok(const char* who, uint32_t want, uint32_t cap, uint32_t* out_n) {
  *out_n = want;
  if (want > cap) return fail(FBK_E_CAPACITY, std::string(who) + ": " + std::to_string(want) + " results, buffers hold " + std::to_string(cap));
  return FBK_OK;
}

// The host ordering of totals that are on the host (fbk_topn_plan::order), written to the caller's buffers.
int32_t topn_order_host(const char* who, const uint64_t* totals, const uint64_t* cand, uint32_t n_a, uint32_t k, uint32_t* out_index, uint64_t* out_count, uint32_t cap,
                        uint32_t* out_n) {
  const std::vector<uint32_t> order = fbk_topn_plan::order(totals, cand, n_a, k);
  if (int32_t rc = topn_capacity_ok(who, uint32_t(order.size()), cap, out_n)) return rc;
  for (size_t j = 0; j < order.size(); ++j) {
    out_index[j] = order[j];
    out_count[j] = totals[order[j]];
  }
  return FBK_OK;
}

// The ordering on the device: {sorted counts dsk, their row indexes dsv, the number of non-zero counts dnz} of n_a totals, and the scratch of the
// stable descending radix sort of (count, index) pairs that start in index order (dval: 0 .. n_a - 1, written before the first sort).
struct TopnSort {
  DevBuf dsk, dval, dsv, dtmp, dnz;
  size_t tmp_bytes = 0;
  bool iota_done = false;
  hipError_t alloc(fbk_ctx* ctx, uint32_t n_a) {
    hipError_t e = dsk.alloc(ctx, uint64_t(n_a) * 8);
    if (e == hipSuccess) e = dval.alloc(ctx, uint64_t(n_a) * 4);
    if (e == hipSuccess) e = dsv.alloc(ctx, uint64_t(n_a) * 4);
    if (e == hipSuccess) e = dnz.alloc(ctx, 16);
    if (e == hipSuccess)
      e = hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, dsk.as<u64>(), dsk.as<u64>(), dval.as<uint32_t>(), dsv.as<uint32_t>(), int(n_a), 0, 64, ctx->stream);
    if (e == hipSuccess) e = dtmp.alloc(ctx, std::max<size_t>(tmp_bytes, 16));
    return e;
  }
};

// launch only: nothing allocated, nothing copied, no synchronisation
int32_t topn_radix_enqueue(fbk_ctx* ctx, TopnSort& s, u64* d_total, uint32_t n_a) {
  if (!s.iota_done) hipLaunchKernelGGL(fbk::k_iota_u32, dim3((n_a + 255) / 256), dim3(256), 0, ctx->stream, s.dval.as<uint32_t>(), n_a);
  s.iota_done = true;
  size_t tb = s.tmp_bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(s.dtmp.p, tb, d_total, s.dsk.as<u64>(), s.dval.as<uint32_t>(), s.dsv.as<uint32_t>(), int(n_a), 0, 64, ctx->stream));
  hipLaunchKernelGGL(fbk::k_count_nonzero_desc, dim3(1), dim3(1), 0, ctx->stream, s.dsk.as<u64>(), n_a, s.dnz.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// The ordering of a prepared TopN's run, launch only.  A field of a few thousand rows: every row finds its own rank (one launch; the radix sort's
// five launches were 30 of the 154 us of TopN(10) over config 3's 64 rows); larger fields: the radix sort.
int32_t topn_order_enqueue(fbk_ctx* ctx, TopnSort& s, u64* d_total, uint32_t n_a) {
  if (n_a > fbk::kRankSortMax) return topn_radix_enqueue(ctx, s, d_total, n_a);
  HIP_TRY(hipMemsetAsync(s.dnz.p, 0, 4, ctx->stream));
  hipLaunchKernelGGL(fbk::k_rank_sort_desc, dim3((n_a + 255) / 256), dim3(256), 0, ctx->stream, d_total, n_a, s.dsk.as<u64>(), s.dsv.as<uint32_t>(), s.dnz.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// fbk_query_topn (fragment.top's per-shard rules, executeTopN's sum over shards: fbk_topn) with nothing left to the host: row lists resident, the
// n asked for, the pass buffers with their plan (thresholds, the candidate pass's n under the semantics in force at prepare), the resolved records
// of the field's rows, and the scratch of the on-device ordering — all sized at prepare.  A run leaves {counts, indexes, number of non-empty rows}
// on the device; topn_read copies the first n.
struct TopnPlan {
  const fbk_batch *a = nullptr, *filter = nullptr;
  uint32_t n_a = 0, n_shards = 0, top_n = 0;
  DevBuf rows;
  const uint32_t* dr[2] = {nullptr, nullptr};  // field rows and filter rows on the device
  TopnBuffers buf;
  TopnSort sort;
  RowRecords recs;
};

// validates and uploads the row lists, sizes the buffers; d_total [n_a]: the totals of every run (the query's result)
int32_t topn_prepare(fbk_ctx* ctx, TopnPlan& P, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards,
                     uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold, u64* d_total) {
  P.a = a;
  P.filter = filter;
  P.n_a = n_a;
  P.n_shards = n_shards;
  P.top_n = n;
  if (int32_t rc = check_rows(rows_a, uint64_t(n_shards) * n_a, a->n_rows, "topk rows")) return rc;
  // (the semantics and option matrix_pass_kb in force when the query is prepared)
  const fbk_topn_plan::Sizes sizes = topn_plan(ctx, n_a, n_shards, TopnSource{filter}, min_threshold, tanimoto_threshold, topn_cand_n(ctx, n, n_a, true));
  if (int32_t rc = upload_rows_multi(ctx, {{rows_a, uint64_t(n_shards) * n_a, UINT32_MAX}, {rows_f, filter ? uint64_t(n_shards) : 0, filter ? filter->n_rows : UINT32_MAX}}, P.rows, P.dr))
    return rc;
  hipError_t e = P.buf.alloc(ctx, sizes, d_total);
  if (e == hipSuccess) e = P.sort.alloc(ctx, n_a);
  if (e != hipSuccess) return fail(FBK_E_NOMEM, std::string("query: ") + hipGetErrorString(e));
  return FBK_OK;
}

int32_t topn_enqueue(fbk_ctx* ctx, TopnPlan& P) {
  const Slot* recs = nullptr;
  if (P.filter)  // (the counts against the filter read them; without a filter the stored cardinalities answer)
    if (int32_t rc = query_row_records(ctx, P.recs, P.a, P.dr[0], P.n_shards, P.n_a, &recs)) return rc;
  if (int32_t rc = topn_totals_enqueue(ctx, P.a, P.dr[0], TopnSource{P.filter, P.dr[1], recs}, P.buf, /*mask=*/true)) return rc;
  return topn_order_enqueue(ctx, P.sort, P.buf.d_total, P.n_a);
}

// out_index = uint32 {number of results, then that many row indexes} (1 + min(n, n_a) words, n = 0: 1 + n_a); out_count = uint64 counts of those rows
int32_t topn_read(fbk_ctx* ctx, const TopnPlan& P, uint32_t* out_index, uint64_t* out_count) {
  uint32_t nz = 0;
  D2H back(ctx);
  HIP_TRY(back.add(&nz, P.sort.dnz.p, 4));
  HIP_TRY(back.finish());
  const uint32_t want = P.top_n ? std::min(P.top_n, nz) : nz;  // rows without a single common column are not results
  if (out_index) out_index[0] = want;
  if (want) {
    D2H back2(ctx);
    if (out_index) HIP_TRY(back2.add(out_index + 1, P.sort.dsv.p, uint64_t(want) * 4));
    if (out_count) HIP_TRY(back2.add(out_count, P.sort.dsk.p, uint64_t(want) * 8));
    HIP_TRY(back2.finish());
  }
  return FBK_OK;
}

// The ordering step of TopK / TopN over totals that are already on the device (d_total: n_a uint64, this context's stream): count descending,
// row index ascending inside one count, zero counts dropped, at most k results (k = 0: all).  Synchronises the stream.
int32_t topn_order_locked(fbk_ctx* ctx, u64* d_total, uint32_t n_a, uint32_t k, uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n) {
  // (BSIData.PivotDescending, bsi.go:18-62.)  A field of a few thousand rows is ordered on the host (32 KB of totals cross the bus; a device radix
  // sort of 64 keys costs 50 us of launch latency, measured); larger fields by a stable descending radix sort of (count, index) pairs that start in
  // index order, and only the winners come back.  FBK_TOPK_DEVICE_SORT=1 / =0 pins the choice (tests).
  bool device_sort = n_a > 4096;
  if (ctx->opt.topk_device_sort >= 0) device_sort = ctx->opt.topk_device_sort == 1;
  if (!device_sort) {
    std::vector<uint64_t> tot(n_a);
    D2H back(ctx);
    HIP_TRY(back.add(tot.data(), d_total, uint64_t(n_a) * 8));
    HIP_TRY(back.finish());
    return topn_order_host("topk", tot.data(), nullptr, n_a, k, out_index, out_count, cap, out_n);
  }
  TopnSort s;
  HIP_TRY(s.alloc(ctx, n_a));
  if (int32_t rc = topn_radix_enqueue(ctx, s, d_total, n_a)) return rc;
  uint32_t nz = 0;
  HIP_TRY(hipMemcpyAsync(&nz, s.dnz.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  // (rows without a single common column are not results)
  if (int32_t rc = topn_capacity_ok("topk", k ? std::min(k, nz) : nz, cap, out_n)) return rc;
  if (*out_n) {
    D2H back(ctx);
    HIP_TRY(back.add(out_index, s.dsv.p, uint64_t(*out_n) * 4));
    HIP_TRY(back.add(out_count, s.dsk.p, uint64_t(*out_n) * 8));
    HIP_TRY(back.finish());
  }
  return FBK_OK;
}

int32_t topn_impl(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, uint32_t k,
                  uint64_t min_threshold, uint64_t tanimoto_threshold, uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n, bool reference_operator = false) {
  if (!ctx || !a || !out_n || (n_shards && n_a && !rows_a) || (filter && n_shards && !rows_f) || (cap && (!out_index || !out_count)))
    return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = topn_args_ok(n_a, tanimoto_threshold)) return rc;
  *out_n = 0;
  if (n_shards == 0 || n_a == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  TopnBuffers B;
  const uint32_t cand_n = topn_cand_n(ctx, k, n_a, reference_operator);
  if (int32_t rc = topn_totals_locked(ctx, a, rows_a, n_a, filter, rows_f, n_shards, min_threshold, tanimoto_threshold, cand_n, B, /*mask=*/true)) return rc;
  return topn_order_locked(ctx, B.d_total, n_a, k, out_index, out_count, cap, out_n);
}

}  // namespace

extern "C" {

int32_t fbk_topk(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, uint32_t k,
                 uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n) try {
  FBK_ENTER(ctx);
  return topn_impl(ctx, a, rows_a, n_a, filter, rows_f, n_shards, k, 0, 0, out_index, out_count, cap, out_n);
} FBK_ABI_CATCH(ctx)

int32_t fbk_topn(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, uint32_t n,
                 uint64_t min_threshold, uint64_t tanimoto_threshold, uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n) try {
  FBK_ENTER(ctx);
  return topn_impl(ctx, a, rows_a, n_a, filter, rows_f, n_shards, n, min_threshold, tanimoto_threshold, out_index, out_count, cap, out_n, /*reference_operator=*/true);
} FBK_ABI_CATCH(ctx)

int32_t fbk_topn_partials(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter, const uint32_t* rows_f,
                          uint32_t n_shards, uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold, uint64_t* out_totals, uint64_t* out_candidates) try {
  FBK_ENTER(ctx);
  if (!ctx || !out_totals || !out_candidates || (n_shards && n_a && (!a || !rows_a)) || (filter && n_shards && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = topn_args_ok(n_a, tanimoto_threshold)) return rc;
  std::memset(out_totals, 0, uint64_t(n_a) * 8);
  std::memset(out_candidates, 0, uint64_t(n_a) * 8);
  if (n_shards == 0 || n_a == 0) return FBK_OK;  // a member without shards: zeros, no candidates
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  TopnBuffers B;
  const uint32_t cand_n = topn_cand_n(ctx, n, n_a, true);
  if (int32_t rc = topn_totals_locked(ctx, a, rows_a, n_a, filter, rows_f, n_shards, min_threshold, tanimoto_threshold, cand_n, B, /*mask=*/false)) return rc;
  D2H back(ctx);
  HIP_TRY(back.add(out_totals, B.d_total, uint64_t(n_a) * 8));
  if (cand_n) HIP_TRY(back.add(out_candidates, B.d_cand, uint64_t(n_a) * 8));
  HIP_TRY(back.finish());
  if (!cand_n)  // no candidate pass: every row that has a total is its own candidate
    for (uint32_t i = 0; i < n_a; ++i) out_candidates[i] = out_totals[i] ? 1 : 0;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_topk_bsi(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter,
                     const uint32_t* rows_f, uint32_t n_shards, uint32_t flags, fbk_batch** out_batch, uint32_t* out_depth) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !out_batch || !out_depth || (n_shards && n_a && !rows_a) || (filter && n_shards && !rows_f))
    return fail(FBK_E_INVALID, "NULL argument");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  if (n_a > (1u << 20)) return fail(FBK_E_INVALID, "topk_bsi: at most 2^20 rows (one shard width of row ids per output row)");
  *out_batch = nullptr;
  *out_depth = 0;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  TopnBuffers B;  // (totals: only with shards and rows; depth stays 0 without)
  DevBuf dmax;
  HIP_TRY(dmax.alloc(ctx, 8));
  HIP_TRY(hipMemsetAsync(dmax.p, 0, 8, ctx->stream));
  u64 mx = 0;
  if (n_shards && n_a) {
    if (int32_t rc = topn_totals_locked(ctx, a, rows_a, n_a, filter, rows_f, n_shards, 0, 0, 0, B, /*mask=*/false)) return rc;
    hipLaunchKernelGGL(fbk::k_max_u64, dim3(std::min<uint32_t>(1024, (n_a + 255) / 256)), dim3(256), 0, ctx->stream, B.d_total, uint64_t(n_a), dmax.as<u64>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&mx, dmax.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  const uint32_t depth = uint32_t(bits_len64(mx));  // planes the largest count needs (bsiBuilder grows the same way, bsi.go:256)
  *out_depth = depth;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, depth, 0, "topk_bsi")) return rc;
  if (depth) {
    fbk_batch* o = out.batch();
    const uint64_t n_slots = uint64_t(depth) * fbk::kSlots;
    HIP_TRY(hipMemsetAsync(o->d_arena, 0, n_slots * 8192ull, ctx->stream));
    hipLaunchKernelGGL(fbk::k_counts_to_bsi, dim3((n_a + 255) / 256), dim3(256), 0, ctx->stream, B.d_total, n_a, depth, o->d_arena);
    hipLaunchKernelGGL(fbk::k_cell_stats, dim3(uint32_t((n_slots + 3) / 4)), dim3(256), 0, ctx->stream, o->d_arena, o->d_slots, out.runs(), n_slots);
    if (int32_t rc = out.finish(flags, 0, nullptr)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
