// fbk_topn_plan.h — host rules of the TopK / TopN family (HIP-free: compiled into the library and into the stand-alone check of the tests,
// tests/cpp/topn_plan_check.cpp).  Two things every call of the family decides the same way, written once:
//   plan()   how many shards one pass holds, which scratch vectors it needs and how large: the one-shot calls, fbk_query_topn (sized
//            once, at prepare) and the fbk_expr_* calls over a tree allocate from it, topn_totals_enqueue (fbk_topn_api.inc) launches from it;
//   order()  the host ordering of totals (BSIData.PivotDescending / Pairs.Less).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace fbk_topn_plan {

// where the per-shard filter of the counts comes from: nowhere (a row's count is its stored cardinality), one row per shard of a
// filter batch (k_rows_vs_filter), a call tree the counting kernel evaluates itself (k_expr_rows_vs_filter)
enum Source : uint32_t { kNoSource = 0, kRowSource = 1, kTreeSource = 2 };

struct Request {
  uint32_t n_a = 0, n_shards = 0;
  Source source = kNoSource;
  uint64_t min_threshold = 0, tanimoto_threshold = 0;
  uint32_t cand_n = 0;          // > 0: the reference's candidate pass with this n (k_topn_candidates)
  uint64_t matrix_pass_kb = 0;  // option matrix_pass_kb: the per-shard counts of one pass stay below this
  bool keep_per_shard = false;  // the caller reads the per-shard counts: ONE pass over all shards
  bool keep_src = false;        // the caller reads the per-shard source counts
};

struct Sizes {
  Request req;
  uint64_t pass_shards = 0;  // shards per pass (>= 1)
  uint64_t tanimoto = 0;     // the Tanimoto threshold in force: 0 without a source (fragment.top ignores it there)
  bool thresholds = false;   // k_topn_filter runs
  bool cands = false;        // k_topn_candidates runs
  // 64-bit words of each vector (0: not needed).  shard: [pass_shards][n_a] counts; cards: [pass_shards][n_a] stored cardinalities (without
  // a source the counts ARE the cardinalities); src: [n_shards] source counts, indexed by the CALL's shard for every source; cand: [n_a] flags
  uint64_t shard_words = 0, cards_words = 0, src_words = 0, cand_words = 0;
};

inline Sizes plan(const Request& r) {
  Sizes s;
  s.req = r;
  const bool sourced = r.source != kNoSource;
  s.tanimoto = sourced ? r.tanimoto_threshold : 0;
  s.thresholds = r.min_threshold > 0 || s.tanimoto > 0;
  s.cands = r.cand_n > 0;
  const uint64_t fit = r.n_a ? (r.matrix_pass_kb << 10) / (uint64_t(r.n_a) * 8) : r.n_shards;
  s.pass_shards = std::max<uint64_t>(1, r.keep_per_shard ? r.n_shards : std::min<uint64_t>(r.n_shards, fit));
  s.shard_words = s.pass_shards * r.n_a;
  const bool rules = s.thresholds || s.cands;  // the kernels of both compare a row's count with its cardinality and the source's
  s.cards_words = rules && sourced ? s.shard_words : 0;
  s.src_words = sourced && (rules || r.keep_src) ? r.n_shards : 0;
  s.cand_words = s.cands ? r.n_a : 0;
  return s;
}

// Row indexes by count descending, index ascending inside one count; rows with a zero total dropped, rows whose flag in `cand`
// (nullptr: no flags) is zero dropped; at most k (k = 0: all).
inline std::vector<uint32_t> order(const uint64_t* totals, const uint64_t* cand, uint32_t n_a, uint32_t k) {
  std::vector<uint32_t> o;
  o.reserve(n_a);
  for (uint32_t i = 0; i < n_a; ++i)
    if (totals[i] && (!cand || cand[i])) o.push_back(i);
  std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return totals[x] > totals[y]; });
  if (k && k < o.size()) o.resize(k);
  return o;
}

}  // namespace fbk_topn_plan
