// fbk_select_plan.h — the key of the radix select and the host rules of fbk_bsi_sort, fbk_bsi_quantiles and fbk_bsi_percentile
// (HIP-free: compiled into the library and into tests/cpp/select_plan_check.cpp), written once: the key (the kernels call the same
// sort_key / sort_value), the descent, Sort's cut, a quantile call's rank table and launches, Percentile's ranks and replay, the chunk.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "fbk_dense_policy.h"

namespace fbk {

constexpr uint32_t kSortDigitBits = 11;  // of a pass of fbk_bsi_sort's and fbk_bsi_quantiles' select
constexpr uint32_t kSortBins = 1u << kSortDigitBits;
constexpr uint32_t kQuantPrefixes = 8;  // histograms of one k_quant_hist launch: 8 * 2048 * 4 = 64 KiB of LDS at most

// The key of a column, order preserving and unsigned (fbk_sort.hip.h describes it) and its three constants
typedef unsigned long long u64;  // (as fbk_kernels.hip.h: the kernels' 64-bit word)
struct SortKey {
  u64 flip;  // 2^63 in the 64-bit form, else 0
  u64 bias;  // 2^bit_depth in the short form, else 0
  u64 desc;  // the key's bits, if descending, else 0
  uint32_t keep_zero;
};

FBK_HD inline constexpr uint32_t key_bits(uint32_t bit_depth) { return bit_depth >= 63 ? 64u : bit_depth + 1; }
FBK_HD inline constexpr uint32_t passes(uint32_t bit_depth, uint32_t digit) { return (key_bits(bit_depth) + digit - 1) / digit; }

// (always_inline: the kernels' code is then what it was when these were __forceinline__ device functions)
#define FBK_KEY_FN FBK_HD inline __attribute__((always_inline))
FBK_KEY_FN SortKey select_key(uint32_t bit_depth, bool descending, bool keep_zero) {
  const bool wide = bit_depth >= 63;
  const u64 bits = wide ? ~0ull : (2ull << bit_depth) - 1;  // (plain selects: a constant `descending` leaves the kernels no trace of it)
  return SortKey{wide ? 1ull << 63 : 0ull, wide ? 0ull : 1ull << bit_depth, descending ? bits : 0ull, uint32_t(keep_zero)};
}

// the key that IS the stored value (Distinct rows).  Not a depth of select_key: testing it costs k_gquant_*, whose depth is run-time, a compare
FBK_KEY_FN SortKey value_key() { return SortKey{0, 0, 0, 1}; }

FBK_KEY_FN u64 sort_key(u64 value, const SortKey& k) { return ((value ^ k.flip) + k.bias) ^ k.desc; }
FBK_KEY_FN long long sort_value(u64 key, const SortKey& k) { return (long long)((((key ^ k.desc) - k.bias)) ^ k.flip); }
#undef FBK_KEY_FN

struct QuantPrefixes { u64 p[kQuantPrefixes]; };  // of one k_quant_hist launch, ascending; entries at and past n_pre are not read

}  // namespace fbk

namespace fbk_select_plan {

// Shards per walk: at most 2^28 / (2^17 * R) of them (R = the rows densified per shard), dealt evenly over the fewest walks.
constexpr uint64_t kExtractScratch = 1ull << 28;
inline uint32_t densify_chunk(uint32_t n_shards, uint64_t densified) { return fbk::even_chunk(n_shards, kExtractScratch, fbk::kDenseRowBytes * densified); }

// The bin of hist[0 .. bins) that holds the 0-based rank, and the columns in the bins before it (a rank past the total: the last bin).
struct Descent { uint32_t bin; uint64_t before; };
inline Descent descend(const uint64_t* hist, uint32_t bins, uint64_t rank) {
  uint64_t before = 0;
  uint32_t b = 0;
  while (b + 1 < bins && before + hist[b] <= rank) before += hist[b++];
  return {b, before};
}

// Sort(offset=, limit=) over `total` columns: the records [lo, K) of the order (executor.go:9367-9383; no limit: UINT64_MAX)
struct SortCut { uint64_t lo, K; };
inline SortCut sort_cut(uint64_t total, uint64_t offset, uint64_t limit) {
  const uint64_t lo = std::min(offset, total);
  return {lo, lo + std::min(limit, total - lo)};
}

// A distinct rank of a quantile call on its way down the digits: its rank among the columns of its prefix, the key's digits so far,
// the columns in its bin of the last pass; step(): one pass further, by the histogram of its prefix
struct Target { uint64_t want, prefix, count; };
inline void step(Target& t, const uint64_t* hist) {
  const Descent d = descend(hist, fbk::kSortBins, t.want);
  t.want -= d.before, t.prefix = (t.prefix << fbk::kSortDigitBits) | d.bin, t.count = hist[d.bin];
}

// The distinct ranks of `ranks`, ascending, as targets; ranks[i] is target of[i].
inline std::vector<Target> rank_table(const std::vector<uint64_t>& ranks, std::vector<uint32_t>& of) {
  std::vector<uint64_t> uniq(ranks);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  of.resize(ranks.size());
  for (size_t i = 0; i < ranks.size(); ++i) of[i] = uint32_t(std::lower_bound(uniq.begin(), uniq.end(), ranks[i]) - uniq.begin());
  std::vector<Target> tg;
  for (uint64_t r : uniq) tg.push_back({r, 0, 0});
  return tg;
}

// Ascending ranks keep ascending prefixes, so the distinct prefixes are runs of tg: the launch that starts at target a takes the
// targets [a, e) with n_pre <= kQuantPrefixes distinct prefixes pre.p[0 .. n_pre).  Returns e (> a).
inline size_t prefix_group(const std::vector<Target>& tg, size_t a, fbk::QuantPrefixes& pre, uint32_t& n_pre) {
  n_pre = 0;
  size_t e = a;
  while (e < tg.size() && (n_pre < fbk::kQuantPrefixes || tg[e].prefix == pre.p[n_pre - 1])) {
    if (n_pre == 0 || tg[e].prefix != pre.p[n_pre - 1]) pre.p[n_pre++] = tg[e].prefix;
    ++e;
  }
  return e;
}

// Percentile(nth) over N >= 1 values: desiredLess L, desiredGreater G (executor.go:1408-1409) and where s[L], s[N-1-G] are in the
// rank list (-1: not below N, or not needed).  The list: 0 and N - 1, then per nth that reaches the search loop L and N - 1 - G.
struct PctNeed { uint64_t L, G; int32_t a = -1, b = -1; };
inline void percentile_ranks(uint64_t N, const double* nth, uint32_t n_nth, std::vector<PctNeed>& need, std::vector<uint64_t>& ranks) {
  need.assign(n_nth, PctNeed{});
  ranks.insert(ranks.end(), {0, N - 1});
  for (uint32_t i = 0; i < n_nth; ++i) {
    // two IEEE operations each, in statements of their own (a product then a quotient: nothing a compiler could contract)
    double less = double(N) * nth[i];
    less = less / 100.0;
    double more = double(N) * (100 - nth[i]);
    more = more / 100.0;
    PctNeed& nd = need[i];
    nd.L = uint64_t(less), nd.G = uint64_t(more);
    if (nd.G == 0 || nd.L == 0) continue;  // the maximum, or the minimum
    if (nd.L < N) nd.a = int32_t(ranks.size()), ranks.push_back(nd.L);
    if (nd.G < N) nd.b = int32_t(ranks.size()), ranks.push_back(N - 1 - nd.G);
  }
}

// The call's answers from the values / counts at percentile_ranks' ranks (false: minimum or maximum + base leaves int64): the loop of
// executor.go:1411-1585 with "leftCount > desiredLess" restated as s[L] < guess, "rightCount > desiredGreater" as s[N-1-G] > guess.
inline bool percentile_finish(const std::vector<PctNeed>& need, const std::vector<int64_t>& vals, const std::vector<uint64_t>& cnts, int64_t base,
                              int64_t* out_values, uint64_t* out_counts) {
  int64_t mn, mx;
  if (__builtin_add_overflow(vals[0], base, &mn) || __builtin_add_overflow(vals[1], base, &mx)) return false;
  for (size_t i = 0; i < need.size(); ++i) {
    const PctNeed& nd = need[i];
    int64_t lo = mn, hi = mx, guess = nd.G == 0 ? mx : mn;
    out_counts[i] = nd.G == 0 ? cnts[1] : nd.L == 0 ? cnts[0] : 1;  // the maximum; the minimum; a guess of the loop
    while (nd.G != 0 && nd.L != 0 && lo < hi) {
      guess = (lo / 2) + (hi / 2) + (((lo % 2) + (hi % 2)) / 2);  // average without overflow (:1497-1501)
      if (nd.a >= 0 && vals[nd.a] + base < guess) hi = guess - 1;
      else if (nd.b >= 0 && vals[nd.b] + base > guess) lo = guess + 1;
      else break;
    }
    out_values[i] = guess;
  }
  return true;
}

}  // namespace fbk_select_plan
