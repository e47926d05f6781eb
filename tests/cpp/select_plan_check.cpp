// Stand-alone check of featurebase_amd/csrc/fbk_select_plan.h (no GPU, no HIP): reads one question per line from stdin and prints the
// header's answer on one line, for tests/test_select_plan_cpu.py.  Signed values are decimal int64, nth values C hex floats.
//   Q                                   -> kSortDigitBits kSortBins kQuantPrefixes kExtractScratch
//   K depth desc keep n v[n]            -> keep_zero, key bits, passes at 11 bits, then per value its key and sort_value(key)
//   D bins rank h[bins]                 -> descend(): bin, columns before it
//   C total offset limit                -> sort_cut(): lo, K
//   T n r[n]                            -> rank_table(): the number of targets, their ranks, then of[n]
//   G n p[n]                            -> prefix_group() over targets with these prefixes, launch by launch: e, n_pre, pre[n_pre]
//   P base n_nth nth[n_nth] n v[n]      -> fbk_bsi_percentile's host side over the sorted values: per nth value and count ("overflow":
//                                          minimum + base or maximum + base leaves int64)
//   S depth n_r r[n_r] n v[n]           -> fbk_bsi_quantiles' select with the histograms counted here: per rank value and count
//   g++ -std=c++17 -fsanitize=address,undefined tests/cpp/select_plan_check.cpp
#include <cinttypes>
#include <cstdio>

#include "../../featurebase_amd/csrc/fbk_select_plan.h"

namespace sp = fbk_select_plan;

static bool read_u64(std::vector<uint64_t>& v) {
  uint64_t n = 0;
  if (std::scanf("%" SCNu64, &n) != 1) return false;
  v.resize(n);
  for (uint64_t& x : v)
    if (std::scanf("%" SCNu64, &x) != 1) return false;
  return true;
}
static bool read_i64(std::vector<int64_t>& v) {
  uint64_t n = 0;
  if (std::scanf("%" SCNu64, &n) != 1) return false;
  v.resize(n);
  for (int64_t& x : v)
    if (std::scanf("%" SCNd64, &x) != 1) return false;
  return true;
}

// the counts of pass `shift` over the keys whose bits above the digit equal pre.p[j] (n_pre == 0: every key), as k_quant_hist's
static void count(const std::vector<uint64_t>& keys, uint32_t shift, const fbk::QuantPrefixes& pre, uint32_t n_pre, std::vector<uint64_t>& hh) {
  std::fill(hh.begin(), hh.end(), 0);
  for (uint64_t key : keys)
    for (uint32_t j = 0; j < (n_pre ? n_pre : 1); ++j)
      if (!n_pre || (key >> (shift + fbk::kSortDigitBits)) == pre.p[j]) ++hh[uint64_t(j) * fbk::kSortBins + ((key >> shift) & (fbk::kSortBins - 1))];
}

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    uint64_t a = 0, b = 0, c = 0;
    int64_t base = 0;
    std::vector<uint64_t> u;
    std::vector<int64_t> v;
    if (kind == 'Q') {
      std::printf("%u %u %u %" PRIu64, fbk::kSortDigitBits, fbk::kSortBins, fbk::kQuantPrefixes, sp::kExtractScratch);
    } else if (kind == 'K' && std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3 && read_i64(v)) {
      const fbk::SortKey sk = fbk::select_key(uint32_t(a), b != 0, c != 0);
      std::printf("%u %u %u", sk.keep_zero, fbk::key_bits(uint32_t(a)), fbk::passes(uint32_t(a), fbk::kSortDigitBits));
      for (int64_t x : v) std::printf(" %llu %lld", fbk::sort_key(uint64_t(x), sk), fbk::sort_value(fbk::sort_key(uint64_t(x), sk), sk));
    } else if (kind == 'D' && std::scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) {
      u.resize(a);
      for (uint64_t& x : u)
        if (std::scanf("%" SCNu64, &x) != 1) return 2;
      const sp::Descent d = sp::descend(u.data(), uint32_t(a), b);
      std::printf("%u %" PRIu64, d.bin, d.before);
    } else if (kind == 'C' && std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3) {
      std::printf("%" PRIu64 " %" PRIu64, sp::sort_cut(a, b, c).lo, sp::sort_cut(a, b, c).K);
    } else if (kind == 'T' && read_u64(u)) {
      std::vector<uint32_t> of;
      const std::vector<sp::Target> tg = sp::rank_table(u, of);
      std::printf("%zu", tg.size());
      for (const sp::Target& t : tg) std::printf(" %" PRIu64, t.want);
      for (uint32_t o : of) std::printf(" %u", o);
    } else if (kind == 'G' && read_u64(u)) {
      std::vector<sp::Target> tg;
      for (uint64_t p : u) tg.push_back({0, p, 0});
      for (size_t at = 0; at < tg.size();) {
        fbk::QuantPrefixes pre{};
        uint32_t n_pre = 0;
        at = sp::prefix_group(tg, at, pre, n_pre);
        std::printf("%zu %u ", at, n_pre);
        for (uint32_t j = 0; j < n_pre; ++j) std::printf("%llu ", pre.p[j]);
      }
    } else if (kind == 'P' && std::scanf("%" SCNd64 " %" SCNu64, &base, &b) == 2) {
      std::vector<double> nth(b);
      for (double& x : nth)
        if (std::scanf("%la", &x) != 1) return 2;
      if (!read_i64(v) || v.empty()) return 2;
      std::sort(v.begin(), v.end());
      std::vector<sp::PctNeed> need;
      std::vector<uint64_t> ranks, cnts;
      std::vector<int64_t> vals, ov(nth.size());
      sp::percentile_ranks(v.size(), nth.data(), uint32_t(nth.size()), need, ranks);
      for (uint64_t r : ranks) vals.push_back(v[r]), cnts.push_back(uint64_t(std::count(v.begin(), v.end(), v[r])));
      std::vector<uint64_t> oc(nth.size());
      if (!sp::percentile_finish(need, vals, cnts, base, ov.data(), oc.data())) std::printf("overflow");
      else
        for (size_t i = 0; i < nth.size(); ++i) std::printf("%" PRId64 " %" PRIu64 " ", ov[i], oc[i]);
    } else if (kind == 'S' && std::scanf("%" SCNu64, &a) == 1 && read_u64(u) && read_i64(v)) {
      const uint32_t depth = uint32_t(a), passes = fbk::passes(depth, fbk::kSortDigitBits);
      const fbk::SortKey sk = fbk::select_key(depth, false, true);
      std::vector<uint64_t> keys, hh(uint64_t(fbk::kQuantPrefixes) * fbk::kSortBins);
      for (int64_t x : v) keys.push_back(fbk::sort_key(uint64_t(x), sk));
      std::vector<uint32_t> of;
      std::vector<sp::Target> tg = sp::rank_table(u, of);
      for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = fbk::kSortDigitBits * (passes - 1 - p);
        for (size_t at = 0; at < tg.size();) {
          fbk::QuantPrefixes pre{};
          uint32_t n_pre = 0, j = 0;
          const size_t e = p ? sp::prefix_group(tg, at, pre, n_pre) : tg.size();
          count(keys, shift, pre, n_pre, hh);
          for (; at < e; ++at) {
            while (n_pre && pre.p[j] != tg[at].prefix) ++j;
            sp::step(tg[at], hh.data() + uint64_t(j) * fbk::kSortBins);
          }
        }
      }
      for (uint32_t o : of) std::printf("%lld %" PRIu64 " ", fbk::sort_value(tg[o].prefix, sk), tg[o].count);
    } else {
      std::fprintf(stderr, "bad question '%c'\n", kind);
      return 2;
    }
    std::printf("\n");
  }
  return 0;
}
