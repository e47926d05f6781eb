// topn_plan_check.cpp — stand-alone driver of the host rules of the TopK / TopN family (featurebase_amd/csrc/fbk_topn_plan.h):
// fbk_topn_plan::plan, the sizing of a call's passes and scratch vectors, and fbk_topn_plan::order, the host ordering of totals; built
// WITHOUT HIP and with -fsanitize=address,undefined by tests/test_topn_plan_cpu.py.
//
//   topn_plan_check < requests
//
// requests (text), one per line:
//   S <n_a> <n_shards> <source 0|1|2> <min_threshold> <tanimoto_threshold> <cand_n> <matrix_pass_kb> <keep_per_shard> <keep_src>
//       -> "<pass_shards> <tanimoto in force> <thresholds> <cands> <shard_words> <cards_words> <src_words> <cand_words>"
//   O <k> <flags 0|1> <n> <n totals> [<n candidate flags>]
//       -> "<m> <m row indexes>"
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../featurebase_amd/csrc/fbk_topn_plan.h"

int main() {
  char kind = 0;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'S') {
      fbk_topn_plan::Request r;
      unsigned source = 0, keep_per_shard = 0, keep_src = 0;
      if (std::scanf("%" SCNu32 " %" SCNu32 " %u %" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu64 " %u %u", &r.n_a, &r.n_shards, &source, &r.min_threshold,
                     &r.tanimoto_threshold, &r.cand_n, &r.matrix_pass_kb, &keep_per_shard, &keep_src) != 9 ||
          source > 2)
        return 2;
      r.source = fbk_topn_plan::Source(source);
      r.keep_per_shard = keep_per_shard != 0;
      r.keep_src = keep_src != 0;
      const fbk_topn_plan::Sizes s = fbk_topn_plan::plan(r);
      std::printf("%" PRIu64 " %" PRIu64 " %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s.pass_shards, s.tanimoto, int(s.thresholds), int(s.cands),
                  s.shard_words, s.cards_words, s.src_words, s.cand_words);
    } else if (kind == 'O') {
      uint32_t k = 0, n = 0;
      unsigned flags = 0;
      if (std::scanf("%" SCNu32 " %u %" SCNu32, &k, &flags, &n) != 3) return 2;
      std::vector<uint64_t> tot(n), cand(flags ? n : 0);
      for (uint64_t& v : tot)
        if (std::scanf("%" SCNu64, &v) != 1) return 2;
      for (uint64_t& v : cand)
        if (std::scanf("%" SCNu64, &v) != 1) return 2;
      const std::vector<uint32_t> o = fbk_topn_plan::order(tot.data(), flags ? cand.data() : nullptr, n, k);
      std::printf("%zu", o.size());
      for (uint32_t i : o) std::printf(" %" PRIu32, i);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
