// Stand-alone check of the host rules of the GroupBy selection stage (featurebase_amd/csrc/fbk_group_select_plan.h, no HIP, no GPU),
// built by tests/test_group_select_plan_cpu.py with -fsanitize=address,undefined.  One case per input line:
//   flags n_sort s0 d0 s1 d1 having_subject having_op lo hi offset limit has_agg n  counts[n]  aggs[n] (when has_agg)
// lo / hi are decimal int64 (a count bound above 2^63 - 1 comes as its two's complement), offset / limit decimal uint64.
// One output line per case: "E <message>" when check() refuses the selection, else "matched n cell0 cell1 ...".
//   g++ -std=c++17 -fsanitize=address,undefined tests/cpp/group_select_check.cpp
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../featurebase_amd/csrc/fbk_group_select_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    fbk_groupby_select s{};
    int has_agg = 0;
    unsigned long long n = 0;
    in >> s.flags >> s.n_sort >> s.sort[0].subject >> s.sort[0].desc >> s.sort[1].subject >> s.sort[1].desc >> s.having_subject >> s.having_op >> s.having_lo >>
        s.having_hi >> s.offset >> s.limit >> has_agg >> n;
    std::vector<uint64_t> counts(n);
    std::vector<int64_t> aggs(has_agg ? n : 0);
    for (uint64_t& c : counts) in >> c;
    for (int64_t& a : aggs) in >> a;
    if (!in) {
      std::printf("E bad input line\n");
      return 2;
    }
    if (const char* what = fbk_group_select::check(&s, has_agg != 0)) {
      std::printf("E %s\n", what);
      continue;
    }
    std::vector<uint32_t> cells;
    const uint64_t matched = fbk_group_select::select(counts.data(), has_agg ? aggs.data() : nullptr, n, s, cells);
    std::printf("%llu %zu", (unsigned long long)matched, cells.size());
    for (uint32_t c : cells) std::printf(" %u", c);
    std::printf("\n");
  }
  return 0;
}
