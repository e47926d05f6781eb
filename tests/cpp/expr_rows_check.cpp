// expr_rows_check.cpp — stand-alone driver of fbk_expr::rows_per_block (featurebase_amd/csrc/fbk_expr_plan.h), the rule that
// sizes the blocks of k_expr_rows_vs_filter; built WITHOUT HIP and with -fsanitize=address,undefined by tests/test_expr_rows_cpu.py.
//
//   expr_rows_check < grid
//
// grid (text): one "<n_a> <n_shards_in_pass> <L>" per line; one rows-per-block per line on stdout.
#include <cstdio>

#include "../../featurebase_amd/csrc/fbk_expr_plan.h"

int main() {
  unsigned n_a = 0, n_shards = 0, L = 0;
  while (std::scanf("%u %u %u", &n_a, &n_shards, &L) == 3) std::printf("%u\n", fbk_expr::rows_per_block(n_a, n_shards, L));
  return 0;
}
