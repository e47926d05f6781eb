// Stand-alone check of featurebase_amd/csrc/fbk_minmax_plan.h (no GPU, no HIP): reads one question per line from stdin and prints
// the header's answer, for tests/test_count_matrix_minmax_cpu.py (and the GPU test, which reads the two constants here).
//   K                          -> kMinmaxDescentCells kMinmaxDescentMaxCells kDescentBlocks
//   P n_a n_b flags            -> path (1 descent, 2 scatter, 0 error)
//   G n_shards cells           -> tiles unit-blocks
//   C n_shards densified_rows  -> shards per densify pass
//   g++ -std=c++17 -fsanitize=address,undefined tests/cpp/minmax_plan_check.cpp
#include <cinttypes>
#include <cstdio>

#include "../../featurebase_amd/csrc/fbk_minmax_plan.h"

int main() {
  namespace mp = fbk_minmax_plan;
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    uint64_t a = 0, b = 0, c = 0;
    if (kind == 'K') {
      std::printf("%u %u %u\n", mp::kMinmaxDescentCells, mp::kMinmaxDescentMaxCells, mp::kDescentBlocks);
    } else if (kind == 'P' && std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3) {
      std::printf("%u\n", mp::path(a, b, uint32_t(c)));
    } else if (kind == 'G' && std::scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) {
      std::printf("%u %u\n", mp::tiles_of(b), mp::descent_grid(uint32_t(a), b));
    } else if (kind == 'C' && std::scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) {
      std::printf("%u\n", mp::densify_chunk(uint32_t(a), b));
    } else {
      std::fprintf(stderr, "bad question '%c'\n", kind);
      return 2;
    }
  }
  return 0;
}
