// Stand-alone check of featurebase_amd/csrc/fbk_group_quantile_plan.h (no GPU, no HIP): reads one question per line from stdin and
// prints the header's answer, for tests/test_count_matrix_quantiles_cpu.py (and the GPU test, which reads the constants here).
//   K                          -> kLdsDigitBits kGlobalDigitBits lds_pairs_cap kAutoLdsPairs kScratchBound kMaxDen kMaxRequests
//   P n_a n_b n_q flags        -> path (1 LDS, 2 GLOBAL, 0 error)
//   N bit_depth digit          -> key bits, passes
//   B bit_depth digit pass     -> the pass's lowest key bit, its width
//   S n_a n_b n_q digit        -> scratch bytes
//   C n_shards densified_rows  -> shards per densify walk
//   R N num den                -> the rank of PERCENTILE_DISC(num / den) over N values
//   g++ -std=c++17 -fsanitize=address,undefined tests/cpp/gquant_plan_check.cpp
#include <cinttypes>
#include <cstdio>

#include "../../featurebase_amd/csrc/fbk_group_quantile_plan.h"

int main() {
  namespace gp = fbk_gquant_plan;
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    uint64_t a = 0, b = 0, c = 0, d = 0;
    if (kind == 'K') {
      std::printf("%u %u %u %u %" PRIu64 " %u %u\n", gp::kLdsDigitBits, gp::kGlobalDigitBits, gp::lds_pairs_cap(), gp::kAutoLdsPairs, gp::kScratchBound, gp::kMaxDen,
                  gp::kMaxRequests);
    } else if (kind == 'P' && std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c, &d) == 4) {
      std::printf("%u\n", gp::path(a, b, uint32_t(c), uint32_t(d)));
    } else if (kind == 'N' && std::scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) {
      std::printf("%u %u\n", gp::key_bits(uint32_t(a)), gp::passes(uint32_t(a), uint32_t(b)));
    } else if (kind == 'B' && std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3) {
      std::printf("%u %u\n", gp::pass_low(uint32_t(a), uint32_t(b), uint32_t(c)), gp::pass_width(uint32_t(a), uint32_t(b), uint32_t(c)));
    } else if (kind == 'S' && std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c, &d) == 4) {
      std::printf("%" PRIu64 "\n", gp::scratch_bytes(a, b, uint32_t(c), uint32_t(d)));
    } else if (kind == 'C' && std::scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) {
      std::printf("%u\n", gp::densify_chunk(uint32_t(a), b));
    } else if (kind == 'R' && std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3) {
      std::printf("%" PRIu64 "\n", gp::disc_rank(a, uint32_t(b), uint32_t(c)));
    } else {
      std::fprintf(stderr, "bad question '%c'\n", kind);
      return 2;
    }
  }
  return 0;
}
