// dense_footprint_check.cpp — stand-alone check of the shape rule that sends a hot dense plan to k_icount_dense_resident and
// of the map (block, iteration, direction) -> pair of its persistent grid (featurebase_amd/csrc/fbk_dense_policy.h).  Host code only:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined scripts/dense_footprint_check.cpp -o build/dense_footprint_check && build/dense_footprint_check
#include <cstdio>
#include <vector>

#include "../featurebase_amd/csrc/fbk_dense_policy.h"

static int failures = 0;
#define EXPECT(c)                                            \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++failures;                                            \
    }                                                        \
  } while (0)

int main() {
  using fbk::dense_footprint_bound;
  constexpr uint64_t MiB = 1ull << 20, row = 128ull << 10;
  static_assert(fbk::kDenseRowBytes == row, "a dense row is 16 containers of 8 KiB");
  static_assert(fbk::kDenseResidentMaxBytes <= 256 * MiB, "never above the size of the Infinity Cache");
  // the benchmark's plan: 1024 pairs over two batches of 1024 rows — exactly 256 MiB, and it qualifies
  EXPECT(dense_footprint_bound(1024, 1024, 1024, false) == 256 * MiB);
  EXPECT(dense_footprint_bound(1024, 1024, 1024, false) <= fbk::kDenseResidentMaxBytes);
  // one row more on either side does not
  EXPECT(dense_footprint_bound(1025, 1025, 1024, false) == 256 * MiB + row);
  EXPECT(dense_footprint_bound(1025, 1024, 1025, false) > fbk::kDenseResidentMaxBytes);
  EXPECT(dense_footprint_bound(1032, 1032, 1032, false) == 258 * MiB);
  // many pairs over small batches: the batches bound it, not the pairs
  EXPECT(dense_footprint_bound(1u << 27, 2, 2, false) == 4 * row);
  EXPECT(dense_footprint_bound(1u << 27, 8, 8, true) == 8 * row);
  // few pairs over large batches: the pairs bound it
  EXPECT(dense_footprint_bound(3, 100000, 100000, false) == 6 * row);
  EXPECT(dense_footprint_bound(3, 100000, 100000, true) == 6 * row);
  // one batch as both operands: its rows count once
  EXPECT(dense_footprint_bound(2048, 2048, 2048, true) == 256 * MiB);
  EXPECT(dense_footprint_bound(2048, 2048, 2048, false) == 512 * MiB);
  EXPECT(dense_footprint_bound(1024, 2049, 2049, true) == 256 * MiB);
  EXPECT(dense_footprint_bound(1025, 2051, 2051, true) > fbk::kDenseResidentMaxBytes);
  // the largest plan (2^27 pairs) over the largest batches (2^32 - 1 rows): no overflow
  EXPECT(dense_footprint_bound(1ull << 27, 0xFFFFFFFFull, 0xFFFFFFFFull, false) == (2ull << 27) * row);
  EXPECT(dense_footprint_bound(0, 5, 5, false) == 0);
  // the persistent grid's map: every pair exactly once, in either direction, and the reversed walk is the exact mirror
  for (uint32_t grid : {1u, 2u, 3u, 8u, 256u})
    for (uint32_t n_pairs : {1u, 2u, 3u, grid - 1, grid, grid + 1, 2 * grid + 3, 7 * grid}) {
      if (n_pairs == 0) continue;
      const uint32_t g = n_pairs < grid ? n_pairs : grid;  // the launch: min(n_pairs, G) blocks
      for (int rev = 0; rev < 2; ++rev) {
        std::vector<int> seen(n_pairs, 0);
        for (uint32_t bid = 0; bid < g; ++bid) {
          const uint32_t n_it = fbk::resident_block_pairs(bid, g, n_pairs);
          EXPECT(n_it >= 1);
          for (uint32_t it = 0; it < n_it; ++it) {
            const uint32_t pair = fbk::resident_pair(bid, g, it, n_it, rev != 0);
            EXPECT(pair < n_pairs);
            if (pair < n_pairs) ++seen[pair];
            EXPECT(pair == fbk::resident_pair(bid, g, n_it - 1 - it, n_it, rev == 0));
          }
        }
        for (uint32_t i = 0; i < n_pairs; ++i) EXPECT(seen[i] == 1);
      }
    }
  EXPECT(fbk::resident_block_pairs(5, 4, 3) == 0);
  if (failures) return 1;
  std::printf("dense footprint ok\n");
  return 0;
}
