// Stand-alone driver of featurebase_amd/csrc/fbk_moments_plan.h for tests/test_bsi_moments_cpu.py (built with
// -fsanitize=address,undefined).  One request per input line, one line of integers per request:
//   R dx dy                          -> cx cy mask n packing             the rows of the byte matrix, the column blocks per tile
//   K                                -> kMaxColumnsPerI32 kMaxShards
//   D xe dx hy ye dy hf fe           -> densified rows per shard
//   C n_shards densified             -> the densify chunk
//   F dx dy k (i j v) * k            -> n, then lo hi of sum_x, sum_y, sum_xx, sum_yy, sum_xy (lo unsigned, hi signed);
//                                       cell [i][j] of the 32 x 32 matrix is v, every other cell 0
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../featurebase_amd/csrc/fbk_moments_plan.h"

namespace mp = fbk_moments_plan;

static void put(unsigned __int128 v) { std::printf(" %llu %lld", (unsigned long long)uint64_t(v), (long long)int64_t(uint64_t(v >> 64))); }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char op = 0;
    in >> op;
    if (op == 'R') {
      uint32_t dx, dy;
      in >> dx >> dy;
      const mp::Rows r = mp::rows(dx, dy);
      std::printf("%u %u %u %u %u\n", r.cx, r.cy, r.mask, r.n, mp::packing(r.n));
    } else if (op == 'K') {
      std::printf("%llu %u\n", (unsigned long long)mp::kMaxColumnsPerI32, mp::kMaxShards);
    } else if (op == 'D') {
      uint32_t xe, dx, hy, ye, dy, hf, fe;
      in >> xe >> dx >> hy >> ye >> dy >> hf >> fe;
      std::printf("%llu\n", (unsigned long long)mp::densified_rows(xe, dx, hy, ye, dy, hf, fe));
    } else if (op == 'C') {
      uint32_t ns;
      uint64_t d;
      in >> ns >> d;
      std::printf("%u\n", mp::densify_chunk(ns, d));
    } else if (op == 'F') {
      uint32_t dx, dy, k;
      in >> dx >> dy >> k;
      std::vector<int64_t> S(mp::kCells, 0);
      for (uint32_t t = 0; t < k; ++t) {
        uint32_t i, j;
        int64_t v;
        in >> i >> j >> v;
        S.at(i * mp::kTile + j) = v;
      }
      const mp::Sums s = mp::fold(S.data(), dx, dy);
      std::printf("%llu", (unsigned long long)s.n);
      put(s.x), put(s.y), put(s.xx), put(s.yy), put(s.xy);
      std::printf("\n");
    } else {
      return 2;
    }
    if (!in) return 3;
  }
  return 0;
}
