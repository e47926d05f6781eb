// count_matrix_plan_check.cpp — stand-alone driver of the host rules of the GroupBy count-matrix family
// (featurebase_amd/csrc/fbk_count_matrix_plan.h): which kernel a pass runs, shards per pass, slots per block and the tile counts, each
// asked the way its call site asks (fbk_count_matrix_api.inc, fbk_matrix_sum_api.inc, fbk_count_cube_api.inc); built WITHOUT HIP and
// with -fsanitize=address,undefined by tests/test_count_matrix_plan_cpu.py.
//
//   count_matrix_plan_check < requests
//
// requests (text), one per line; pin = option matrix_spb (0: not pinned):
//   P <n_a> <n_b> <has_filter> <all_dense> <matrix_fused -1|0|1>   -> "<path 0 rows-vs-filter | 1 dense | 2 fused | 3 generic>"
//   S <n_shards> <n_a> <n_b> <matrix_pass_kb> <keep_per_shard>     -> "<pass_shards>"
//   R <units> <n_shards> <floor> <enough> <pin>                    -> "<spb>"                        the rule itself
//   D <n_a> <n_b> <n_shards> <pin>                                 -> "<tm> <tn> <tiles> <spb> <blocks>"   dense
//   F <n_a> <n_b> <n_shards> <n_cu> <pin>                          -> "<tiles> <spb> <blocks>"       fused
//   G <n_a> <n_shards> <pin>                                       -> "<agroups> <spb> <blocks>"     generic: the site passes no pin
//   M <n_a> <n_b> <n_shards> <pin>                                 -> "<tiles> <spb> <blocks>"       sum: the site passes no pin
//   C <n_p> <n_a> <n_b> <n_shards> <pin>                           -> "<pt> <tiles> <spb> <blocks>"  cube
#include <cinttypes>
#include <cstdio>

#include "../../featurebase_amd/csrc/fbk_count_matrix_plan.h"

namespace mp = fbk_count_matrix_plan;

int main() {
  char kind = 0;
  while (std::scanf(" %c", &kind) == 1) {
    uint32_t n_p = 0, n_a = 0, n_b = 0, ns = 0, pin = 0, floor = 0;
    uint64_t kb = 0, units = 0, enough = 0;
    unsigned f = 0, d = 0, keep = 0;
    int fused = 0, n_cu = 0;
    if (kind == 'P') {
      if (std::scanf("%" SCNu32 " %" SCNu32 " %u %u %d", &n_a, &n_b, &f, &d, &fused) != 5) return 2;
      std::printf("%u\n", unsigned(mp::path(n_a, n_b, f != 0, d != 0, fused)));
    } else if (kind == 'S') {
      if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %u", &ns, &n_a, &n_b, &kb, &keep) != 5 || !n_a || !n_b) return 2;
      std::printf("%" PRIu64 "\n", mp::pass_shards(ns, uint64_t(n_a) * n_b, kb, keep != 0));
    } else if (kind == 'R') {
      if (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu32, &units, &ns, &floor, &enough, &pin) != 5) return 2;
      std::printf("%" PRIu32 "\n", mp::slots_per_block(units, ns, floor, enough, pin));
    } else if (kind == 'D') {
      if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &n_a, &n_b, &ns, &pin) != 4) return 2;
      const mp::DenseTiles t = mp::dense_tiles(n_a, n_b);
      const uint32_t spb = mp::slots_per_block(t.tiles, ns, mp::kDenseFloor, mp::kDenseEnough, pin);
      std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", t.tm, t.tn, t.tiles, spb, uint64_t(ns) * (16 / spb) * t.tiles);
    } else if (kind == 'F') {
      if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %d %" SCNu32, &n_a, &n_b, &ns, &n_cu, &pin) != 5) return 2;
      const uint32_t tiles = mp::tiles32(n_a, n_b);
      const uint32_t spb = mp::slots_per_block(tiles, ns, mp::kFusedFloor, mp::fused_enough(n_cu), pin);
      std::printf("%" PRIu32 " %" PRIu32 " %" PRIu64 "\n", tiles, spb, uint64_t(ns) * (16 / spb) * tiles);
    } else if (kind == 'G') {
      if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &n_a, &ns, &pin) != 3) return 2;
      const uint32_t agroups = mp::generic_agroups(n_a);
      const uint32_t spb = mp::slots_per_block(agroups, ns, mp::kGenericFloor, mp::kGenericEnough, 0);
      std::printf("%" PRIu32 " %" PRIu32 " %" PRIu64 "\n", agroups, spb, uint64_t(ns) * (16 / spb) * agroups);
    } else if (kind == 'M') {
      if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &n_a, &n_b, &ns, &pin) != 4) return 2;
      const uint32_t tiles = mp::tiles32(n_a, n_b);
      const uint32_t spb = mp::slots_per_block(tiles, ns, mp::kSumFloor, mp::kSumEnough, 0);
      std::printf("%" PRIu32 " %" PRIu32 " %" PRIu64 "\n", tiles, spb, uint64_t(ns) * (16 / spb) * tiles);
    } else if (kind == 'C') {
      if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &n_p, &n_a, &n_b, &ns, &pin) != 5) return 2;
      const uint64_t tiles = mp::cube_tiles(n_p, n_a, n_b);
      const uint32_t spb = mp::slots_per_block(tiles, ns, mp::kCubeFloor, mp::kCubeEnough, pin);
      std::printf("%" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu64 "\n", mp::cube_pt(n_p), tiles, spb, uint64_t(ns) * (16 / spb) * tiles);
    } else {
      return 2;
    }
  }
  return 0;
}
