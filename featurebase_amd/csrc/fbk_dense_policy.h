// fbk_dense_policy.h — shape rules of the dense count: which plans take k_icount_dense_resident (plan_icount_dense,
// fbk_plan_api.inc) and which pairs a block of its persistent grid walks, in which order; the size of a dense row and how many
// shards of densified rows a chunk of scratch holds (even_chunk).  Plain C++, HIP not needed: scripts/dense_footprint_check.cpp and
// the plan checks under tests/cpp compile it on their own.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define FBK_HD __host__ __device__
#else
#define FBK_HD
#endif

namespace fbk {

// k_icount_dense_resident: block `bid` of `grid` takes the pairs bid, bid + grid, ... below n_pairs — resident_block_pairs of
// them — and iteration `it` of a reversed launch takes the pair that iteration n_it - 1 - it of a forward launch takes.
FBK_HD inline uint32_t resident_block_pairs(uint32_t bid, uint32_t grid, uint32_t n_pairs) {
  return bid < n_pairs ? (n_pairs - bid + grid - 1) / grid : 0u;
}
FBK_HD inline uint32_t resident_pair(uint32_t bid, uint32_t grid, uint32_t it, uint32_t n_it, bool rev) {
  return bid + (rev ? n_it - 1u - it : it) * grid;
}

constexpr uint64_t kDenseRowBytes = 16ull * 8192;  // one dense row: 16 bitmap containers

// Shards per densify chunk (fbk_dense_operands.inc): at most budget / per_shard of them, and the shards dealt evenly over the chunks
// that takes (no short last chunk).  The callers' rules (fbk_minmax_plan.h, fbk_group_quantile_plan.h, fbk_moments_plan.h) and
// their stand-alone checks call it with their own budget.
inline uint32_t even_chunk(uint32_t n_shards, uint64_t budget, uint64_t per_shard) {
  if (n_shards == 0 || per_shard == 0) return n_shards;
  const uint64_t fit = budget / per_shard, most = fit < 1 ? 1 : fit < n_shards ? fit : n_shards;
  const uint64_t chunks = (n_shards + most - 1) / most;
  return uint32_t((n_shards + chunks - 1) / chunks);
}

// Upper bound of the bytes one dense count of a plan reads, from the shape alone (the row lists are not looked at): a plan
// of n_pairs pairs touches at most min(n_pairs, rows) distinct rows of each batch, and at most min(2 * n_pairs, rows) of a
// batch that is both operands.
inline uint64_t dense_footprint_bound(uint64_t n_pairs, uint64_t rows_a, uint64_t rows_b, bool same_batch) {
  const auto mn = [](uint64_t x, uint64_t y) { return x < y ? x : y; };
  const uint64_t rows = same_batch ? mn(2 * n_pairs, rows_a) : mn(n_pairs, rows_a) + mn(n_pairs, rows_b);
  return rows * kDenseRowBytes;
}

// Plans up to this bound take k_icount_dense_resident when they are hot: the size of the Infinity Cache.  Re-read by every
// launch, the resident kernel is ahead of the non-temporal one at every size measured, 128 to 512 MiB (alternating
// directions: the last 256 MiB read are hits whatever the total) — but past the cache's size less and less of a plan can be
// resident, and on rows that are not it is 8 % behind (46.5 against 43.2 us, profiles/dense_resident.txt).
constexpr uint64_t kDenseResidentMaxBytes = 256ull << 20;

}  // namespace fbk
