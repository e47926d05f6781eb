// fbk_minmax_plan.h — host rules of fbk_count_matrix_minmax (HIP-free: compiled into the library and into the stand-alone check of
// the tests, tests/cpp/minmax_plan_check.cpp).  What fbk_matrix_minmax_api.inc decides before it launches, written once:
//   kMinmaxDescentMaxCells  the most groups (n_a * n_b) the plane-descent path takes at all (FBK_MINMAX_DESCENT above it is an error);
//   kMinmaxDescentCells     the most groups FBK_MINMAX_AUTO gives to the descent; above it the per-column scatter runs;
//   path()                  the path of a call from its shape and its flags (0: the flags / shape are an error);
//   descent_grid()          the unit blocks of a descent launch: bounds the partials;
//   densify_chunk()         the shards per pass when an operand goes through DenseOperands (fbk_dense_policy.h's even_chunk).
// The tests read both constants through the checker: they build a case exactly at each boundary.
#pragma once

#include <algorithm>
#include <cstdint>

#include "fbk_dense_policy.h"

namespace fbk_minmax_plan {

constexpr uint32_t kAuto = 0, kDescent = 1, kScatter = 2;  // FBK_MINMAX_AUTO / _DESCENT / _SCATTER (include/fbk.h)

// The descent's work grows with the groups whatever the data (n_a * n_b / 64 lane groups x words x ~2 scans of bit_depth steps):
// sixteen 64-group tiles are the most it is ever asked for.
constexpr uint32_t kMinmaxDescentMaxCells = 1024;
// Fixed from the sweep of scripts/bench_groupby_minmax.py (docs/history/DESIGN_minmax_measurements.md): the largest swept group count
// at which the pinned descent's median time is not above the pinned scatter's (with counts) at depth 20 on mutex-like rows.  That is
// one tile: 2.66 ms against 2.88 ms at 64 groups, 5.26 against 3.40 at 128 (128 shards).  On such rows the scatter does one update per
// column whatever the number of groups, and the descent's work doubles with every doubling of the groups.
constexpr uint32_t kMinmaxDescentCells = 64;
static_assert(kMinmaxDescentMaxCells % 64 == 0 && kMinmaxDescentMaxCells <= 1024, "whole 64-group tiles, at most sixteen");
static_assert(kMinmaxDescentCells % 64 == 0 && kMinmaxDescentCells >= 64 && kMinmaxDescentCells <= kMinmaxDescentMaxCells, "");

// kDescent, kScatter, or 0: unknown flags, or the descent pinned above its cap
inline constexpr uint32_t path(uint64_t n_a, uint64_t n_b, uint32_t flags) {
  const uint64_t cells = n_a * n_b;
  return flags == kAuto      ? (cells <= kMinmaxDescentCells ? kDescent : kScatter)
         : flags == kDescent ? (cells <= kMinmaxDescentMaxCells ? kDescent : 0u)
         : flags == kScatter ? kScatter
                             : 0u;
}

// A descent launch is (unit blocks) x (64-group tiles) blocks of four wavefronts; a block leaves one 64-byte partial per group of
// its tile.  At most kDescentBlocks blocks in all, so the partials of a launch stay within kDescentBlocks * 64 * 64 B = 8 MiB.
constexpr uint32_t kDescentBlocks = 2048;
constexpr uint32_t kUnitsPerShard = 1024;  // units of 16 words of a shard's 16384
inline constexpr uint32_t tiles_of(uint64_t cells) { return uint32_t((cells + 63) / 64); }
inline uint32_t descent_grid(uint32_t n_shards, uint64_t cells) {
  const uint64_t units = uint64_t(n_shards) * kUnitsPerShard;
  return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((units + 3) / 4, kDescentBlocks / tiles_of(cells))));
}

// Shards per pass: at most 2^30 / (2^17 * R) of them (R = the rows densified per shard), dealt evenly over the fewest passes
// (fbk_count_matrix_distinct's stage 2 arithmetic).
constexpr uint64_t kScratch = 1ull << 30;
inline uint32_t densify_chunk(uint32_t n_shards, uint64_t densified) { return fbk::even_chunk(n_shards, kScratch, fbk::kDenseRowBytes * densified); }

}  // namespace fbk_minmax_plan
