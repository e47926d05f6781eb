// fbk_count_matrix_plan.h — host rules of the GroupBy count-matrix family (HIP-free: compiled into the library and into the stand-alone
// check of the tests, tests/cpp/count_matrix_plan_check.cpp).  What fbk_count_matrix (fbk_count_matrix_api.inc), fbk_count_matrix_sum
// and fbk_count_cube decide before they launch, written once:
//   path()             which of the count matrix's four kernels a pass runs;
//   pass_shards()      how many shards one pass holds under option matrix_pass_kb;
//   slots_per_block()  how many of a shard's 16 container slots one block covers, with each call site's floor and block count;
//   the tile counts the call sites multiply it with.
#pragma once

#include <algorithm>
#include <cstdint>

namespace fbk_count_matrix_plan {

enum Path : uint32_t { kRowsVsFilter = 0, kDense = 1, kFused = 2, kGeneric = 3 };

// Encoded rows: the generic pair kernel (k_count_matrix<4>), or the matrix-core kernel that decodes the rows in place
// (fbk_matrix_fusedq.hip.h)?  Round 4, scripts/small_shapes_ab.py, 64 shards of config 3's rows, interleaved in one process
// (profiles/r04_small_shapes_ab.json): the fused kernel costs 65-75 us whatever the shape up to a 32 x 32 tile (it decodes
// every row once), the generic kernel ~38 us + 1.5 us per pair — 2 x 2: 44 against 65 us, 8 x 8: 139 against 70, 4 x 16: 156
// against 70, 3 x 30: 241 against 73.  From 16 pairs per shard on the rows are decoded once.  (Rounds 1-4 had a third path —
// rows densified into temporary bitmap rows, then the dense kernel: 681 + 347 us against ~400 us for the first in-kernel
// decode on 256 shards of config 3's rows, never chosen since round 2 — removed in round 5.)
inline bool prefers_fused(uint32_t n_a, uint32_t n_b) { return uint64_t(n_a) * n_b >= 16; }

// all_dense: every container of the three batches a bitmap at a fixed address; matrix_fused: the option — 1 / 0 pins the in-kernel
// decode / the generic pair kernel, -1: by the matrix size (prefers_fused)
inline Path path(uint32_t n_a, uint32_t n_b, bool has_filter, bool all_dense, int matrix_fused) {
  if (n_b == 1 && !has_filter) return kRowsVsFilter;  // many rows x one row (doTopK / fragment.top): the single B row is the filter of k_rows_vs_filter
  if (all_dense && n_b > 1) return kDense;            // the matrix-core kernel (fbk_matrix_mfma.hip.h)
  if (n_b > 1 && matrix_fused != 0 && (matrix_fused == 1 || prefers_fused(n_a, n_b))) return kFused;
  return kGeneric;
}

// The per-shard matrices (the reference's per-shard map results) are only an intermediate of the reduce over shards when the caller
// does not ask for them, so the shards are processed in passes of at most matrix_pass_kb (~1 GiB) of per-shard matrices each (a
// 1000 x 1000 GroupBy over 1024 shards would otherwise need 8 GB for them).  width = n_a * n_b > 0; tests force several passes.
inline uint64_t pass_shards(uint32_t n_shards, uint64_t width, uint64_t matrix_pass_kb, bool keep_per_shard) {
  const uint64_t pass_bytes = matrix_pass_kb << 10;
  return std::max<uint64_t>(1, keep_per_shard ? n_shards : std::min<uint64_t>(n_shards, pass_bytes / (width * 8)));
}

// Slots per block: 16 (whole shards, plain stores), halved (atomic adds into the per-shard matrix) while it is above `floor` and the
// grid — n_shards * (16 / spb) * units_per_shard_at_16 blocks — holds fewer than `enough` blocks.  pinned != 0 (option matrix_spb =
// 1|2|4|8|16, tests walk every value) replaces the result, below the floor too; a site that does not honour the option passes 0.
inline uint32_t slots_per_block(uint64_t units_per_shard_at_16, uint32_t n_shards, uint32_t floor, uint64_t enough, uint32_t pinned) {
  uint32_t spb = 16;
  while (spb > floor && uint64_t(n_shards) * (16 / spb) * units_per_shard_at_16 < enough) spb >>= 1;
  return pinned ? pinned : spb;
}

// 32 x 32 tiles of an n_a x n_b matrix
inline uint32_t tiles32(uint32_t n_a, uint32_t n_b) { return ((n_a + 31) / 32) * ((n_b + 31) / 32); }

// The dense kernel: a side of more than 32 rows gets two 32-row tiles per block: the operand expansion of the
// other side is reused, which is what bounds a matrix of many tiles (scripts/tune_matrix.hip)
struct DenseTiles {
  uint32_t tm, tn, tiles;
};
inline DenseTiles dense_tiles(uint32_t n_a, uint32_t n_b) {
  const uint32_t tm = n_a > 32 ? 2 : 1, tn = n_b > 32 ? 2 : 1;
  return {tm, tn, ((n_a + 32 * tm - 1) / (32 * tm)) * ((n_b + 32 * tn - 1) / (32 * tn))};
}
// Slots per block: 2 blocks fit a CU, so 512 run at a time — with one block per shard (spb 16) the 1024 shards a rank of BASELINE
// configs[3] owns are two rounds of ~700 us blocks and whatever the slowest CU loses shows in full; ~8192 blocks (16 rounds)
// even that out at the price of atomic adds into the per-shard matrix.  scripts/matrix_spb_sweep.py, 1024 shards x 32 x 32 +
// filter, interleaved in one process (profiles/r04_matrix_spb_sweep.json): spb 16 1382 us (1356 .. 1443), spb 4 1372 (1368 ..
// 1388), spb 2 1364 (1354 .. 1379): from ~4096 blocks (8 rounds) on it no longer matters.
constexpr uint32_t kDenseFloor = 2;
constexpr uint64_t kDenseEnough = 4096;

// The fused kernel: one block per (shard, slot group, 32 x 32 tile); its 160 KB of LDS give one block per CU at a time.
// (one block per CU at a time; a block builds its work lists once per slot and pays a set-up and a final reduction, so
// fewer, longer blocks win as long as every CU has one: 256 shards, spb 16 / 8 / 4 / 2 = 256 / 512 / 1024 / 2048 blocks:
// 329 / 333 / 339 / 355 us, profiles/r04_fused_spb_sweep.json)
// (units by ticket, as the dense launch takes them, were tried here in round 6 — profiles/r06_tickets_ab_fused.json: config 3's 256
// shards 261 -> 284 us at 4 slots per unit, config 4's log-uniform rows 1013 -> 1032 us: this kernel is bound by the CU's instruction
// issue, not by HBM, so the XCDs' different memory paces do not show, and a ticket costs an atomic round trip that nothing hides with
// one block per CU)
constexpr uint32_t kFusedFloor = 2;
inline uint64_t fused_enough(int n_cu) { return uint64_t(std::max(n_cu, 1)); }

// The generic pair kernel (k_count_matrix<kGenericTA>): a block takes a group of 8 * TA rows of A.  Enough blocks to fill 256 CUs:
// whole rows per block (plain stores) when there are many shards, otherwise split the 16 slots over several blocks (atomic adds)
constexpr int kGenericTA = 4;
inline uint32_t generic_agroups(uint32_t n_a) { return (n_a + 8 * kGenericTA - 1) / (8 * kGenericTA); }
constexpr uint32_t kGenericFloor = 1;
constexpr uint64_t kGenericEnough = 1024;

// GroupBy Sum and the cube: whole shards while the grid still holds ~2048 blocks, fewer slots (more atomics) below
constexpr uint32_t kSumFloor = 1, kCubeFloor = 1;
constexpr uint64_t kSumEnough = 2048, kCubeEnough = 2048;

// The cube: P rows per block: 8 accumulators share one B expansion; a field of at most 4 rows would spend half of them on repeats
inline uint32_t cube_pt(uint32_t n_p) { return n_p <= 4 ? 4 : 8; }
inline uint64_t cube_tiles(uint32_t n_p, uint32_t n_a, uint32_t n_b) {
  const uint32_t pt = cube_pt(n_p);
  return uint64_t((n_p + pt - 1) / pt) * ((n_a + 31) / 32) * ((n_b + 31) / 32);
}

}  // namespace fbk_count_matrix_plan
