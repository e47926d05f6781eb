// fbk_group_walk.hip.h — the per-column walk of the GroupBy aggregates over an int field that scatter by column (lanes = columns):
// Count(Distinct) (fbk_matrix_distinct.hip.h), Min / Max (fbk_matrix_minmax.hip.h's path (b)) and the percentile
// (fbk_group_quantile.hip.h), for DENSE operands.  Included by fbk.hip before fbk_matrix_distinct.hip.h.
//
// A wavefront takes units of kGroupWalkWords 64-column words of one shard, grid-stride.  Per word: valid = exists & F is
// wave-uniform and a word without a column is skipped; the 64 x 64 transpose of the planes gives every lane its column's magnitude;
// transposes of the words of 64 B rows and of 64 A rows give it its membership masks.  What a lane derives from its column (a rank, a
// magnitude class, a key digit) and what it does per (A row, B mask) are the caller's two functors; the launch is the host's
// GroupFieldOperands (fbk_group_field.inc), at most kGroupWalkBlocks blocks of four wavefronts.
#pragma once
#include "fbk_bsi_kernels.hip.h"

namespace fbk {

constexpr uint32_t kGroupWalkWords = 16;     // 64-column words per wavefront unit (a 128-byte line of every row)
constexpr uint32_t kGroupWalkBlocks = 2048;  // most blocks of a launch
constexpr uint64_t kGroupRowWords = (uint64_t)kSlots * 1024;  // u64 words of a dense row

// The operands of a GroupBy kernel over an int field, as parameters and as arguments.  arenaB == nullptr: the one-field form
// (nB == 1).  arenaF == nullptr: no filter.  rowsS[shard] = exists row, + 1 sign, + 2 + p plane p.
#define FBK_GROUP_PARAMS                                                                                                                     \
  const uint8_t *__restrict__ arenaA, const uint32_t *__restrict__ rowsA, uint32_t nA, const uint8_t *__restrict__ arenaB,                  \
      const uint32_t *__restrict__ rowsB, uint32_t nB, const uint8_t *__restrict__ arenaF, const uint32_t *__restrict__ rowsF,               \
      const uint8_t *__restrict__ arenaS, const uint32_t *__restrict__ rowsS, uint32_t depth, uint32_t n_shards
#define FBK_GROUP_ARGS arenaA, rowsA, nA, arenaB, rowsB, nB, arenaF, rowsF, arenaS, rowsS, depth, n_shards

// The A rows [a0, a0 + ta) of the call's nA.
//   column(ex + w, valid_bit, mag) -> on   per word and lane: ex + w is the word of the exists row (the sign's is kGroupRowWords u64
//                                          further), valid_bit the lane's bit of exists & F, mag its column's magnitude.  A lane
//                                          that is not on takes no further part in the word.
//   cell(a_row, wj, bm)                    once per A row (a0 + a_row) the lane's column is in; bm != 0: bit b = the column is
//                                          in B row 64 wj + b (the one-field form: wj = 0, bm = 1).
// kColumnDrops: column() may turn a lane with valid_bit off; then a word that keeps no lane is left before the B rows are read.
template <bool kColumnDrops, class Column, class Cell>
__device__ __forceinline__ void group_column_walk(FBK_GROUP_PARAMS, uint32_t a0, uint32_t ta, Column column, Cell cell) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint64_t kRowWords = kGroupRowWords;
  constexpr uint32_t kUnits = kRowWords / kGroupWalkWords;  // units per shard
  const uint32_t wb = (nB + 63) / 64;
  const TrConst tc = tr_const(lane);
  const uint64_t units = (uint64_t)n_shards * kUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t shard = uint32_t(u / kUnits), w0 = uint32_t(u % kUnits) * kGroupWalkWords;
    const u64* ex = reinterpret_cast<const u64*>(arenaS) + (uint64_t)rowsS[shard] * kRowWords;
    const u64* fl = arenaF ? reinterpret_cast<const u64*>(arenaF) + (uint64_t)rowsF[shard] * kRowWords : nullptr;
    const uint32_t* ra = rowsA + (uint64_t)shard * nA + a0;
    const uint32_t* rb = arenaB ? rowsB + (uint64_t)shard * nB : nullptr;
    for (uint32_t w = w0; w < w0 + kGroupWalkWords; ++w) {
      u64 valid = ex[w];  // (wave-uniform)
      if (fl) valid &= fl[w];
      if (valid == 0) continue;
      // lane p holds plane p's word; transposed, lane c holds the magnitude of column c
      const u64 pw = (uint32_t)lane < depth ? ex[(uint64_t)(2 + lane) * kRowWords + w] : 0ull;
      const u64 mag = wave_transpose64(pw, tc);
      const bool on = column(ex + w, bool((valid >> lane) & 1), mag);
      if constexpr (kColumnDrops) {
        if (__ballot(on) == 0) continue;
      }
      for (uint32_t wj = 0; wj < wb; ++wj) {
        u64 bm = 1;  // the one-field form: every column is in "B row 0"
        if (rb) {
          const uint32_t j = wj * 64 + (uint32_t)lane;
          const u64 bw = j < nB ? reinterpret_cast<const u64*>(arenaB)[(uint64_t)rb[j] * kRowWords + w] : 0ull;
          bm = wave_transpose64(bw, tc);
        }
        const bool onb = on && bm != 0;
        if (__ballot(onb) == 0) continue;
        for (uint32_t wa = 0; wa * 64 < ta; ++wa) {
          const uint32_t ia = wa * 64 + (uint32_t)lane;
          const u64 aw = ia < ta ? reinterpret_cast<const u64*>(arenaA)[(uint64_t)ra[ia] * kRowWords + w] : 0ull;
          u64 am = wave_transpose64(aw, tc);
          if (!onb) am = 0;
          while (am) {
            const uint32_t ka = (uint32_t)__builtin_ctzll(am);
            am &= am - 1;
            cell(wa * 64 + ka, wj, bm);
          }
        }
      }
    }
  }
}

}  // namespace fbk
