// fbk_matrix_minmax.hip.h — GroupBy with Min / Max of an int field per group (SQL SELECT a, b, MIN(x), MAX(x) ... GROUP BY a, b;
// per group fragment.min / fragment.max, fragment.go:754-853, folded over the shards by ValCount.Smaller / Larger,
// executor.go:8446-8548) for all (A row, B row) groups at once, for DENSE operands.
//
// A column's value is sign ? -magnitude : magnitude, up to 65 bits at depth 64, so a group is kept as four UNSIGNED magnitudes of
// two classes: the negatives are the columns with the sign set and magnitude != 0, everything else of the group is positive (a
// set sign over magnitude 0 is the value 0).
//   [0] maxmag_neg  [1] minmag_neg  [2] minmag_pos  [3] maxmag_pos      identities: max 0, min ~0
//   min = (maxmag_neg >= 1) ? -maxmag_neg : minmag_pos          max = (the group has a positive) ? maxmag_pos : -minmag_neg
// written as int64 with wrap-around (as fbk_bsi_min / fbk_bsi_max); neither a flag word nor a 65-bit key is needed.  An empty group
// is INT64_MAX / INT64_MIN with counts 0.
//
// Two paths (the rule between them: fbk_minmax_plan.h):
//  (a) plane descent, lanes = groups — few groups.
//   k_minmax_descent  grid (unit blocks, 64-group tiles).  A wavefront owns the tile's 64 groups (lane = group) and walks units of
//                     kGroupWalkWords consecutive 64-column words of a shard (grid-stride).  Per word the wave-uniform words — exists
//                     & F, sign, the OR of the planes, the planes — come through scalar loads (their addresses are uniform), four
//                     words (32 bytes) of a row per load: a word at a time every scan step waited on a load of its own; the
//                     lane forms m = A_i & B_j & valid, neg = m & sign & anymag, pos = m & ~neg and runs the reference's
//                     MSB -> LSB scans on its own 64-bit masks: maxmag(S): t = S & P_k, t != 0 ? S = t, bit k set; minmag(S) the
//                     same with ~P_k.  The surviving S holds the holders: popcount(S) is the count, so values and counts come from
//                     ONE pass.  Only the two scans that can matter run: for the min, neg != 0 ? maxmag(neg) : minmag(pos); for the
//                     max, pos != 0 ? maxmag(pos) : minmag(neg).  (So magnitudes [1] and [2] are complete only when the final
//                     formula reads them, and "the group has a positive" is count[3] > 0 on this path.)  A lane with m == 0 skips
//                     the scans, a word with valid == 0 is skipped by the wave.  The block's four waves fold through LDS into ONE
//                     64-byte partial per (block, group): [unit block][tile][64] x {4 magnitudes, 4 counts}.
//                     Work: n_a n_b / 64 lane groups x words with valid != 0 x 2 scans x bit_depth steps (~10 vector instructions
//                     each), whatever the rows hold; bytes: the planes, the filter and every A / B row once per TILE.
//                     The grid is at most fbk_minmax_plan::kDescentBlocks blocks: partials <= 2048 x 64 groups x 64 B = 8 MiB.
//   k_minmax_fold     one wavefront per group: the partials of a launch folded in a fixed order (lanes over blocks, then a
//                     butterfly), no atomics; into the running state when the call takes several chunks of shards; after the last
//                     one converted to the int64 / count outputs.
//  (b) per-column scatter, lanes = columns — many groups.
//   k_minmax_scatter  group_column_walk (fbk_group_walk.hip.h): a lane's column is negative where the sign is set and the walk's
//                     magnitude is not 0, and every column of exists & F takes part; for each (i, j) of its masks the lane
//                     updates the group's two magnitudes of its class in state[groups][4] with 64-bit atomicMax / atomicMin
//                     (global_atomic_umax_x2 / umin_x2: no compare-and-swap loop).  The state only moves one way, so before each
//                     atomic the lane reads the magnitude with a relaxed agent-scope load (it bypasses L1) and skips an atomic
//                     that cannot improve it: in a skewed or low-cardinality group almost every atomic becomes a load.
//   k_minmax_holders  (counts asked for) the same walk again: a lane whose (class, magnitude) is its group's final minimum
//                     (maximum) adds 1 to the group's min (max) count.
//   k_minmax_finish   state and counts -> the outputs.
//                     Work: Σ over columns of |A rows holding it| x |B rows holding it| updates: optimal for mutex-like fields,
//                     poor for set fields with many rows per column.  Scratch: 48 B per group (768 MiB at 4096 x 4096), not tiled.
#pragma once
#include "fbk_group_walk.hip.h"

namespace fbk {

constexpr uint32_t kMinmaxStep = 4;  // words per step of the descent
struct alignas(32) MinmaxWords {     // kMinmaxStep consecutive words of a row
  u64 w[kMinmaxStep];
};
static_assert(kGroupWalkWords % kMinmaxStep == 0, "");

struct MinmaxPartial {  // 64 bytes
  u64 mag[4];           // maxmag_neg, minmag_neg, minmag_pos, maxmag_pos
  u64 cnt[4];           // their holders
};

__device__ __forceinline__ MinmaxPartial mm_identity() { return {{0ull, ~0ull, ~0ull, 0ull}, {0ull, 0ull, 0ull, 0ull}}; }
__device__ __forceinline__ void mm_fold_max(u64& mag, u64& cnt, u64 m, u64 c) {
  cnt = m > mag ? c : m == mag ? cnt + c : cnt;
  mag = m > mag ? m : mag;
}
__device__ __forceinline__ void mm_fold_min(u64& mag, u64& cnt, u64 m, u64 c) {
  cnt = m < mag ? c : m == mag ? cnt + c : cnt;
  mag = m < mag ? m : mag;
}
__device__ __forceinline__ void mm_fold(MinmaxPartial& a, const MinmaxPartial& b) {
  mm_fold_max(a.mag[0], a.cnt[0], b.mag[0], b.cnt[0]);
  mm_fold_min(a.mag[1], a.cnt[1], b.mag[1], b.cnt[1]);
  mm_fold_min(a.mag[2], a.cnt[2], b.mag[2], b.cnt[2]);
  mm_fold_max(a.mag[3], a.cnt[3], b.mag[3], b.cnt[3]);
}
// the four magnitudes -> the outputs; cmin / cmax: the holders of the chosen magnitudes
__device__ __forceinline__ void mm_write(const u64* mag, bool pos_any, u64 c_maxneg, u64 c_minneg, u64 c_minpos, u64 c_maxpos, uint64_t at,
                                         long long* __restrict__ out_min, long long* __restrict__ out_max, u64* __restrict__ out_cmin,
                                         u64* __restrict__ out_cmax) {
  const bool neg_any = mag[0] >= 1;
  out_min[at] = neg_any ? (long long)(0ull - mag[0]) : pos_any ? (long long)mag[2] : INT64_MAX;
  out_max[at] = pos_any ? (long long)mag[3] : neg_any ? (long long)(0ull - mag[1]) : INT64_MIN;
  if (out_cmin) {
    out_cmin[at] = neg_any ? c_maxneg : pos_any ? c_minpos : 0ull;
    out_cmax[at] = pos_any ? c_maxpos : neg_any ? c_minneg : 0ull;
  }
}

// ---- (a) plane descent ---------------------------------------------------------------------------------------------------------
// grid (unit blocks, ceil(nA * nB / 64)).  partial: [gridDim.x][gridDim.y][64].
__global__ void __launch_bounds__(256) k_minmax_descent(FBK_GROUP_PARAMS, MinmaxPartial* __restrict__ partial) {
  __shared__ u64 sh[3][8][64];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint64_t kRowWords = (uint64_t)kSlots * 1024;  // u64 words of a row
  constexpr uint32_t kUnits = kRowWords / kGroupWalkWords;  // units per shard
  const uint32_t cell = blockIdx.y * 64 + (uint32_t)lane;
  const bool live = cell < nA * nB;
  const uint32_t i = live ? cell / nB : 0, j = live ? cell % nB : 0;
  MinmaxPartial st = mm_identity();
  // the wave's units (shard, unit of the shard), grid-stride, in 32-bit counters: the grid is at most 2048 x 4 waves (fbk_minmax_plan.h)
  for (uint32_t uu = blockIdx.x * 4 + wv, shard = uu / kUnits; shard < n_shards; uu += gridDim.x * 4, shard += uu / kUnits) {
    uu %= kUnits;
    const uint32_t w0 = uu * kGroupWalkWords;
    const u64* ex = reinterpret_cast<const u64*>(arenaS) + (uint64_t)rowsS[shard] * kRowWords;  // (wave-uniform, as fl and every ex[...] below)
    const u64* fl = arenaF ? reinterpret_cast<const u64*>(arenaF) + (uint64_t)rowsF[shard] * kRowWords : nullptr;
    const u64* pa = reinterpret_cast<const u64*>(arenaA) + (uint64_t)rowsA[(uint64_t)shard * nA + i] * kRowWords;
    const u64* pb = arenaB ? reinterpret_cast<const u64*>(arenaB) + (uint64_t)rowsB[(uint64_t)shard * nB + j] * kRowWords : nullptr;
    for (uint32_t w = w0; w < w0 + kGroupWalkWords; w += kMinmaxStep) {
      // kMinmaxStep words at a time: one 32-byte scalar load per uniform row and step, and four independent scans per lane
      const MinmaxWords e = *reinterpret_cast<const MinmaxWords*>(ex + w);
      u64 valid[kMinmaxStep], m[kMinmaxStep], many = 0;
      for (uint32_t q = 0; q < kMinmaxStep; ++q) valid[q] = e.w[q];
      if (fl) {
        const MinmaxWords f = *reinterpret_cast<const MinmaxWords*>(fl + w);
        for (uint32_t q = 0; q < kMinmaxStep; ++q) valid[q] &= f.w[q];
      }
      if ((valid[0] | valid[1] | valid[2] | valid[3]) == 0) continue;
      {
        const MinmaxWords a = *reinterpret_cast<const MinmaxWords*>(pa + w);
        for (uint32_t q = 0; q < kMinmaxStep; ++q) m[q] = live ? a.w[q] & valid[q] : 0ull;
      }
      if (pb) {
        const MinmaxWords b = *reinterpret_cast<const MinmaxWords*>(pb + w);
        for (uint32_t q = 0; q < kMinmaxStep; ++q) m[q] &= b.w[q];
      }
      for (uint32_t q = 0; q < kMinmaxStep; ++q) many |= m[q];
      if (__ballot(many != 0) == 0) continue;
      u64 anymag[kMinmaxStep] = {0ull, 0ull, 0ull, 0ull};  // (per lane, in vector registers: as scalars the kernel spills scalar registers)
      for (uint32_t k = 0; k < depth; ++k) {
        const MinmaxWords p = *reinterpret_cast<const MinmaxWords*>(ex + (uint64_t)(2 + k) * kRowWords + w);
        for (uint32_t q = 0; q < kMinmaxStep; ++q) anymag[q] |= p.w[q] & m[q];
      }
      const MinmaxWords sign = *reinterpret_cast<const MinmaxWords*>(ex + kRowWords + w);
      if (many != 0) {
        // scan 1, the minimum: the largest magnitude of neg, else the smallest of pos; scan 2, the maximum: the largest of pos, else
        // the smallest of neg.  inv: the scan is a minmag (it keeps the columns WITHOUT plane k, and a plane nobody lacks is a 1)
        u64 inv1[kMinmaxStep], inv2[kMinmaxStep], s1[kMinmaxStep], s2[kMinmaxStep], v1[kMinmaxStep], v2[kMinmaxStep];
        for (uint32_t q = 0; q < kMinmaxStep; ++q) {
          const u64 neg = m[q] & sign.w[q] & anymag[q], pos = m[q] & ~neg;
          inv1[q] = neg ? 0ull : ~0ull, inv2[q] = pos ? 0ull : ~0ull;
          s1[q] = neg ? neg : pos, s2[q] = pos ? pos : neg, v1[q] = 0, v2[q] = 0;
        }
        for (uint32_t k = depth; k-- > 0;) {
          const MinmaxWords p = *reinterpret_cast<const MinmaxWords*>(ex + (uint64_t)(2 + k) * kRowWords + w);
#pragma unroll
          for (uint32_t q = 0; q < kMinmaxStep; ++q) {
            const u64 t1 = s1[q] & (p.w[q] ^ inv1[q]), t2 = s2[q] & (p.w[q] ^ inv2[q]);
            s1[q] = t1 ? t1 : s1[q];
            s2[q] = t2 ? t2 : s2[q];
            v1[q] = (v1[q] << 1) | (u64(t1 != 0) ^ (inv1[q] & 1));
            v2[q] = (v2[q] << 1) | (u64(t2 != 0) ^ (inv2[q] & 1));
          }
        }
#pragma unroll
        for (uint32_t q = 0; q < kMinmaxStep; ++q) {
          if (m[q] == 0) continue;
          const u64 c1 = (u64)__popcll(s1[q]), c2 = (u64)__popcll(s2[q]);
          if (inv1[q] == 0) mm_fold_max(st.mag[0], st.cnt[0], v1[q], c1);  // (the word has negatives)
          else mm_fold_min(st.mag[2], st.cnt[2], v1[q], c1);
          if (inv2[q] == 0) mm_fold_max(st.mag[3], st.cnt[3], v2[q], c2);  // (the word has positives)
          else mm_fold_min(st.mag[1], st.cnt[1], v2[q], c2);
        }
      }
    }
  }
  // the block's waves through LDS, one partial per (block, group)
  if (wv > 0) {
    for (int q = 0; q < 4; ++q) sh[wv - 1][q][lane] = st.mag[q], sh[wv - 1][4 + q][lane] = st.cnt[q];
  }
  __syncthreads();
  if (wv == 0) {
    for (int o = 0; o < 3; ++o) {
      MinmaxPartial other;
      for (int q = 0; q < 4; ++q) other.mag[q] = sh[o][q][lane], other.cnt[q] = sh[o][4 + q][lane];
      mm_fold(st, other);
    }
    partial[((uint64_t)blockIdx.x * gridDim.y + blockIdx.y) * 64 + lane] = st;
  }
}

// One wavefront per group.  partial: [blocks][cells_p] (cells_p = the tiles' 64 groups each); state: [cells], read unless `first`,
// written always; the outputs are written when `last` (out_cmin == nullptr: no counts).
__global__ void __launch_bounds__(256) k_minmax_fold(const MinmaxPartial* __restrict__ partial, uint32_t blocks, uint32_t cells_p, uint32_t cells,
                                                     MinmaxPartial* __restrict__ state, int first, int last, long long* __restrict__ out_min,
                                                     long long* __restrict__ out_max, u64* __restrict__ out_cmin, u64* __restrict__ out_cmax) {
  const int lane = threadIdx.x & 63;
  const uint32_t cell = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (cell >= cells) return;  // (wave-uniform)
  MinmaxPartial acc = mm_identity();
  for (uint32_t b = (uint32_t)lane; b < blocks; b += 64) mm_fold(acc, partial[(uint64_t)b * cells_p + cell]);
  for (int off = 32; off > 0; off >>= 1) {
    MinmaxPartial other;
    for (int q = 0; q < 4; ++q) {
      other.mag[q] = (u64)__shfl_xor((unsigned long long)acc.mag[q], off);
      other.cnt[q] = (u64)__shfl_xor((unsigned long long)acc.cnt[q], off);
    }
    mm_fold(acc, other);
  }
  if (lane != 0) return;
  if (!first) mm_fold(acc, state[cell]);
  state[cell] = acc;
  if (last) mm_write(acc.mag, acc.cnt[3] > 0, acc.cnt[0], acc.cnt[1], acc.cnt[2], acc.cnt[3], cell, out_min, out_max, out_cmin, out_cmax);
}

// ---- (b) per-column scatter ----------------------------------------------------------------------------------------------------
// state: [nA * nB][4] magnitudes; counts: [nA * nB][2] (min holders, max holders)
__global__ void __launch_bounds__(256) k_minmax_init(u64* __restrict__ state, u64* __restrict__ counts, uint64_t cells) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  state[c * 4 + 0] = 0ull, state[c * 4 + 1] = ~0ull, state[c * 4 + 2] = ~0ull, state[c * 4 + 3] = 0ull;
  counts[c * 2] = 0ull, counts[c * 2 + 1] = 0ull;
}

// kHolders == false: the magnitudes (state is updated); true: the holders of the final magnitudes (state is read, counts updated)
template <bool kHolders>
__device__ __forceinline__ void minmax_walk(FBK_GROUP_PARAMS, u64* state, u64* counts) {
  const int lane = threadIdx.x & 63;
  u64 mag = 0;                // of the lane's column
  bool isneg = false;         // its class: the sign is set and mag != 0
  int hi = 3, lo = 2;         // the class's maxmag / minmag
  group_column_walk<false>(
      FBK_GROUP_ARGS, 0, nA,
      [&](const u64* exw, bool valid, u64 m) {
        mag = m;
        isneg = ((exw[kGroupRowWords] >> lane) & 1) && mag != 0;
        hi = isneg ? 0 : 3, lo = isneg ? 1 : 2;
        return valid;
      },
      [&](uint32_t a_row, uint32_t wj, u64 bm) {
        for (u64 b = bm; b; b &= b - 1) {
          const uint64_t cell = (uint64_t)a_row * nB + wj * 64 + (uint32_t)__builtin_ctzll(b);
          u64* st = state + cell * 4;
          if constexpr (!kHolders) {
            if (mag > __hip_atomic_load(st + hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
              atomicMax(reinterpret_cast<unsigned long long*>(st + hi), (unsigned long long)mag);
            if (mag < __hip_atomic_load(st + lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
              atomicMin(reinterpret_cast<unsigned long long*>(st + lo), (unsigned long long)mag);
          } else {
            const bool neg_any = st[0] >= 1, pos_any = st[2] <= st[3];
            const bool is_min = neg_any ? (isneg && mag == st[0]) : (!isneg && mag == st[2]);
            const bool is_max = pos_any ? (!isneg && mag == st[3]) : (isneg && mag == st[1]);
            if (is_min) atomicAdd(reinterpret_cast<unsigned long long*>(counts + cell * 2), 1ull);
            if (is_max) atomicAdd(reinterpret_cast<unsigned long long*>(counts + cell * 2 + 1), 1ull);
          }
        }
      });
}

__global__ void __launch_bounds__(256) k_minmax_scatter(FBK_GROUP_PARAMS, u64* state) { minmax_walk<false>(FBK_GROUP_ARGS, state, nullptr); }

__global__ void __launch_bounds__(256) k_minmax_holders(FBK_GROUP_PARAMS, u64* state, u64* __restrict__ counts) {
  minmax_walk<true>(FBK_GROUP_ARGS, state, counts);
}

// out_cmin == nullptr: no counts
__global__ void __launch_bounds__(256) k_minmax_finish(const u64* __restrict__ state, const u64* __restrict__ counts, uint64_t cells,
                                                       long long* __restrict__ out_min, long long* __restrict__ out_max,
                                                       u64* __restrict__ out_cmin, u64* __restrict__ out_cmax) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const u64 mag[4] = {state[c * 4], state[c * 4 + 1], state[c * 4 + 2], state[c * 4 + 3]};
  const u64 cmin = counts[c * 2], cmax = counts[c * 2 + 1];
  mm_write(mag, mag[2] <= mag[3], cmin, cmax, cmin, cmax, c, out_min, out_max, out_cmin, out_cmax);
}

}  // namespace fbk
