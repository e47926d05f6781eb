// fbk_matrix_distinct.hip.h — GroupBy with aggregate=Count(Distinct(field=v)) (executor.go:3338-3386: one Count(Distinct(
// Intersect(group rows, filter))) per result group) for all (A row, B row) groups at once, for DENSE operands.
//
// The distinct values U of exists ∩ F over all shards come first, sorted (fbk_bsi_distinct's device half).  Then every column
// of exists ∩ F has a rank r = the index of its value in U, and a group's distinct count is the number of ranks some column of
// the group holds: a presence bitmap per A row and rank, one bit per B row,
//   P[i][w][r] bit b = some column of A_i ∩ B_(64 w + b) ∩ F ∩ exists holds the value U[r],
// and distinct[i][j] = Σ_r bit (j mod 64) of P[i][j / 64][r].  The presence bitmap of one call can be large (n_a x m x n_b bits):
// the host tiles it in blocks of A rows [a0, a0 + ta) and ranges of ranks [r0, r0 + tr), each tile one scatter over the operands
// and one popcount pass.
//
// Two kernels:
//   k_mdist_scatter   one wavefront per run of kMdistWords 64-column words of one shard (grid-stride): per word the 64 x 64
//                     transpose of the planes gives every lane its column's value (as k_bsi_values), a binary search in U its
//                     rank (the search tree's top, kMdistFences values of U, staged in LDS; the rest in U itself), transposes
//                     of the words of 64 B rows and 64 A rows its membership masks; per A row the lane holds, one atomicOr of
//                     its B mask into P.  Atomics: Σ_c |A(c)| x ceil(n_b / 64) over the columns with a value in the tile.
//   k_mdist_popcount  one wavefront per (A row, B word, part of the ranks): 64 ranks' words at a time, transposed so that lane
//                     b holds the 64 ranks' bits of B row 64 w + b, popcounts added to the result.
#pragma once
#include "fbk_bsi_kernels.hip.h"

namespace fbk {

constexpr uint32_t kMdistFences = 4096;  // values of U staged in LDS per block (32 KiB): every stride-th one
constexpr uint32_t kMdistWords = 16;     // 64-column words per wavefront unit (a 128-byte line of every row)

// P: [ta][ceil(nB / 64)][tr] u64, zeroed by the caller; tr a multiple of 64.  arenaB == nullptr: the one-field form (nB == 1).
// rowsS[shard] = exists row, + 1 sign, + 2 + p plane p.  U: the m sorted distinct values (m >= 1).
__global__ void __launch_bounds__(256) k_mdist_scatter(const uint8_t* __restrict__ arenaA, const uint32_t* __restrict__ rowsA, uint32_t nA,
                                                       uint32_t a0, uint32_t ta, const uint8_t* __restrict__ arenaB,
                                                       const uint32_t* __restrict__ rowsB, uint32_t nB, const uint8_t* __restrict__ arenaF,
                                                       const uint32_t* __restrict__ rowsF, const uint8_t* __restrict__ arenaS,
                                                       const uint32_t* __restrict__ rowsS, uint32_t depth, const long long* __restrict__ U,
                                                       uint32_t m, uint32_t r0, uint32_t tr, uint32_t n_shards, u64* __restrict__ P) {
  __shared__ long long fence[kMdistFences];
  const uint32_t stride = (m + kMdistFences - 1) / kMdistFences, nf = (m + stride - 1) / stride;
  for (uint32_t t = threadIdx.x; t < nf; t += 256) fence[t] = U[(uint64_t)t * stride];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint64_t kRowWords = (uint64_t)kSlots * 1024;  // u64 words of a row
  constexpr uint32_t kUnits = kRowWords / kMdistWords;     // units per shard
  const uint32_t wb = (nB + 63) / 64;
  const TrConst tc = tr_const(lane);
  const uint64_t units = (uint64_t)n_shards * kUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t shard = uint32_t(u / kUnits), w0 = uint32_t(u % kUnits) * kMdistWords;
    const u64* ex = reinterpret_cast<const u64*>(arenaS) + (uint64_t)rowsS[shard] * kRowWords;
    const u64* fl = arenaF ? reinterpret_cast<const u64*>(arenaF) + (uint64_t)rowsF[shard] * kRowWords : nullptr;
    const uint32_t* ra = rowsA + (uint64_t)shard * nA + a0;
    const uint32_t* rb = arenaB ? rowsB + (uint64_t)shard * nB : nullptr;
    for (uint32_t w = w0; w < w0 + kMdistWords; ++w) {
      u64 valid = ex[w];  // (wave-uniform)
      if (fl) valid &= fl[w];
      if (valid == 0) continue;
      // lane p holds plane p's word; transposed, lane c holds the magnitude of column c
      const u64 pw = (uint32_t)lane < depth ? ex[(uint64_t)(2 + lane) * kRowWords + w] : 0ull;
      const u64 mag = wave_transpose64(pw, tc);
      const bool neg = (ex[kRowWords + w] >> lane) & 1;
      const long long v = (long long)(neg ? 0ull - mag : mag);
      uint32_t rank = UINT32_MAX;
      if ((valid >> lane) & 1) {
        // the last fence <= v (fence[0] = U[0] <= v), then the last value <= v among the stride values it starts
        uint32_t lo = 0, hi = nf;
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (fence[mid] <= v) lo = mid;
          else hi = mid;
        }
        uint32_t b = lo * stride, e = min(b + stride, m);
        while (e - b > 1) {
          const uint32_t mid = (b + e) >> 1;
          if (U[mid] <= v) b = mid;
          else e = mid;
        }
        if ((stride == 1 ? fence[lo] : U[b]) == v && b >= r0 && b - r0 < tr) rank = b - r0;
      }
      const bool on = rank != UINT32_MAX;
      if (__ballot(on) == 0) continue;
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
            const uint32_t k = (uint32_t)__builtin_ctzll(am);
            am &= am - 1;
            atomicOr(reinterpret_cast<unsigned long long*>(P) + ((uint64_t)(wa * 64 + k) * wb + wj) * tr + rank, (unsigned long long)bm);
          }
        }
      }
    }
  }
}

// out[(a0 + i) * nB + j] += the ranks of the tile present for (i, j).  splits parts of the tile's tr / 64 rank words per (i, w).
__global__ void __launch_bounds__(256) k_mdist_popcount(const u64* __restrict__ P, uint32_t ta, uint32_t nB, uint32_t tr, uint32_t a0,
                                                        uint32_t splits, u64* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t wb = (nB + 63) / 64;
  const uint32_t pair = wave / splits, part = wave % splits;
  if (pair >= ta * wb) return;  // (wave-uniform)
  const uint32_t i = pair / wb, wj = pair % wb;
  const uint32_t n64 = tr / 64, per = (n64 + splits - 1) / splits;
  const uint32_t c0 = min(n64, part * per), c1 = min(n64, c0 + per);
  const u64* p = P + ((uint64_t)i * wb + wj) * tr;
  const TrConst tc = tr_const(lane);
  uint32_t cnt = 0;
  for (uint32_t c = c0; c < c1; ++c) cnt += (uint32_t)__popcll(wave_transpose64(p[(uint64_t)c * 64 + lane], tc));
  const uint32_t j = wj * 64 + (uint32_t)lane;
  if (cnt && j < nB) atomicAdd(reinterpret_cast<unsigned long long*>(out) + (uint64_t)(a0 + i) * nB + j, (unsigned long long)cnt);
}

}  // namespace fbk
