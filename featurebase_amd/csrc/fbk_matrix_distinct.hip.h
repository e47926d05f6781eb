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
//   k_mdist_scatter   group_column_walk (fbk_group_walk.hip.h): a lane's column gets its value from the walk's magnitude and the
//                     sign, and by a binary search in U its rank (the search tree's top, kMdistFences values of U, staged in
//                     LDS; the rest in U itself); a word none of whose columns has a value in the tile is left there.  Per A row
//                     the lane holds, one atomicOr of its B mask into P.  Atomics: Σ_c |A(c)| x ceil(n_b / 64) over the columns
//                     with a value in the tile.
//   k_mdist_popcount  one wavefront per (A row, B word, part of the ranks): 64 ranks' words at a time, transposed so that lane
//                     b holds the 64 ranks' bits of B row 64 w + b, popcounts added to the result.
#pragma once
#include "fbk_group_walk.hip.h"

namespace fbk {

constexpr uint32_t kMdistFences = 4096;  // values of U staged in LDS per block (32 KiB): every stride-th one

// P: [ta][ceil(nB / 64)][tr] u64, zeroed by the caller; tr a multiple of 64.  U: the m sorted distinct values (m >= 1).
__global__ void __launch_bounds__(256) k_mdist_scatter(FBK_GROUP_PARAMS, uint32_t a0, uint32_t ta, const long long* __restrict__ U, uint32_t m,
                                                       uint32_t r0, uint32_t tr, u64* __restrict__ P) {
  __shared__ long long fence[kMdistFences];
  const uint32_t stride = (m + kMdistFences - 1) / kMdistFences, nf = (m + stride - 1) / stride;
  for (uint32_t t = threadIdx.x; t < nf; t += 256) fence[t] = U[(uint64_t)t * stride];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t wb = (nB + 63) / 64;
  uint32_t rank = UINT32_MAX;  // of the lane's column in the tile; UINT32_MAX: its value is not in the tile
  group_column_walk<true>(
      FBK_GROUP_ARGS, a0, ta,
      [&](const u64* exw, bool valid, u64 mag) {
        const bool neg = (exw[kGroupRowWords] >> lane) & 1;
        const long long v = (long long)(neg ? 0ull - mag : mag);
        rank = UINT32_MAX;
        if (valid) {
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
        return rank != UINT32_MAX;
      },
      [&](uint32_t a_row, uint32_t wj, u64 bm) {
        atomicOr(reinterpret_cast<unsigned long long*>(P) + ((uint64_t)a_row * wb + wj) * tr + rank, (unsigned long long)bm);
      });
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
