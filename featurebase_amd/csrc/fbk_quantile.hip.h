// fbk_quantile.hip.h — the values at several ranks of an int field over exists ∩ filter in ONE radix select (fbk_bsi_quantiles), and
// Percentile(field=, nth=, filter=) (executePercentile, executor.go:1310-1601) replayed from four such values (fbk_bsi_percentile).
//
// The select is fbk_sort.hip.h's (sort_walk_unit, SortKey, 11 bits per pass, most significant digit first) with SEVERAL prefixes
// alive at once: after a pass every rank asked for sits in one bin, so the next pass has at most n_ranks distinct prefixes, and
// ranks that share a prefix share a histogram.  Ascending keys, stored zeros kept (sk.desc = 0, sk.keep_zero = 1).
//   k_quant_hist      one launch serves up to kQuantPrefixes prefixes, passed by value in ascending order (wave-uniform scalars).  A
//                     column matches by comparing key >> (shift + 11) with them; the match's histogram [prefix][2048] lives in LDS
//                     (n_pre * 8 KiB, dynamic: a launch for few prefixes keeps its occupancy).  A word whose active columns all
//                     fall into one (prefix, bin) costs one LDS add, as in k_sort_hist.  Every block STORES its n_pre * 2048
//                     counts: no global atomics per column.
//   k_quant_hist_sum  adds the blocks' counts per bin: sums of counts, independent of the grid, the chunking and the block order.
// The host reads n_pre * 2048 counts per launch, picks for every rank the bin that holds it and carries rank and prefix forward
// (fbk_quantile_api.inc).  More than kQuantPrefixes live prefixes take ceil(prefixes / kQuantPrefixes) walks of that pass.
#pragma once
#include "fbk_sort.hip.h"

namespace fbk {

constexpr uint32_t kQuantHistBlocks = 1024;  // most blocks of a launch: the partials stay within 1024 * 64 KiB = 2^26 bytes

// part[block][j][d] = the columns of exists ∩ filter this block walked whose key has prefix pre.p[j] above bit shift + 11 and digit
// d at bit `shift`.  n_pre == 0: no prefix yet (pass 0), one histogram of every column.  shift + 11 < 64 whenever n_pre != 0.
__global__ void __launch_bounds__(256) k_quant_hist(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                                   const uint32_t* __restrict__ rowsF, uint32_t ns, uint32_t depth, SortKey sk, uint32_t shift, QuantPrefixes pre,
                                                   uint32_t n_pre, uint32_t* __restrict__ part) {
  extern __shared__ uint32_t qh[];
  const uint32_t n_hist = n_pre ? n_pre : 1, n_bins = n_hist * kSortBins;
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t i = threadIdx.x; i < n_bins; i += 256) qh[i] = 0;
  __syncthreads();
  const TrConst tc = tr_const(lane);
  const uint32_t pshift = n_pre ? shift + kSortDigitBits : 0;
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    sort_walk_unit(arenaS, rowsS, arenaF, rowsF, ls, un, depth, sk, lane, tc, [&](uint32_t, u64 key, bool part_of) {
      uint32_t j = 0;
      bool hit = part_of;
      if (n_pre) {
        const u64 kp = key >> pshift;
        j = kQuantPrefixes;
#pragma unroll
        for (uint32_t q = 0; q < kQuantPrefixes; ++q)
          if (q < n_pre && kp == pre.p[q]) j = q;
        hit = part_of && j < kQuantPrefixes;
      }
      const uint32_t slot = j * kSortBins + ((uint32_t)(key >> shift) & (kSortBins - 1));
      const u64 act = __ballot(hit);
      if (act == 0) return;
      const uint32_t first = (uint32_t)__builtin_ctzll(act);
      const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, (int)first);
      if (__ballot(hit && slot == s0) == act) {
        if ((uint32_t)lane == first) atomicAdd(&qh[s0], (uint32_t)__popcll(act));
      } else if (hit) {
        atomicAdd(&qh[slot], 1u);  // (hit: j < n_pre, so slot < n_bins)
      }
    });
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_bins; i += 256) part[(uint64_t)blockIdx.x * n_bins + i] = qh[i];
}

// ghist[d] += the sum over the launch's n_blocks blocks of part[block][d], d < n_bins (a multiple of 256); grid (n_bins / 256,
// slices of the blocks): one atomic add of a partial SUM per bin and slice (they commute)
__global__ void __launch_bounds__(256) k_quant_hist_sum(const uint32_t* __restrict__ part, uint32_t n_blocks, uint32_t n_bins, u64* __restrict__ ghist) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d >= n_bins) return;
  u64 s = 0;
  for (uint32_t b = blockIdx.y; b < n_blocks; b += gridDim.y) s += part[(uint64_t)b * n_bins + d];
  if (s) atomicAdd(reinterpret_cast<unsigned long long*>(ghist) + d, (unsigned long long)s);
}

}  // namespace fbk
