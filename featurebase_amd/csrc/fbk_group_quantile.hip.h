// fbk_group_quantile.hip.h — GroupBy with a percentile of an int field per group (SQL SELECT a, b, PERCENTILE_DISC(x, p) ... GROUP BY
// a, b) for all (A row, B row) groups at once, for DENSE operands: ONE radix select (fbk_quantile.hip.h's, most significant digit
// first, on fbk_sort.hip.h's key: ascending, stored zeros take part) whose histograms are kept PER GROUP, on group_column_walk
// (fbk_group_walk.hip.h).
//
//   k_gquant_hist_global / _lds   the walk's magnitude and the sign give the lane its column's key; every column of exists & F takes
//                     part.  For every (i, j) of its masks and every request q of that group the lane compares the key's bits
//                     above the current digit with slot[group][q].prefix and, where they are equal, adds 1 to
//                     hist[group][q][digit].  Pass 0 has no prefix and ONE histogram per group, shared by its requests; its sum
//                     is the group's N.  A group without a column and a request that is done carry a prefix no key has.  Every
//                     pass reads each plane once whatever the number of groups.
//        GLOBAL       64-bit counters in device memory, atomicAdd (global_atomic_add_x2, no return): for many groups, where the
//                     adds spread over many lines.
//        LDS          32-bit counters of ALL the call's (group, request) pairs in the block's LDS (at most 64 KiB, dynamic); every
//                     block STORES its counts and k_quant_hist_sum adds them per bin: for few groups, where global atomics would
//                     all land on a few hundred addresses.
//   k_gquant_resolve  one wavefront per (group, request) between the passes, on the device: lanes sum bins / 64 consecutive bins each,
//                     a wave scan finds the lane and then the bin that holds the remaining rank; the digit is appended to the
//                     prefix and the counts below it leave the rank.  After pass 0 it first takes N and turns num / den into the rank
//                     (fbk_group_quantile_plan.h: disc_rank).  After the last pass the bin's count is the request's count and the
//                     completed key, converted back, its value.
// Every count is a sum of integer adds: the result does not depend on the grid, the chunking or the order of the blocks.
#pragma once
#include "fbk_group_quantile_plan.h"
#include "fbk_group_walk.hip.h"
#include "fbk_quantile.hip.h"

namespace fbk {

constexpr u64 kGquantNoPrefix = ~0ull;  // no key >> (1 or more) equals it: an empty group's requests

struct GquantSlot {  // a request of a group on its way down the digits
  u64 prefix;        // the key's digits so far
  u64 rank;          // its rank among the group's columns with that prefix
};

__device__ __forceinline__ void gquant_add(u64* p) { atomicAdd(reinterpret_cast<unsigned long long*>(p), 1ull); }
__device__ __forceinline__ void gquant_add(uint32_t* p) { atomicAdd(p, 1u); }

// n_h == 0: pass 0, hist[group][bins]; else hist[group][n_h][bins] and slots[group][n_h].  Counter: u64 (device memory) or uint32_t
// (LDS).
template <class Counter>
__device__ __forceinline__ void gquant_walk(FBK_GROUP_PARAMS, uint32_t shift, uint32_t wbits, uint32_t dbits, uint32_t n_h,
                                            const GquantSlot* __restrict__ slots, Counter* hist) {
  const SortKey sk = select_key(depth, false, true);  // as fbk_bsi_quantiles'; built here, where its constant fields cost no scalar registers
  const int lane = threadIdx.x & 63;
  const uint32_t bins = 1u << dbits, pshift = n_h ? shift + wbits : 0;  // (n_h != 0: shift + wbits < 64); the digit: wbits <= dbits bits
  uint32_t digit = 0;  // of the lane's column's key
  u64 kp = 0;          // the key's bits above the digit
  group_column_walk<false>(
      FBK_GROUP_ARGS, 0, nA,
      [&](const u64* exw, bool valid, u64 mag) {
        const bool neg = depth && ((exw[kGroupRowWords] >> lane) & 1);  // (depth == 0 reads neither plane nor sign)
        const u64 key = sort_key(neg ? 0ull - mag : mag, sk);
        digit = (uint32_t)(key >> shift) & ((1u << wbits) - 1);
        kp = key >> pshift;
        return valid;
      },
      [&](uint32_t a_row, uint32_t wj, u64 bm) {
        for (u64 b = bm; b; b &= b - 1) {
          const uint64_t cell = (uint64_t)a_row * nB + wj * 64 + (uint32_t)__builtin_ctzll(b);  // < nA * nB: the masks' bits are rows
          if (n_h == 0) {
            gquant_add(hist + cell * bins + digit);
          } else {
            for (uint32_t q = 0; q < n_h; ++q)
              if (slots[cell * n_h + q].prefix == kp) gquant_add(hist + ((cell * n_h + q) << dbits) + digit);
          }
        }
      });
}

// hist: [nA * nB][max(1, n_h)][1 << dbits], zeroed by the caller
__global__ void __launch_bounds__(256) k_gquant_hist_global(FBK_GROUP_PARAMS, uint32_t shift, uint32_t wbits, uint32_t dbits, uint32_t n_h,
                                                            const GquantSlot* __restrict__ slots, u64* hist) {
  gquant_walk<u64>(FBK_GROUP_ARGS, shift, wbits, dbits, n_h, slots, hist);
}

// part: [gridDim.x][n_bins], n_bins = nA * nB * max(1, n_h) << dbits counters = the dynamic LDS of the launch (at most 64 KiB)
__global__ void __launch_bounds__(256) k_gquant_hist_lds(FBK_GROUP_PARAMS, uint32_t shift, uint32_t wbits, uint32_t dbits, uint32_t n_h,
                                                         const GquantSlot* __restrict__ slots, uint32_t n_bins, uint32_t* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint32_t gq[];
  for (uint32_t i = threadIdx.x; i < n_bins; i += 256) gq[i] = 0;
  __syncthreads();
  gquant_walk<uint32_t>(FBK_GROUP_ARGS, shift, wbits, dbits, n_h, slots, gq);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_bins; i += 256) part[(uint64_t)blockIdx.x * n_bins + i] = gq[i];
}

// One wavefront per pair = group * max(1, n_q) + q.  hist: the finished pass's (first: [cells][bins], else [pairs][bins]; its digit
// had wbits bits, the bins beyond are zero).  first:
// totals[group] = N, and the requests start (n_q == 0: the totals alone); last: out_values / out_counts [pairs].  q_num / q_den on
// the device.
__global__ void __launch_bounds__(256) k_gquant_resolve(const u64* __restrict__ hist, uint32_t cells, uint32_t n_q, uint32_t dbits, uint32_t wbits, int first, int last,
                                                        const uint32_t* __restrict__ q_num, const uint32_t* __restrict__ q_den, uint32_t depth,
                                                        GquantSlot* __restrict__ slots, u64* __restrict__ out_totals, long long* __restrict__ out_values,
                                                        u64* __restrict__ out_counts) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nq1 = n_q ? n_q : 1;
  const uint64_t pair = (uint64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (pair >= (uint64_t)cells * nq1) return;  // (wave-uniform)
  const uint32_t cell = uint32_t(pair / nq1), q = uint32_t(pair % nq1);
  const uint32_t per = (1u << dbits) >> 6;  // bins of a lane (dbits >= 8: 4 or more)
  const u64* h = hist + ((first ? (uint64_t)cell : pair) << dbits);
  u64 s = 0;
  for (uint32_t t = 0; t < per; ++t) s += h[lane * per + t];
  u64 incl = s;
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const u64 o = (u64)__shfl_up((unsigned long long)incl, off);
    if (lane >= off) incl += o;
  }
  u64 prefix = 0, rank;
  if (first) {
    const u64 total = (u64)__shfl((unsigned long long)incl, 63);
    if (q == 0 && lane == 0) out_totals[cell] = total;
    if (n_q == 0) return;
    if (total == 0) {
      if (lane == 0) slots[pair] = {kGquantNoPrefix, 0ull}, out_values[pair] = 0, out_counts[pair] = 0ull;
      return;
    }
    rank = fbk_gquant_plan::disc_rank(total, q_num[q], q_den[q]);
  } else {
    prefix = slots[pair].prefix, rank = slots[pair].rank;
    if (prefix == kGquantNoPrefix) return;  // an empty group: written after pass 0
  }
  // the rank is below the histogram's total (pass 0: below N; later: below the count of the bin it came from)
  const u64 holds = __ballot(incl > rank);
  if (holds == 0 || lane != (uint32_t)__builtin_ctzll(holds)) return;
  u64 before = incl - s;
  uint32_t b = lane * per;
  u64 c = h[b];
  while (before + c <= rank && b + 1 < (lane + 1) * per) before += c, c = h[++b];
  prefix = (prefix << wbits) | b, rank -= before;
  slots[pair] = {prefix, rank};
  if (last) out_values[pair] = sort_value(prefix, select_key(depth, false, true)), out_counts[pair] = c;
}

}  // namespace fbk
