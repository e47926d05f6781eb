// fbk_group_select.hip.h — the GroupBy selection stage (having / sort / offset / limit) over totals that are on the device:
// counts[n] (u64) and, where the call has an aggregate, aggs[n] (int64 bits), n <= 2^24 cells.  Host side: fbk_group_select_api.inc;
// the rules (predicate, keys) are fbk_group_select_plan.h's, the same functions the host path runs.
//
// Everything is an ORDERED COMPACTION of a list of items — the cells 0 .. n-1 (list == nullptr), or a list of cells that an earlier
// compaction wrote — in units of 512 items, one wave each:
//   k_gs_count    per unit, the items of class A and of class B (a 64-lane __ballot per 64 items, popcount);
//   (host)        ONE exclusive scan over {A counts, 0, B counts, 0} (hipcub::DeviceScan) gives every unit's first rank and both totals;
//   k_gs_emit     the same ballots again: an item's rank is its unit's first rank + the popcounts of the ballots before it + the
//                 popcount of its ballot below its lane, and the item writes its CELL at that rank.  Nothing but cells is written:
//                 counts, aggregates and keys are re-read through them.
// The classes:  kGsMatched  A = the groups (count > 0 and having), no B; only the ranks [lo, end) are written (without a sort that is
//                           offset / limit: nothing else leaves the pass);
//               kGsBelow    A = key < T, B = key == T for the composite key T of rank K that the radix select found (state):
//                           A goes to ranks [0, n_less), the first `want` items of B in list order behind them.
// The radix select (k_gs_hist + k_gs_pick) walks the composite key {term 0, term 1} MSB first, 8 bits per pass; the digit is chosen
// ON THE DEVICE (k_gs_pick, one thread's walk over 256 bins), so the 8 or 16 passes need no round trip to the host.
// Results do not depend on the grid or on the order in which blocks run: histogram bins are integer sums, ranks come from popcounts.
#pragma once

#include "fbk_group_select_plan.h"
#include "fbk_kernels.hip.h"

namespace fbk {

constexpr uint32_t kGsUnit = 512;           // items per wave
constexpr uint32_t kGsBlock = 4 * kGsUnit;  // items per block of 256 threads
constexpr uint32_t kGsBins = 256;           // one radix-select digit: 8 bits
constexpr uint32_t kGsHistBlocks = 1024;    // k_gs_hist: at most this many blocks, striding over the list

enum GsMode : uint32_t { kGsMatched = 0, kGsBelow = 1 };

// the radix select's state, in device memory between its passes
struct GsState {
  u64 t[2];    // the digits of T chosen so far (term 0, term 1)
  u64 want;    // the rank looked for among the keys that share T's prefix; at the end: the ties to take
  u64 n_less;  // keys below T's prefix; at the end: keys below T
};

using GsRules = fbk_group_select::Rules;

__device__ __forceinline__ u64 gs_bits(const long long* __restrict__ aggs, uint32_t cell) { return aggs ? u64(aggs[cell]) : 0; }

// the class of item i: bit 0 = A, bit 1 = B
template <GsMode MODE>
__device__ __forceinline__ uint32_t gs_class(const u64* __restrict__ counts, const long long* __restrict__ aggs, uint32_t cell, const GsRules& r, u64 t0, u64 t1) {
  const u64 c = counts[cell], a = gs_bits(aggs, cell);
  if (MODE == kGsMatched) return fbk_group_select::passes(r, c, a) ? 1u : 0u;
  const u64 k0 = fbk_group_select::key(r, 0, c, a), k1 = r.n_sort > 1 ? fbk_group_select::key(r, 1, c, a) : 0;
  if (k0 < t0 || (k0 == t0 && k1 < t1)) return 1u;
  return k0 == t0 && k1 == t1 ? 2u : 0u;
}

// unit u (one wave) counts its 512 items: cnt[u] = class A, cnt[n_units + 1 + u] = class B (kGsBelow only)
template <GsMode MODE>
__global__ void __launch_bounds__(256) k_gs_count(const u64* __restrict__ counts, const long long* __restrict__ aggs, const uint32_t* __restrict__ list, uint32_t n,
                                                  GsRules r, const GsState* __restrict__ state, uint32_t n_units, uint32_t* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_units) return;  // (a whole wave leaves: no ballot is split)
  u64 t0 = 0, t1 = 0;
  if (MODE == kGsBelow) t0 = state->t[0], t1 = state->t[1];
  uint32_t na = 0, nb = 0;
  for (uint32_t k = 0; k < kGsUnit / 64; ++k) {
    const uint32_t i = u * kGsUnit + k * 64 + lane;
    const uint32_t cls = i < n ? gs_class<MODE>(counts, aggs, list ? list[i] : i, r, t0, t1) : 0u;
    na += uint32_t(__popcll(__ballot(cls & 1u)));
    if (MODE == kGsBelow) nb += uint32_t(__popcll(__ballot(cls & 2u)));
  }
  if (lane == 0) {
    cnt[u] = na;
    if (MODE == kGsBelow) cnt[n_units + 1 + u] = nb;
  }
}

// pre = the exclusive scan of cnt.  kGsMatched: the items of class A with ranks in [lo, end) write their cell to out[rank - lo].
// kGsBelow: class A to out[rank], class B with a rank below state->want to out[state->n_less + rank].  Every store is checked against cap.
template <GsMode MODE>
__global__ void __launch_bounds__(256) k_gs_emit(const u64* __restrict__ counts, const long long* __restrict__ aggs, const uint32_t* __restrict__ list, uint32_t n,
                                                 GsRules r, const GsState* __restrict__ state, uint32_t n_units, const uint32_t* __restrict__ pre, uint32_t lo,
                                                 uint32_t end, uint32_t cap, uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_units) return;
  u64 t0 = 0, t1 = 0, take_b = 0, base_b = 0;
  uint32_t ra = pre[u], rb = 0;
  if (MODE == kGsBelow) {
    t0 = state->t[0], t1 = state->t[1], take_b = state->want, base_b = state->n_less;
    rb = pre[n_units + 1 + u] - pre[n_units];  // (pre[n_units] = all of class A: the scan runs on over the B counts)
  }
  if (MODE == kGsMatched && (ra >= end || pre[u + 1] <= lo)) return;  // nothing of this unit is inside the window
  const u64 below = (1ull << lane) - 1;
  for (uint32_t k = 0; k < kGsUnit / 64; ++k) {
    const uint32_t i = u * kGsUnit + k * 64 + lane;
    const uint32_t cell = i < n ? (list ? list[i] : i) : 0u;
    const uint32_t cls = i < n ? gs_class<MODE>(counts, aggs, cell, r, t0, t1) : 0u;
    const u64 ma = __ballot(cls & 1u);
    if (cls & 1u) {
      const uint32_t rank = ra + uint32_t(__popcll(ma & below));
      if (rank >= lo && rank < end && rank - lo < cap) out[rank - lo] = cell;
    }
    ra += uint32_t(__popcll(ma));
    if (MODE == kGsBelow) {
      const u64 mb = __ballot(cls & 2u);
      if (cls & 2u) {
        const u64 rank = u64(rb) + u64(__popcll(mb & below));
        if (rank < take_b && base_b + rank < cap) out[base_b + rank] = cell;
      }
      rb += uint32_t(__popcll(mb));
    }
  }
}

// One pass of the radix select over the m cells of `list`: hist[digit] += the keys that share T's prefix above (word, shift), by
// their 8 bits at shift of term `word`.
__global__ void __launch_bounds__(256) k_gs_hist(const u64* __restrict__ counts, const long long* __restrict__ aggs, const uint32_t* __restrict__ list, uint32_t m,
                                                 GsRules r, const GsState* __restrict__ state, uint32_t word, uint32_t shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kGsBins];
  h[threadIdx.x] = 0;
  __syncthreads();
  const u64 t0 = state->t[0], t1 = state->t[1];
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < m; i += uint64_t(gridDim.x) * 256) {
    const uint32_t cell = list[i];
    const u64 c = counts[cell], a = gs_bits(aggs, cell);
    const u64 k0 = fbk_group_select::key(r, 0, c, a);
    bool in;
    u64 kw;
    if (word == 0) {
      kw = k0, in = (((k0 ^ t0) >> shift) >> 8) == 0;
    } else {
      kw = fbk_group_select::key(r, 1, c, a), in = k0 == t0 && (((kw ^ t1) >> shift) >> 8) == 0;
    }
    if (in) atomicAdd(&h[uint32_t(kw >> shift) & (kGsBins - 1)], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// The digit of T at (word, shift): the bin in which the cumulative count reaches state->want.  One block; clears hist for the next pass.
__global__ void __launch_bounds__(256) k_gs_pick(uint32_t* __restrict__ hist, GsState* __restrict__ state, uint32_t word, uint32_t shift) {
  __shared__ uint32_t h[kGsBins];
  h[threadIdx.x] = hist[threadIdx.x];
  __syncthreads();
  hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    const u64 want = state->want;
    u64 before = 0;
    uint32_t b = 0;
    while (b + 1 < kGsBins && before + h[b] < want) before += h[b++];
    state->n_less += before;
    state->want = want - before;
    state->t[word] |= u64(b) << shift;
  }
}

// keys[i] = the order-preserving key of sort term `term` of cell list[i]
__global__ void __launch_bounds__(256) k_gs_keys(const u64* __restrict__ counts, const long long* __restrict__ aggs, const uint32_t* __restrict__ list, uint32_t m,
                                                 GsRules r, uint32_t term, u64* __restrict__ keys) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t cell = list[i];
  keys[i] = fbk_group_select::key(r, term, counts[cell], gs_bits(aggs, cell));
}

// the records of the result: cell, count and aggregate of list[0 .. m)
__global__ void __launch_bounds__(256) k_gs_records(const u64* __restrict__ counts, const long long* __restrict__ aggs, const uint32_t* __restrict__ list, uint32_t m,
                                                    u64* __restrict__ out_counts, long long* __restrict__ out_aggs) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t cell = list[i];
  out_counts[i] = counts[cell];
  if (aggs) out_aggs[i] = aggs[cell];
}

}  // namespace fbk
