// fbk_sort.hip.h — Sort(filter, field=, sort-desc=, limit=, offset=) by an int field (executor.go:9321-9385) as a SELECTION: with
// K = offset + limit far below the columns of exists ∩ filter only the K smallest keys matter.  The reference builds a Go map
// column -> value per shard (one Intersect and a map update per set bit of every plane, fragment.go:2907-2969), sorts every shard
// and merges whole shard results pairwise before it cuts; here the planes are streamed a few times and K candidates are sorted.
//
// Key of a column (order preserving, unsigned): value = sign ? -magnitude : magnitude (int64 wrap-around, as k_extract_bsi);
//   bit_depth <= 62: key = value + 2^bit_depth, bit_depth + 1 bits;  63, 64: key = value ^ 2^63, 64 bits;
//   descending: the key's bits complemented, so "smallest key first" is the order in both directions and ties stay in ascending
//   column order.  SortKey carries the three constants; sort_value() is the inverse (all in the HIP-free fbk_select_plan.h).
// Operands are DENSE rows (k_densify_rows, a chunk of shards at a time: fbk_sort_api.inc).  One wavefront per 1024-column unit as
// k_extract_bsi: lane p loads plane p's line, per 64-column word one in-register transpose gives lane c the magnitude of column c.
//   k_sort_hist     radix select, most significant digit first, 11 bits per pass: the columns whose key matches the prefix chosen so
//                   far add to an LDS histogram of the next digit; every block STORES its 2048 counts (no global atomics: 8192
//                   blocks adding 2048 bins each would be 16 M contended atomics per pass against 90 us of plane reads) and
//   k_sort_hist_sum adds the blocks' counts per bin (sums of counts: independent of the grid and of the order of the blocks).  The
//                   host reads 2048 counts per pass, picks the digit that holds rank K and carries the rank forward.  Pass 0 also
//                   gives the total.
//   k_sort_count    per unit: the columns with key < T and with key == T (T = the K-th smallest key)
//   (hipcub scan)   exclusive prefixes of both over all units: the rank of every candidate is ARITHMETIC, as Extract's
//   k_sort_collect  key and column id of the n_less columns below T at their rank in ascending column order, and of the first
//                   r = K - n_less columns with key == T (ascending column id, across shards) behind them.  A unit without a
//                   candidate costs four dwords.  No cursor, no atomics: every slot has one writer.
//   (hipcub sort)   stable radix sort of the n_less pairs by key; the ties are already in their final place
//   k_sort_emit     ranks [offset, K): column ids and values
// fbk_extract_open_columns: k_extract_scatter ORs the bits of a column list into a handle's sel words (atomic OR of distinct
// bits: commutes), k_extract_scan counts them, k_extract_upre adds the shards' bases.
#pragma once
#include "fbk_extract.hip.h"
#include "fbk_select_plan.h"

namespace fbk {

constexpr uint32_t kSortHistBlocks = 1024;  // most blocks of a k_sort_hist launch (each stores kSortBins counts)

__device__ __forceinline__ u64 sort_readlane(u64 x, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, (int)l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)l);
  return ((u64)hi << 32) | lo;
}

// The unit `un` of launch-local shard ls: fn(k, key, part) for every word k that holds a column of exists ∩ filter; part = this
// lane's column takes part (in exists ∩ filter, and magnitude != 0 unless keep_zero).  Every lane of the wave calls fn.
// Returns false (nothing loaded but the exists / filter lines) when the unit holds no such column.
template <class Fn>
__device__ __forceinline__ bool sort_walk_unit(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                               const uint32_t* __restrict__ rowsF, uint32_t ls, uint32_t un, uint32_t depth, const SortKey& sk, int lane,
                                               const TrConst& tc, Fn&& fn) {
  const u64* ex = reinterpret_cast<const u64*>(arenaS) + (uint64_t)rowsS[ls] * kExtractRowWords + (uint64_t)un * kExtractWords;
  u64 mine = 0, sgn = 0;
  if (lane < (int)kExtractWords) {
    mine = ex[lane];
    sgn = ex[kExtractRowWords + lane];
    if (arenaF) mine &= (reinterpret_cast<const u64*>(arenaF) + (uint64_t)rowsF[ls] * kExtractRowWords + (uint64_t)un * kExtractWords)[lane];
  }
  if (__ballot(mine != 0) == 0) return false;  // (wave-uniform)
  u64 pw[kExtractWords];
  extract_load_line(ex + (uint64_t)(2 + lane) * kExtractRowWords, (uint32_t)lane < depth, pw);
#pragma unroll
  for (uint32_t k = 0; k < kExtractWords; ++k) {
    const u64 m = sort_readlane(mine, k);
    if (m == 0) continue;
    const u64 sg = sort_readlane(sgn, k);
    const u64 mag = wave_transpose64(pw[k], tc);
    const bool neg = (sg >> lane) & 1;
    const bool part = ((m >> lane) & 1) && (sk.keep_zero || mag != 0);
    fn(k, sort_key(neg ? 0ull - mag : mag, sk), part);
  }
  return true;
}

// part[block][d] = the participating columns this block walked whose key has `prefix` above bit shift + 11 (every one if
// !has_prefix) and digit d at bit `shift`
__global__ void __launch_bounds__(256) k_sort_hist(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                                  const uint32_t* __restrict__ rowsF, uint32_t ns, uint32_t depth, SortKey sk, uint32_t shift, u64 prefix,
                                                  uint32_t has_prefix, uint32_t* __restrict__ part) {
  __shared__ uint32_t h[kSortBins];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t i = threadIdx.x; i < kSortBins; i += 256) h[i] = 0;
  __syncthreads();
  const TrConst tc = tr_const(lane);
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    sort_walk_unit(arenaS, rowsS, arenaF, rowsF, ls, un, depth, sk, lane, tc, [&](uint32_t, u64 key, bool part) {
      const bool hit = part && (!has_prefix || (key >> (shift + kSortDigitBits)) == prefix);
      const uint32_t bin = (uint32_t)(key >> shift) & (kSortBins - 1);
      const u64 act = __ballot(hit);
      if (act == 0) return;
      // a word whose columns all fall into one bin (few distinct values, all equal): one LDS add instead of 64 on one address
      const uint32_t first = (uint32_t)__builtin_ctzll(act);
      const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)first);
      if (__ballot(hit && bin == b0) == act) {
        if ((uint32_t)lane == first) atomicAdd(&h[b0], (uint32_t)__popcll(act));
      } else if (hit) {
        atomicAdd(&h[bin], 1u);
      }
    });
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kSortBins; i += 256) part[(uint64_t)blockIdx.x * kSortBins + i] = h[i];
}

// ghist[d] += the sum over the launch's n_blocks blocks of part[block][d]; grid (kSortBins / 256, slices of the blocks): one atomic
// add of a partial SUM per bin and slice (64 K adds of counts per pass: they commute)
__global__ void __launch_bounds__(256) k_sort_hist_sum(const uint32_t* __restrict__ part, uint32_t n_blocks, u64* __restrict__ ghist) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  u64 s = 0;
  for (uint32_t b = blockIdx.y; b < n_blocks; b += gridDim.y) s += part[(uint64_t)b * kSortBins + d];
  if (s) atomicAdd(reinterpret_cast<unsigned long long*>(ghist) + d, (unsigned long long)s);
}

// n_lt[abs unit] / n_eq[abs unit] = the participating columns of the unit with key < T / key == T (take_all: every one / none).
// abs unit = (abs0 + ls) * 1024 + un; every unit of the launch is written.
__global__ void __launch_bounds__(256) k_sort_count(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                                   const uint32_t* __restrict__ rowsF, uint32_t ns, uint32_t abs0, uint32_t depth, SortKey sk, u64 T,
                                                   uint32_t take_all, u64* __restrict__ n_lt, u64* __restrict__ n_eq) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TrConst tc = tr_const(lane);
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    uint32_t cl = 0, ce = 0;
    sort_walk_unit(arenaS, rowsS, arenaF, rowsF, ls, un, depth, sk, lane, tc, [&](uint32_t, u64 key, bool part) {
      cl += (uint32_t)__popcll(__ballot(part && (take_all || key < T)));
      ce += (uint32_t)__popcll(__ballot(part && !take_all && key == T));
    });
    const uint64_t au = (uint64_t)(abs0 + ls) * kExtractUnits + un;
    if (lane == 0) n_lt[au] = cl;
    if (lane == 1) n_eq[au] = ce;
  }
}

// keys / cols [K]: slots [0, n_less) the columns with key < T at their rank (ascending column id), slots [n_less, n_less + r) the
// first r columns with key == T.  p_lt / p_eq [all units + 1]: the exclusive prefixes of k_sort_count's counts.
__global__ void __launch_bounds__(256) k_sort_collect(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                                     const uint32_t* __restrict__ rowsF, uint32_t ns, uint32_t abs0, uint32_t depth, SortKey sk, u64 T,
                                                     uint32_t take_all, const u64* __restrict__ p_lt, const u64* __restrict__ p_eq,
                                                     const u64* __restrict__ shard_ids, u64 n_less, u64 r, u64* __restrict__ keys, u64* __restrict__ cols) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TrConst tc = tr_const(lane);
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    const uint64_t au = (uint64_t)(abs0 + ls) * kExtractUnits + un;
    u64 lp = p_lt[au], ep = p_eq[au];
    if (p_lt[au + 1] == lp && (ep >= r || p_eq[au + 1] == ep)) continue;  // (wave-uniform) no candidate in these 1024
    const u64 col0 = (shard_ids[abs0 + ls] << 20) + (u64)un * (kExtractWords * 64);
    sort_walk_unit(arenaS, rowsS, arenaF, rowsF, ls, un, depth, sk, lane, tc, [&](uint32_t k, u64 key, bool part) {
      const bool lt = part && (take_all || key < T), eq = part && !take_all && key == T;
      const u64 ml = __ballot(lt), me = __ballot(eq);
      const u64 col = col0 + k * 64 + (uint32_t)lane;
      if (lt) {
        const u64 at = lp + extract_below(ml);
        if (at < n_less) keys[at] = key, cols[at] = col;
      }
      if (eq) {
        const u64 e = ep + extract_below(me);
        if (e < r) keys[n_less + e] = key, cols[n_less + e] = col;
      }
      lp += (uint32_t)__popcll(ml);
      ep += (uint32_t)__popcll(me);
    });
  }
}

// records [off, off + n) of the result: ranks below n_less from the sorted pairs, the ties from the collected ones
__global__ void __launch_bounds__(256) k_sort_emit(const u64* __restrict__ skeys, const u64* __restrict__ scols, const u64* __restrict__ keys,
                                                  const u64* __restrict__ cols, u64 n_less, u64 off, u64 n, SortKey sk, u64* __restrict__ out_cols,
                                                  long long* __restrict__ out_vals) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 j = off + i;
  const bool s = j < n_less;
  out_cols[i] = s ? scols[j] : cols[j];
  out_vals[i] = sort_value(s ? skeys[j] : keys[j], sk);
}

// sel[bit >> 6] |= 1 << (bit & 63) for the n bit positions (shard of the span * 2^20 + position); sel is zeroed before
__global__ void __launch_bounds__(256) k_extract_scatter(const u64* __restrict__ bitpos, u64 n, u64 n_words, u64* __restrict__ sel) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 p = bitpos[i];
  if ((p >> 6) < n_words) atomicOr(reinterpret_cast<unsigned long long*>(sel) + (p >> 6), 1ull << (p & 63));
}

// upre[s * 1024 + u] = shard_base[s] + unit_pre[s * 1024 + u]; upre[n_units] = n
__global__ void __launch_bounds__(256) k_extract_upre(const uint32_t* __restrict__ unit_pre, const u64* __restrict__ shard_base, u64 n_units, u64 n,
                                                     uint32_t* __restrict__ upre) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i < n_units) upre[i] = (uint32_t)(shard_base[i / kExtractUnits] + unit_pre[i]);
  if (i == n_units) upre[i] = (uint32_t)n;
}

}  // namespace fbk
