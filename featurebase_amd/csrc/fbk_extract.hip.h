// fbk_extract.hip.h — Extract(filter, Rows(f1), Rows(f2), …) (executor.go:4711-5046): the records of a column filter, one field per
// call.  The reference rotates a bit matrix the slow way (filter.Columns(), a map from column to output slot, then one Intersect
// per bit plane / per row of a set field and a map lookup per set bit); here the rotation is the 64 x 64 in-register transpose of
// fbk_bsi_kernels.hip.h and the output slot of a column is ARITHMETIC: its rank among the selected columns = the prefix of its
// unit (16 words = 1024 columns, a 128-byte line of every row) + the selected columns of the unit's earlier words + those of the
// lanes below.  No atomics, no global cursor; every device write is a plain vector store.  Operands are DENSE rows (k_densify_rows
// makes them so, a chunk of shards at a time: fbk_extract_api.inc).
//
// fbk_extract_open (all shards, then the selected span only):
//   k_extract_scan      one block per shard: popcounts of the filter's 1024 units and their exclusive prefix inside the shard
//   (k_bsi_cell_scan)   exclusive prefix of the shards' totals: the host reads it, applies offset / limit, finds the span
//   k_extract_select    one wavefront per unit of the span: the filter's words with the columns of rank [lo, hi) only — the handle's
//                       resident `sel` — and the unit's rank prefix relative to lo
// per field (the span only; a unit without a selected column costs two dwords, a word without one nothing but its sel word):
//   k_extract_columns   column ids = shard id * 2^20 + position, at their rank
//   k_extract_bsi       lane p loads plane p's line, per word one transpose gives lane c the magnitude of column c; value and
//                       present byte of EVERY selected column are stored (0 / 0 outside exists): the outputs need no memset
//   k_extract_rows      <false> counts, <true> fills: per block of 64 field rows lane i loads row i's line, the transpose gives lane
//                       c its 64-row membership mask.  The lane that holds a column is the only writer of counts[rank] in the
//                       whole launch sequence, so launches over later row blocks just continue it: ascending items, no atomics
//   k_extract_tile_sums / (k_bsi_cell_scan) / k_extract_offsets   counts -> CSR offsets, tiles of 4096 columns
#pragma once
#include "fbk_bsi_kernels.hip.h"

namespace fbk {

constexpr uint32_t kExtractWords = 16;                                  // 64-column words per unit
constexpr uint32_t kExtractUnits = kSlots * 1024 / kExtractWords;       // units per shard (1024: k_extract_scan's block)
constexpr uint64_t kExtractRowWords = (uint64_t)kSlots * 1024;          // u64 words of a dense row
constexpr uint32_t kExtractTile = 4096;                                 // columns per block of the offsets scan

__device__ __forceinline__ uint32_t extract_below(u64 x) {  // set bits of x in the lanes below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(x >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)x, 0u));
}

__device__ __forceinline__ u64 extract_uniform(u64 x) {  // a wave-uniform word, and the compiler knows it (the transposes need every lane)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)x), hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return ((u64)hi << 32) | lo;
}

// exclusive prefix of v over the 1024 threads of a block; *total = the block's sum (every thread)
__device__ __forceinline__ uint32_t extract_block_scan(uint32_t v, uint32_t* wsum /* [16] shared */, uint32_t* total) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t x = (uint32_t)__shfl_up((int)incl, o, kWave);
    if (lane >= o) incl += x;
  }
  __syncthreads();  // (wsum may still be read from an earlier call)
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const uint32_t s = wsum[w];
    if (w < wv) before += s;
    all += s;
  }
  *total = all;
  return before + incl - v;
}

// unit_pre[shard * 1024 + u] = the filter's columns in the units before u of that shard; shard_tot[shard] = its columns.
// One block of 1024 threads per shard: sixteen coalesced passes over the row, the popcounts as bytes through the LDS.
__global__ void __launch_bounds__(1024) k_extract_scan(const uint8_t* __restrict__ arenaF, const uint32_t* __restrict__ rowsF,
                                                      uint32_t* __restrict__ unit_pre, uint32_t* __restrict__ shard_tot) {
  __shared__ uint32_t pc4[kSlots * 1024 / 4];
  __shared__ uint32_t wsum[16];
  const uint32_t t = threadIdx.x, shard = blockIdx.x;
  const u64* f = reinterpret_cast<const u64*>(arenaF) + (uint64_t)rowsF[shard] * kExtractRowWords;
  uint8_t* pc = reinterpret_cast<uint8_t*>(pc4);
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) pc[i * 1024 + t] = (uint8_t)__popcll(f[i * 1024 + t]);
  __syncthreads();
  const uint4 q = reinterpret_cast<const uint4*>(pc4)[t];  // the sixteen words of unit t
  auto bytes = [](uint32_t x) {
    const uint32_t s = (x & 0x00FF00FFu) + ((x >> 8) & 0x00FF00FFu);
    return (s & 0xFFFFu) + (s >> 16);
  };
  const uint32_t v = bytes(q.x) + bytes(q.y) + bytes(q.z) + bytes(q.w);
  uint32_t total;
  const uint32_t excl = extract_block_scan(v, wsum, &total);
  unit_pre[(uint64_t)shard * kExtractUnits + t] = excl;
  if (t == 0) shard_tot[shard] = total;
}

// The selected part of the filter.  Launch-local shard ls is shard abs0 + ls of the call and shard span0 + ls of the span.
// sel[su * 16 + k] = word k of span unit su with the columns of rank [lo, hi) only; upre[su] = the selected columns before the unit
// (= rank - lo of its first one); the unit su_end - 1 also writes upre[su_end] = hi - lo.
__global__ void __launch_bounds__(256) k_extract_select(const uint8_t* __restrict__ arenaF, const uint32_t* __restrict__ rowsF, uint32_t ns,
                                                       const uint32_t* __restrict__ unit_pre, const u64* __restrict__ shard_base, uint32_t abs0,
                                                       uint32_t span0, u64 lo, u64 hi, u64 su_end, u64* __restrict__ sel,
                                                       uint32_t* __restrict__ upre) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    const uint64_t su = (uint64_t)(span0 + ls) * kExtractUnits + un;
    u64 gp = shard_base[abs0 + ls] + unit_pre[(uint64_t)(abs0 + ls) * kExtractUnits + un];
    const u64* f = reinterpret_cast<const u64*>(arenaF) + (uint64_t)rowsF[ls] * kExtractRowWords + (uint64_t)un * kExtractWords;
    const u64 first = gp;
    u64 mine = 0;
#pragma unroll 1  // (unrolled, the sixteen words and their running ranks overflow the scalar file)
    for (uint32_t k = 0; k < kExtractWords; ++k) {
      const u64 x = extract_uniform(f[k]);
      const uint32_t n = (uint32_t)__popcll(x);
      u64 keep;
      if (gp >= lo && gp + n <= hi) keep = x;
      else if (gp + n <= lo || gp >= hi) keep = 0;
      else {
        const u64 ord = gp + extract_below(x);
        keep = __ballot(((x >> lane) & 1) != 0 && ord >= lo && ord < hi);
      }
      if ((uint32_t)lane == k) mine = keep;
      gp += n;
    }
    if (lane < (int)kExtractWords) sel[su * kExtractWords + lane] = mine;
    auto rel = [&](u64 g) { return (uint32_t)((g < lo ? lo : g > hi ? hi : g) - lo); };
    if (lane == 0) upre[su] = rel(first);
    if (lane == 1 && su + 1 == su_end) upre[su_end] = rel(gp);
  }
}

// out[rank] = shard id * 2^20 + position, for the n selected columns of the span's n_units units
__global__ void __launch_bounds__(256) k_extract_columns(const u64* __restrict__ sel, const uint32_t* __restrict__ upre,
                                                        const u64* __restrict__ shard_ids, u64 n_units, u64 n, u64* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < n_units; u += (uint64_t)gridDim.x * 4) {
    u64 r = upre[u];
    if (upre[u + 1] == r) continue;  // (wave-uniform) no selected column in these 1024
    const u64 col0 = (shard_ids[u / kExtractUnits] << 20) + (u % kExtractUnits) * (kExtractWords * 64);
    for (uint32_t k = 0; k < kExtractWords; ++k) {
      const u64 x = sel[u * kExtractWords + k];
      if (x == 0) continue;
      const u64 at = r + extract_below(x);
      if (((x >> lane) & 1) && at < n) out[at] = col0 + k * 64 + (uint32_t)lane;
      r += (uint32_t)__popcll(x);
    }
  }
}

// the line (16 words) of one row at a unit, or zeros: eight 16-byte loads per lane
__device__ __forceinline__ void extract_load_line(const u64* p, bool live, u64 (&w)[kExtractWords]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ulonglong2 v = make_ulonglong2(0, 0);
    if (live) v = reinterpret_cast<const ulonglong2*>(p)[i];
    w[2 * i] = v.x;
    w[2 * i + 1] = v.y;
  }
}

// Int field.  rowsS[ls] = the exists row of launch-local shard ls (+1 sign, +2+p plane p) = span shard s0 + ls.
// vals[rank] = present ? (sign ? -magnitude : magnitude) : 0, pres[rank] = present, for every selected column of the launch.
__global__ void __launch_bounds__(256) k_extract_bsi(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, uint32_t ns,
                                                    uint32_t s0, uint32_t depth, const u64* __restrict__ sel, const uint32_t* __restrict__ upre,
                                                    u64 n, long long* __restrict__ vals, uint8_t* __restrict__ pres) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TrConst tc = tr_const(lane);
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    const uint64_t su = (uint64_t)(s0 + ls) * kExtractUnits + un;
    u64 r = upre[su];
    if (upre[su + 1] == r) continue;  // (wave-uniform)
    const u64* ex = reinterpret_cast<const u64*>(arenaS) + (uint64_t)rowsS[ls] * kExtractRowWords + (uint64_t)un * kExtractWords;
    u64 pw[kExtractWords];
    extract_load_line(ex + (uint64_t)(2 + lane) * kExtractRowWords, (uint32_t)lane < depth, pw);
#pragma unroll
    for (uint32_t k = 0; k < kExtractWords; ++k) {
      const u64 x = extract_uniform(sel[su * kExtractWords + k]);
      if (x == 0) continue;
      const u64 mag = wave_transpose64(pw[k], tc);
      const u64 e = ex[k], sg = ex[kExtractRowWords + k];
      const u64 at = r + extract_below(x);
      if (((x >> lane) & 1) && at < n) {
        const bool present = (e >> lane) & 1, neg = (sg >> lane) & 1;
        vals[at] = present ? (long long)(neg ? 0ull - mag : mag) : 0ll;
        pres[at] = present ? 1 : 0;
      }
      r += (uint32_t)__popcll(x);
    }
  }
}

// Set field, rows [i0, i0 + nr) of it: rowsA[ls * row_stride + j] = row i0 + j of launch-local shard ls (span shard s0 + ls).
// !FILL: counts[rank] += the rows of the launch that hold the column.  FILL: their indices, ascending, to
// items[offs[rank] + counts[rank] ...], and counts[rank] moves on.  counts is zeroed before the first launch of each pass.
template <bool FILL>
__global__ void __launch_bounds__(256) k_extract_rows(const uint8_t* __restrict__ arenaA, const uint32_t* __restrict__ rowsA, uint32_t row_stride,
                                                     uint32_t nr, uint32_t i0, uint32_t ns, uint32_t s0, const u64* __restrict__ sel,
                                                     const uint32_t* __restrict__ upre, u64 n, uint32_t* counts, const u64* __restrict__ offs,
                                                     uint32_t* __restrict__ items, u64 m) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TrConst tc = tr_const(lane);
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    const uint64_t su = (uint64_t)(s0 + ls) * kExtractUnits + un;
    const u64 r0 = upre[su];
    if (upre[su + 1] == r0) continue;  // (wave-uniform)
    const uint32_t* ra = rowsA + (uint64_t)ls * row_stride;
    for (uint32_t j0 = 0; j0 < nr; j0 += 64) {
      const uint32_t j = j0 + (uint32_t)lane;
      const bool live = j < nr;
      u64 aw[kExtractWords];
      extract_load_line(reinterpret_cast<const u64*>(arenaA) + (uint64_t)(live ? ra[j] : 0u) * kExtractRowWords + (uint64_t)un * kExtractWords, live, aw);
      u64 r = r0;
#pragma unroll
      for (uint32_t k = 0; k < kExtractWords; ++k) {
        const u64 x = extract_uniform(sel[su * kExtractWords + k]);
        if (x == 0) continue;
        u64 msk = wave_transpose64(aw[k], tc);  // bit i: the column is in row i0 + j0 + i
        const u64 at = r + extract_below(x);
        if (((x >> lane) & 1) && at < n && msk != 0) {
          const uint32_t c = counts[at];
          counts[at] = c + (uint32_t)__popcll(msk);
          if (FILL) {
            u64 p = offs[at] + c;
            while (msk) {
              if (p < m) items[p] = i0 + j0 + (uint32_t)__builtin_ctzll(msk);
              ++p;
              msk &= msk - 1;
            }
          }
        }
        r += (uint32_t)__popcll(x);
      }
    }
  }
}

// counts [n_tiles * 4096] (zero padded) -> tile_sum[tile]
__global__ void __launch_bounds__(1024) k_extract_tile_sums(const uint32_t* __restrict__ counts, uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t wsum[16];
  const uint4 q = reinterpret_cast<const uint4*>(counts)[(uint64_t)blockIdx.x * 1024 + threadIdx.x];
  uint32_t total;
  (void)extract_block_scan(q.x + q.y + q.z + q.w, wsum, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// offs[i] = tile_base[tile] + the counts before i inside the tile, for i < n_out
__global__ void __launch_bounds__(1024) k_extract_offsets(const uint32_t* __restrict__ counts, const u64* __restrict__ tile_base, u64 n_out,
                                                         u64* __restrict__ offs) {
  __shared__ uint32_t wsum[16];
  const uint64_t i = ((uint64_t)blockIdx.x * 1024 + threadIdx.x) * 4;
  const uint4 q = reinterpret_cast<const uint4*>(counts)[i / 4];
  uint32_t total;
  const u64 b = tile_base[blockIdx.x] + extract_block_scan(q.x + q.y + q.z + q.w, wsum, &total);
  if (i < n_out) offs[i] = b;
  if (i + 1 < n_out) offs[i + 1] = b + q.x;
  if (i + 2 < n_out) offs[i + 2] = b + q.x + q.y;
  if (i + 3 < n_out) offs[i + 3] = b + q.x + q.y + q.z;
}

}  // namespace fbk
