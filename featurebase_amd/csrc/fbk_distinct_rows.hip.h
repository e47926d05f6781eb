// fbk_distinct_rows.hip.h — Distinct(filter, field=f) over an int field as a ROW (executeDistinctShardBSI, executor.go:2034-2153):
// the reference returns SignedRow{Neg, Pos}, two rows whose COLUMNS are the values (+ bsiGroup.Base; v >= 0 sets column v of Pos,
// v < 0 column -v of Neg, :2123-2130), united over the shards (:1190-1196) — the operand a foreign-key join intersects with
// (handlePreCalls, :362-449).  Setting a bit is de-duplication: no value list, no sort.
//
// The planes are walked as fbk_bsi_sort walks them (sort_walk_unit with a neutral SortKey: the key is the stored value), twice:
//   (k_drow_inner    only for values of both signs that lie too far from 0: the smallest position of either sign, the window's start)
//   k_drow_presence  one bit per output shard (position >> 20) and sign, inside a window [lo, lo + span) of shards the host derived
//                    from the bit depth and the base, or from the minimum and maximum.  A word whose 64 columns fall into one
//                    shard (small keys, clustered keys) issues one OR, not 64 (k_sort_hist's ballot idiom).
//   (host)           the set presence bits are the output rows, ascending, Pos before Neg; the exclusive popcount prefix per
//                    presence word maps a shard to its row; the output arena is n rows of 16 x 8 KiB cells, zeroed.
//   k_drow_scatter   every participating column: row = prefix[word] + the presence bits below its shard, then a 64-bit OR of its
//                    bit.  The word is READ first and no atomic is issued for a bit already set: a join's child index holds many
//                    records per parent, so after the first few thousand columns nearly every bit is set and the pass is loads.
//   k_drow_finish    one wavefront per output cell: cardinality, run count (bitmapCountRuns), the cell's Slot.
// OR of bits commutes: the result does not depend on the grid, the chunking or the order of the blocks.
#pragma once
#include "fbk_sort.hip.h"

namespace fbk {

constexpr uint32_t kDrowWindowShards = 1u << 23;  // shards a sign's presence bitmap spans at most (2^20 bytes)

struct DrowWindow {
  u64 lo[2];         // first shard of the window: [0] Pos, [1] Neg
  uint32_t span[2];  // shards in it (0: the sign cannot occur), <= kDrowWindowShards
  uint32_t word0[2]; // the sign's first u64 word in the presence bitmap / the prefix table
};

__device__ __forceinline__ u64 drow_lo(const DrowWindow& w, uint32_t neg) { return neg ? w.lo[1] : w.lo[0]; }  // (selects: no indexed copy of the arguments)
__device__ __forceinline__ uint32_t drow_span(const DrowWindow& w, uint32_t neg) { return neg ? w.span[1] : w.span[0]; }
__device__ __forceinline__ uint32_t drow_word0(const DrowWindow& w, uint32_t neg) { return neg ? w.word0[1] : w.word0[0]; }

// (sign, position) of a stored value: v = stored + base; v >= 0 -> position v of Pos, else position -v of Neg
__device__ __forceinline__ u64 drow_position(u64 stored, u64 base, uint32_t& neg) {
  const u64 v = stored + base;
  neg = (uint32_t)(v >> 63);
  return neg ? 0ull - v : v;
}

__device__ __forceinline__ void drow_or(u64* w, u64 bit) {
  if ((__atomic_load_n(w, __ATOMIC_RELAXED) & bit) == 0) atomicOr(reinterpret_cast<unsigned long long*>(w), (unsigned long long)bit);
}

// pres[win.word0[sign] + (shard - win.lo[sign]) / 64] |= the bit of every (sign, shard) a participating column's position falls in
__global__ void __launch_bounds__(256) k_drow_presence(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                                      const uint32_t* __restrict__ rowsF, uint32_t ns, uint32_t depth, u64 base, DrowWindow win,
                                                      u64* __restrict__ pres) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TrConst tc = tr_const(lane);
  const SortKey sk = value_key();
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    sort_walk_unit(arenaS, rowsS, arenaF, rowsF, ls, un, depth, sk, lane, tc, [&](uint32_t, u64 key, bool part) {
      uint32_t neg;
      const u64 rel = (drow_position(key, base, neg) >> 20) - drow_lo(win, neg);
      const bool hit = part && rel < (u64)drow_span(win, neg);  // (the window holds every position: the test keeps a wrong one from a store)
      const uint32_t code = (neg << 31) | (uint32_t)rel;   // (rel < 2^23 where hit)
      const u64 act = __ballot(hit);
      if (act == 0) return;
      const uint32_t first = (uint32_t)__builtin_ctzll(act);
      const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)first);
      const bool one = __ballot(hit && code == c0) == act;  // every column of the word in one shard: one OR
      if (one ? (uint32_t)lane == first : hit) drow_or(pres + drow_word0(win, neg) + (rel >> 6), 1ull << (rel & 63));
    });
  }
}

// inner[0] / inner[1] = the smallest position of Pos / Neg among the participating columns (both ~0 before; min commutes).  For a
// field with values of both signs whose windows cannot start at 0: one atomic per sign and unit that holds such a column.
__global__ void __launch_bounds__(256) k_drow_inner(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                                   const uint32_t* __restrict__ rowsF, uint32_t ns, uint32_t depth, u64 base, u64* __restrict__ inner) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TrConst tc = tr_const(lane);
  const SortKey sk = value_key();
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    u64 mp = ~0ull, mn = ~0ull;
    sort_walk_unit(arenaS, rowsS, arenaF, rowsF, ls, un, depth, sk, lane, tc, [&](uint32_t, u64 key, bool part) {
      uint32_t neg;
      const u64 p = drow_position(key, base, neg);
      if (part && !neg) mp = p < mp ? p : mp;
      if (part && neg) mn = p < mn ? p : mn;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 op = (u64)__shfl_xor((unsigned long long)mp, o, kWave), on = (u64)__shfl_xor((unsigned long long)mn, o, kWave);
      mp = op < mp ? op : mp;
      mn = on < mn ? on : mn;
    }
    if (lane == 0 && mp != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(inner), (unsigned long long)mp);
    if (lane == 1 && mn != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(inner) + 1, (unsigned long long)mn);
  }
}

// arena: rows of kSlots cells of 8 KiB, zeroed; row of (sign, shard) = row0[sign] + pre[word] + popcount(pres[word] below the shard)
__global__ void __launch_bounds__(256) k_drow_scatter(const uint8_t* __restrict__ arenaS, const uint32_t* __restrict__ rowsS, const uint8_t* __restrict__ arenaF,
                                                     const uint32_t* __restrict__ rowsF, uint32_t ns, uint32_t depth, u64 base, DrowWindow win,
                                                     const u64* __restrict__ pres, const uint32_t* __restrict__ pre, uint32_t n_pos, uint32_t n_rows,
                                                     u64* __restrict__ arena) {
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TrConst tc = tr_const(lane);
  const SortKey sk = value_key();
  const uint64_t units = (uint64_t)ns * kExtractUnits;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + wv; u < units; u += (uint64_t)gridDim.x * 4) {
    const uint32_t ls = uint32_t(u / kExtractUnits), un = uint32_t(u % kExtractUnits);
    sort_walk_unit(arenaS, rowsS, arenaF, rowsF, ls, un, depth, sk, lane, tc, [&](uint32_t, u64 key, bool part) {
      uint32_t neg;
      const u64 p = drow_position(key, base, neg);
      const u64 rel = (p >> 20) - drow_lo(win, neg);
      if (!(part && rel < (u64)drow_span(win, neg))) return;
      const uint32_t w = drow_word0(win, neg) + (uint32_t)(rel >> 6);
      const u64 pw = pres[w], bit = 1ull << (rel & 63);
      const uint32_t row = (neg ? n_pos : 0u) + pre[w] + (uint32_t)__popcll(pw & (bit - 1));
      if (!(pw & bit) || row >= n_rows) return;  // (k_drow_presence set the bit: nothing is stored outside the arena)
      drow_or(arena + (uint64_t)row * kExtractRowWords + ((p & 0xFFFFFu) >> 6), 1ull << (p & 63));
    });
  }
}

// one wavefront per cell: slots[cell] = the bitmap at cell * 8 KiB or nil, runs[cell] = bitmapCountRuns, counts[row] += cardinality
// (counts zeroed before; 16 adds of counts per row: they commute)
__global__ void __launch_bounds__(256) k_drow_finish(const uint8_t* __restrict__ arena, uint32_t n_cells, Slot* __restrict__ slots, uint32_t* __restrict__ runs,
                                                    u64* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t cell = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= n_cells) return;  // (wave-uniform)
  u64 w[kWordsPerLane];
  frag_load_bitmap(arena + (uint64_t)cell * 8192, lane, w);
  const uint32_t c = wave_reduce_add(frag_popcount(w));
  const uint32_t r = wave_reduce_add(frag_count_runs(w, lane));
  if (lane == 0) {
    Slot s;
    s.off = (uint64_t)cell * 8192;
    s.len = kWords;
    s.tn = make_tn(c ? kTypeBitmap : kTypeNil, c);
    slots[cell] = s;
    runs[cell] = r;
    if (c) atomicAdd(reinterpret_cast<unsigned long long*>(counts) + cell / kSlots, (unsigned long long)c);
  }
}

}  // namespace fbk
