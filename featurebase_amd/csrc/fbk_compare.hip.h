// fbk_compare.hip.h — fbk_bsi_compare: the Row of `value_x op value_y` over two int (BSI) fields, the column-against-column
// predicate of SQL WHERE x < y.  It is the BSI Range scan (k_bsi_range_slot, fbk_bsi_kernels.hip.h) with the constant's bit
// replaced by the other field's plane: one WAVEFRONT per (shard, slot), 16 words per lane, every plane of either field read
// exactly once in its encoded form, nothing transposed and no value ever formed.  The rules (which instance, how many steps,
// the final combination) are fbk_compare_plan.h's.
//
// The walk is LSB -> MSB, so the unsigned comparison needs no second pass: with a, b the two bits of a step,
//     lt = (~a & b) | (~(a ^ b) & lt)        gt = (a & ~b) | (~(a ^ b) & gt)
// — the highest differing bit wins because it is applied last.
//
// The plane loop asks for containers in the order a0 b0 a1 b1 ... (a: x's plane, b: y's); request j lands in register set j % 3, so
// while step i (sets 2i % 3 and (2i + 1) % 3) is applied, a of step i + 1 is in flight in the third set, and the two sets of step
// i are asked for b of i + 1 and a of i + 2 as soon as they are free (a load never depends on the accumulators).  The loop body is
// ONE straight-line step whatever the operands are: a plane at or above a field's depth, or a nil container, is not read — a
// wave-uniform mask turns its register set into zeros.  (A body that branched on the kind of step, with the signs, exists and the
// filter as steps of the same loop, cost the register allocator 800 bytes of spills; range_sum_plane found the same.)  Signs,
// exists and the filter are read before / after the loop, into the same three sets.
//   OFFSET = false (base_x == base_y):   W0 = max(depth_x, depth_y) plane steps, then the signs, then E
//     a, b are the magnitude planes; nz |= a | b.  After the walk, with the signs sx, sy,
//         x < y  <=>  (sx & ~sy & nz) | (~sx & ~sy & lt) | (sx & sy & gt)      x > y mirrored      x == y: neither.
//     The raw signs get "-0 against 0" wrong and nothing else; nz repairs it.  Three accumulators: lt, gt in registers, nz in LDS
//     (each lane reads only what it wrote): 160 registers of state and loads, two wavefronts per SIMD as k_bsi_range_slot.
//   OFFSET = true:   the signs, then W plane steps (fbk_compare_plan::steps), then E
//     both values stream into two's complement, t = (plane ^ s) ^ c; c &= (plane ^ s), c starting as the sign (-m = ~m + 1);
//     k = base_x - base_y is added to x's stream with a wave-uniform bit per step (kbit 0: u = t ^ ck; ck &= t;  kbit 1:
//     u = ~(t ^ ck); ck |= t); u and y's stream go through the recurrence, with a and b exchanged at step W - 1 (the sign bit of a
//     W-bit number: the side that has it is the smaller one).  Carries out of step W - 1 are discarded.  Five accumulators in
//     registers: lt, gt, cx, cy, ck; the two signs live in LDS.
// E = exists_x & exists_y (& filter) masks the result at the end: junk sign and plane bits outside exists make junk in lt / gt of
// their own columns only.
#pragma once
#include "fbk_bsi_kernels.hip.h"

namespace fbk {

struct CompareArgs {
  const Slot* xslots;
  const uint8_t* xarena;
  const uint32_t* xbase;
  const Slot* yslots;
  const uint8_t* yarena;
  const uint32_t* ybase;
  const Slot* fslots;  // nullptr: no filter
  const uint8_t* farena;
  const uint32_t* frows;
  uint8_t* arenaO;  // WRITE = 1: the output cells, their descriptors and (or nullptr) their run counts
  Slot* outSlots;
  uint32_t* outRuns;
  u64* out_counts;  // per shard, zeroed by the caller; may be nullptr when WRITE = 1
  u64 k_low;        // bits 0..63 of k = base_x - base_y (OFFSET only)
  uint32_t k_neg;   // every bit from 64 on
  uint32_t n_shards, depth_x, depth_y;
  uint32_t steps;                      // W0 / W (fbk_compare_plan::steps)
  uint32_t take_lt, take_gt, invert;  // fbk_compare_plan::combine
  uint32_t encode;                     // WRITE = 1: Container.optimize() in the epilogue (frag_store_encoded)
};

constexpr int kCompareDescs = 72;  // exists, sign and at most 64 planes of one field (bsi_stage_descs stages depth + 2 <= 66 of them)
static_assert(kCompareDescs <= kBsiDescCap, "");

// WRITE: 0 counts only (no cell and no descriptor is written), 1 cells
template <bool OFFSET, int WRITE>
__global__ void __launch_bounds__(64, OFFSET ? 1 : 2) k_bsi_compare_slot(const CompareArgs g) {
  __shared__ u64 lds[kWords];
  __shared__ Slot tabx[kCompareDescs], taby[kCompareDescs];
  __shared__ u64 keep[OFFSET ? 2 * kWords : kWords];  // OFFSET: sx, sy, read at every plane step; otherwise nz
  const int lane = threadIdx.x;
  const uint64_t cell = blockIdx.x;
  const uint64_t shard = cell >> 4;
  const uint32_t slot = cell & 15;
  if (shard >= g.n_shards) return;
  const uint64_t rx = g.xbase[shard], ry = g.ybase[shard];
  bsi_stage_descs(g.xslots, rx, slot, g.depth_x + 2, lane, tabx);
  bsi_stage_descs(g.yslots, ry, slot, g.depth_y + 2, lane, taby);
  Slot sf;
  sf.off = 0, sf.len = 0, sf.tn = 0;
  if (g.fslots) sf = g.fslots[(uint64_t)g.frows[shard] * kSlots + slot];
  // no participating column in this slot: exists_x, exists_y or the filter has no container here (wave-uniform)
  if (slot_n(tabx[0]) == 0 || slot_n(taby[0]) == 0 || (g.fslots && slot_n(sf) == 0)) {
    if (WRITE && lane == 0) {
      Slot so;
      so.off = cell * 8192ull, so.len = kWords, so.tn = make_tn(kTypeNil, 0);
      g.outSlots[cell] = so;
      if (g.outRuns) g.outRuns[cell] = 0;
    }
    return;
  }
  const uint32_t W = g.steps;
  u64 lt[kWordsPerLane], gt[kWordsPerLane];
  u64 cx[OFFSET ? kWordsPerLane : 1], cy[OFFSET ? kWordsPerLane : 1], ck[OFFSET ? kWordsPerLane : 1];
  u64 T[3][kWordsPerLane];
  frag_zero(lt);
  frag_zero(gt);
#pragma unroll
  for (int u = 0; u < 3; ++u) frag_zero(T[u]);
  // row r of a field's fragment (0 exists, 1 sign, 2 + i plane i); beyond the field's depth: no container, like a nil one
  auto row_x = [&](uint32_t r) __attribute__((always_inline)) {
    Slot sp;
    sp.off = 0, sp.len = 0, sp.tn = 0;
    if (r < g.depth_x + 2u) sp = tabx[r];
    return sp;
  };
  auto row_y = [&](uint32_t r) __attribute__((always_inline)) {
    Slot sp;
    sp.off = 0, sp.len = 0, sp.tn = 0;
    if (r < g.depth_y + 2u) sp = taby[r];
    return sp;
  };
  // a container without bits is not read and the register set keeps what it held: the caller masks it with mask_of()
  auto fetch = [&](const Slot& sp, const uint8_t* __restrict__ arena, u64(&w)[kWordsPerLane]) __attribute__((always_inline)) {
    if (slot_n(sp)) frag_load(sp, arena, lane, lds, w);
  };
  auto mask_of = [](const Slot& sp) __attribute__((always_inline)) { return slot_n(sp) ? ~0ull : 0ull; };

  if constexpr (OFFSET) {
    const Slot ssx = row_x(1), ssy = row_y(1);
    fetch(ssx, g.xarena, T[0]);
    fetch(ssy, g.yarena, T[1]);
    const u64 mx = mask_of(ssx), my = mask_of(ssy);
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) {
      const u64 sx = T[0][q] & mx, sy = T[1][q] & my;
      keep[q * kWave + lane] = sx;
      keep[kWords + q * kWave + lane] = sy;
      cx[OFFSET ? q : 0] = sx;
      cy[OFFSET ? q : 0] = sy;
      ck[OFFSET ? q : 0] = 0;
    }
  } else {
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) keep[q * kWave + lane] = 0;
  }

  // request j of the plane loop: plane j / 2 of x (j even) or of y (j odd)
  auto request = [&](uint32_t j, u64(&w)[kWordsPerLane]) __attribute__((always_inline)) {
    const uint32_t i = j >> 1;
    if (i >= W) return;
    if (j & 1u) fetch(row_y(2u + i), g.yarena, w);
    else fetch(row_x(2u + i), g.xarena, w);
  };
  auto step = [&](uint32_t i, const u64(&A)[kWordsPerLane], const u64(&B)[kWordsPerLane]) __attribute__((always_inline)) {
    const u64 ma = mask_of(row_x(2u + i)), mb = mask_of(row_y(2u + i));  // (wave-uniform)
    if constexpr (OFFSET) {
      const u64 kb = (i < 64u ? (uint32_t)(g.k_low >> i) & 1u : g.k_neg) ? ~0ull : 0ull;  // bit i of k
      const u64 sw = i + 1u == W ? ~0ull : 0ull;                                          // the sign bit: a and b exchanged
#pragma unroll
      for (int q = 0; q < kWordsPerLane; ++q) {
        const u64 ax = (A[q] & ma) ^ keep[q * kWave + lane], ay = (B[q] & mb) ^ keep[kWords + q * kWave + lane];
        const u64 t = ax ^ cx[OFFSET ? q : 0];
        cx[OFFSET ? q : 0] &= ax;
        const u64 b = ay ^ cy[OFFSET ? q : 0];
        cy[OFFSET ? q : 0] &= ay;
        const u64 c = ck[OFFSET ? q : 0];
        const u64 a = t ^ c ^ kb;
        ck[OFFSET ? q : 0] = (c & t) | (kb & (c | t));  // kbit 0: ck &= t; kbit 1: ck |= t
        const u64 d = a ^ b;
        lt[q] = (d & (b ^ (d & sw))) | (~d & lt[q]);
        gt[q] = (d & (a ^ (d & sw))) | (~d & gt[q]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < kWordsPerLane; ++q) {
        const u64 a = A[q] & ma, b = B[q] & mb, d = a ^ b;
        lt[q] = (d & b) | (~d & lt[q]);
        gt[q] = (d & a) | (~d & gt[q]);
        keep[q * kWave + lane] |= a | b;
      }
    }
  };
#pragma unroll
  for (int u = 0; u < 3; ++u) request((uint32_t)u, T[u]);
  for (uint32_t i0 = 0; i0 < W; i0 += 3) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const uint32_t i = i0 + (uint32_t)u;
      if (i < W) {  // (wave-uniform)
        step(i, T[(2 * u) % 3], T[(2 * u + 1) % 3]);
        __builtin_amdgcn_sched_barrier(0);     // (loads hoisted above the step would need registers of their own)
        request(2u * i + 3u, T[(2 * u) % 3]);  // these two register sets are free again
        request(2u * i + 4u, T[(2 * u + 1) % 3]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  if constexpr (!OFFSET) {
    const Slot ssx = row_x(1), ssy = row_y(1);
    fetch(ssx, g.xarena, T[0]);
    fetch(ssy, g.yarena, T[1]);
    const u64 mx = mask_of(ssx), my = mask_of(ssy);
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) {
      const u64 sx = T[0][q] & mx, sy = T[1][q] & my, nz = keep[q * kWave + lane], l = lt[q], h = gt[q];
      lt[q] = (sx & ~sy & nz) | (~sx & ~sy & l) | (sx & sy & h);
      gt[q] = (sy & ~sx & nz) | (~sx & ~sy & h) | (sx & sy & l);
    }
  }
  // E and the operator's combination of lt / gt (exists_x, exists_y and the filter have containers here: checked above)
  __builtin_amdgcn_sched_barrier(0);  // (these loads are not to be hoisted above the signs: no registers for them there)
  frag_load(tabx[0], g.xarena, lane, lds, T[0]);
  frag_load(taby[0], g.yarena, lane, lds, T[1]);
#pragma unroll
  for (int q = 0; q < kWordsPerLane; ++q) T[0][q] &= T[1][q];
  if (g.fslots) {
    frag_load(sf, g.farena, lane, lds, T[1]);
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) T[0][q] &= T[1][q];
  }
  const u64 ml = g.take_lt ? ~0ull : 0ull, mg = g.take_gt ? ~0ull : 0ull, inv = g.invert ? ~0ull : 0ull;
#pragma unroll
  for (int q = 0; q < kWordsPerLane; ++q) lt[q] = T[0][q] & (((lt[q] & ml) | (gt[q] & mg)) ^ inv);
  const uint32_t c = wave_reduce_add(frag_popcount(lt));
  if (WRITE) {
    Slot so;
    so.off = cell * 8192ull;
    so.len = kWords;
    so.tn = make_tn(c ? kTypeBitmap : kTypeNil, c);
    uint32_t rr = 0;
    if (g.outRuns || g.encode) rr = wave_reduce_add(frag_count_runs(lt, lane));
    if (g.encode && c) {  // Container.optimize() applied here, as k_bsi_range_slot does
      uint32_t t_out, l_out;
      frag_store_encoded(lt, c, rr, lane, lds, g.arenaO + so.off, t_out, l_out);
      so.len = l_out;
      so.tn = make_tn(t_out, c);
    } else if (c) {
      frag_store_bitmap(g.arenaO + so.off, lane, lt);
    }
    if (lane == 0) {
      g.outSlots[cell] = so;
      if (g.outRuns) g.outRuns[cell] = rr;
    }
  }
  if (lane == 0 && c && g.out_counts) atomicAdd(&g.out_counts[shard], (u64)c);
}

}  // namespace fbk
