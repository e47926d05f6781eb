// fbk_expr.hip.h — k_expr_slot: a whole bitmap call tree per (shard, slot) in one launch (fbk_expr_*; included by fbk.hip), and
// k_expr_agg_slot: the same tree, then Sum / Min / Max of a BSI field over its result (fbk_expr_bsi_agg; at the end of the file).
//
// The host planner (fbk_expr_plan.h) lowers the caller's postfix program to a straight-line instruction list over an
// accumulator X, the BSI scans' matched register M and a stack of saved fragments.  One WAVEFRONT runs that list on one
// 8 KiB container column, 16 words per lane, exactly as k_bsi_range_slot runs a plane program — the BSI leaves of a tree
// ARE such programs, expanded in place, and a set leaf is one more "X op= row" instruction of the same kind:
//   * X, M and the kAhead = 2 operands in flight live in registers (4 x 32 VGPRs, two wavefronts per SIMD);
//   * the stack lives in LDS, sized PER LAUNCH from what the lowered program needs (dynamic shared memory: 8 KiB of decode
//     scratch plus 8 KiB per saved fragment).  A register array indexed by a run-time stack pointer would go to scratch
//     memory; LDS indexed by a wave-uniform pointer costs nothing, and a typical WHERE clause needs no saved value at all
//     (every "op leaf" is applied to X directly), so it runs at the occupancy of the BSI kernel;
//   * an operand's address never depends on X: the container of instruction pc + kAhead is requested before instruction
//     pc is applied (the issue(pc + kAhead) pattern of k_bsi_range_slot).  Leaf table, row lists, instruction words and
//     descriptors are wave-uniform and come through scalar loads;
//   * a nil container is zeros and a full one (n = 65536) ones, without a load;
//   * epilogue as the neighbours: popcount, run count, Container.optimize() through frag_store_encoded when asked for.
// No write to memory before the epilogue; the per-shard count is one vector atomicAdd per non-empty cell.
#pragma once
#include "fbk_kernels.hip.h"
#include "fbk_bsi_kernels.hip.h"
#include "fbk_expr_plan.h"

namespace fbk {

// one leaf of the call tree on the device (32 bytes, wave-uniform: scalar loads)
struct alignas(16) ExprLeaf {
  const Slot* slots;
  const uint8_t* arena;
  const uint32_t* rows;  // [n_shards]: the shard's row (ROW leaf) or the base row of its BSI fragment
  uint32_t n_rows;       // rows of the leaf per shard: 1, or bit depth + 2
  uint32_t pad;
};

// X = f(X, t) for the instructions kLoad .. kAndnRev, t(q) the operand's word q (N words per thread: 16 in the wavefront
// evaluator below, 4 in the block-wide one of fbk_expr_topk.hip.h)
template <int N, class F>
__device__ __forceinline__ void expr_apply_x(uint32_t op, u64 (&X)[N], F t) {
  if (op == fbk_expr::kXor) {
#pragma unroll
    for (int q = 0; q < N; ++q) X[q] ^= t(q);
  } else {
    // ((X ^ a) | k) & (T ^ b)) ^ c: uniform masks instead of one loop per operation
    const u64 a = (op == fbk_expr::kAndnRev || op == fbk_expr::kOr) ? ~0ull : 0ull;
    const u64 k = op == fbk_expr::kLoad ? ~0ull : 0ull;
    const u64 b = (op == fbk_expr::kAndn || op == fbk_expr::kOr) ? ~0ull : 0ull;
    const u64 c = op == fbk_expr::kOr ? ~0ull : 0ull;
#pragma unroll
    for (int q = 0; q < N; ++q) X[q] = ((((X[q] ^ a) | k) & (t(q) ^ b)) ^ c);
  }
}

// The lowered program on one (shard, slot), shared by k_expr_slot and k_expr_agg_slot: X holds the tree's value when it returns.
// lds = [0, kWords) decode scratch, then 8 KiB per saved fragment; M and the kAhead operand buffers T are the caller's, so that it
// can go on using their registers.
constexpr int kExprAhead = 2;
__device__ __forceinline__ void expr_run(const ExprLeaf* __restrict__ leaves, const uint32_t* __restrict__ prog, uint32_t prog_len, uint64_t shard,
                                         uint32_t slot, int lane, uint32_t n_saved, u64* lds, u64 (&X)[kWordsPerLane], u64 (&M)[kWordsPerLane],
                                         u64 (&T)[kExprAhead][kWordsPerLane]) {
  constexpr int kAhead = kExprAhead;
  u64* stack = lds + kWords;
  frag_zero(X);
  frag_zero(M);
  uint32_t sp = 0;  // (wave-uniform)
  auto issue = [&](uint32_t pc, u64 (&w)[kWordsPerLane]) {
    if (pc >= prog_len) return;
    const uint32_t ins = prog[pc];
    if ((ins >> 24) > fbk_expr::kMorXAn) return;  // no operand
    const ExprLeaf& lf = leaves[(ins >> fbk_expr::kLeafShift) & 0xFFFu];
    const uint64_t row = (uint64_t)lf.rows[shard] + (ins & fbk_expr::kRowMask);
    const Slot s = lf.slots[row * kSlots + slot];
    const uint32_t n = slot_n(s);
    if (n == 0) {
      frag_zero(w);
    } else if (n == 65536u) {
#pragma unroll
      for (int q = 0; q < kWordsPerLane; ++q) w[q] = ~0ull;
    } else {
      frag_load(s, lf.arena, lane, lds, w);
    }
  };
#pragma unroll
  for (int u = 0; u < kAhead; ++u) {
    frag_zero(T[u]);
    issue((uint32_t)u, T[u]);
  }
  for (uint32_t pc0 = 0; pc0 < prog_len; pc0 += kAhead) {
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const uint32_t pc = pc0 + (uint32_t)u;
      if (pc < prog_len) {  // (wave-uniform)
        const uint32_t op = prog[pc] >> 24;
        if (op <= fbk_expr::kAndnRev) {
          expr_apply_x(op, X, [&](int q) { return T[u][q]; });
        } else if (op <= fbk_expr::kMorXAn) {
          const u64 inv = op == fbk_expr::kMorXAn ? ~0ull : 0ull;
#pragma unroll
          for (int q = 0; q < kWordsPerLane; ++q) M[q] |= X[q] & (T[u][q] ^ inv);
        } else if (op == fbk_expr::kMZero) {
          frag_zero(M);
        } else if (op == fbk_expr::kXFromM) {
#pragma unroll
          for (int q = 0; q < kWordsPerLane; ++q) X[q] = M[q];
        } else if (op == fbk_expr::kZeroX) {
          frag_zero(X);
        } else if (op == fbk_expr::kPush && sp < n_saved) {  // (n_saved: what the launch sized the stack for)
          u64* s = stack + (size_t)sp * kWords;  // a lane reads back only the words it wrote: no synchronisation
#pragma unroll
          for (int q = 0; q < kWordsPerLane; ++q) s[q * kWave + lane] = X[q];
          ++sp;
        } else if (op > fbk_expr::kPop && sp) {
          --sp;
          const u64* s = stack + (size_t)sp * kWords;
          expr_apply_x(op - fbk_expr::kPop, X, [&](int q) { return s[q * kWave + lane]; });
        }
        issue(pc + kAhead, T[u]);
      }
    }
  }
}

__global__ void __launch_bounds__(64) k_expr_slot(const ExprLeaf* __restrict__ leaves, const uint32_t* __restrict__ prog, uint32_t prog_len,
                                                 uint32_t n_shards, uint32_t n_saved, uint8_t* __restrict__ arenaO, Slot* __restrict__ outSlots,
                                                 uint32_t* __restrict__ outRuns, u64* __restrict__ out_counts, uint32_t encode) {
  extern __shared__ u64 expr_lds[];  // [0, kWords): decode scratch / encode staging; then 8 KiB per saved fragment
  u64* lds = expr_lds;
  const int lane = threadIdx.x;
  const uint64_t cell = blockIdx.x;
  const uint64_t shard = cell >> 4;
  const uint32_t slot = cell & 15;
  if (shard >= n_shards) return;
  u64 X[kWordsPerLane], M[kWordsPerLane], T[kExprAhead][kWordsPerLane];
  expr_run(leaves, prog, prog_len, shard, slot, lane, n_saved, lds, X, M, T);
  const uint32_t c = wave_reduce_add(frag_popcount(X));
  if (!outSlots) {  // count only
    if (lane == 0 && c) atomicAdd(&out_counts[shard], (u64)c);
    return;
  }
  Slot so;
  so.off = cell * 8192ull;
  so.len = kWords;
  so.tn = make_tn(c ? kTypeBitmap : kTypeNil, c);
  uint32_t rr = 0;
  if (outRuns || encode) rr = wave_reduce_add(frag_count_runs(X, lane));  // bitmapCountRuns (roaring.go:3372-3380)
  if (encode && c) {  // Container.optimize() applied here (frag_store_encoded, fbk_kernels.hip.h): the scratch is free now
    uint32_t t_out, l_out;
    frag_store_encoded(X, c, rr, lane, lds, arenaO + so.off, t_out, l_out);
    so.len = l_out;
    so.tn = make_tn(t_out, c);
  } else if (c) {
    frag_store_bitmap(arenaO + so.off, lane, X);
  }
  if (lane == 0) {
    outSlots[cell] = so;
    if (outRuns) outRuns[cell] = rr;
    if (c && out_counts) atomicAdd(&out_counts[shard], (u64)c);
  }
}

// ---- the tree, then Sum / Min / Max of a BSI field over it (fbk_expr_bsi_agg, fbk_query_expr_bsi) ------------------------------
// executeSum / executeMin / executeMax evaluate the filter (executeBitmapCallShard) and hand the Row to fragment.sum / min / max
// (fragment.go:724-853).  Here the filter never leaves the wavefront: when the program ends, X IS the filter fragment k_bsi_sum_slot
// and k_bsi_minmax_slot start from, and M and the two operand buffers are free — the registers their scans need.  The field's
// descriptors are staged in static LDS next to the dynamic block (bsi_stage_descs), its containers decode through the scratch at
// [0, kWords) (the saved values above it are dead by now).  X &= exists first: a nil exists container gives zeros, a full one
// leaves X as it is without a load.  agg = FBK_AGG_SUM (0): the arithmetic of k_bsi_sum_slot — pos in X, neg in M, the planes
// through T[0..1] with both loads in flight, popcount << i per lane in uint64 (wrap-around), one wave reduction at the end,
// out[shard * 3] += {psum, nsum, count}; a wave whose |X| is 0 returns without touching the planes.  FBK_AGG_MIN (1) / _MAX (2): the
// scan of k_bsi_minmax_slot — F = X, the sign decision through M, the current plane in T[0] and the next one, requested before
// the current one decides, in T[1]; out[cell * 2] = {magnitude, count | scan flag}, folded per shard on the host (bsi_minmax_fold).
__global__ void __launch_bounds__(64) k_expr_agg_slot(const ExprLeaf* __restrict__ leaves, const uint32_t* __restrict__ prog, uint32_t prog_len,
                                                     uint32_t n_shards, uint32_t n_saved, const Slot* __restrict__ slots,
                                                     const uint8_t* __restrict__ arena, const uint32_t* __restrict__ base, uint32_t bit_depth,
                                                     uint32_t agg, u64* __restrict__ out) {
  extern __shared__ u64 expr_lds[];
  __shared__ Slot tab[kBsiDescCap];
  u64* lds = expr_lds;
  const int lane = threadIdx.x;
  const uint64_t cell = blockIdx.x;
  const uint64_t shard = cell >> 4;
  const uint32_t slot = cell & 15;
  if (shard >= n_shards) return;
  u64 X[kWordsPerLane], M[kWordsPerLane], T[kExprAhead][kWordsPerLane];
  expr_run(leaves, prog, prog_len, shard, slot, lane, n_saved, lds, X, M, T);
  const uint64_t r0 = base[shard];
  bsi_stage_descs(slots, r0, slot, bit_depth + 2, lane, tab);
  auto load_row = [&](uint32_t r, u64 (&w)[kWordsPerLane]) {  // row r of the fragment: 0 exists, 1 sign, 2 + i plane i
    const Slot sp = bsi_desc(slots, r0, slot, r, tab);
    if (slot_n(sp) == 0) frag_zero(w);
    else frag_load(sp, arena, lane, lds, w);
  };
  {
    const uint32_t ne = slot_n(tab[0]);
    if (ne == 0) {
      frag_zero(X);
    } else if (ne != 65536u) {
      load_row(0, T[0]);
#pragma unroll
      for (int q = 0; q < kWordsPerLane; ++q) X[q] &= T[0][q];
    }
  }
  uint32_t cur = wave_reduce_add(frag_popcount(X));
  if (agg == 0) {  // FBK_AGG_SUM
    if (cur == 0) return;  // (wave-uniform) nothing considered in this slot
    load_row(1, T[0]);
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) {
      M[q] = X[q] & T[0][q];
      X[q] &= ~T[0][q];
    }
    u64 psum = 0, nsum = 0;
#pragma unroll
    for (int u = 0; u < kExprAhead; ++u)
      if ((uint32_t)u < bit_depth) load_row(2u + (uint32_t)u, T[u]);
    for (uint32_t i0 = 0; i0 < bit_depth; i0 += kExprAhead) {
#pragma unroll
      for (int u = 0; u < kExprAhead; ++u) {
        const uint32_t i = i0 + (uint32_t)u;
        if (i < bit_depth) {  // (wave-uniform)
          uint32_t pc = 0, nc = 0;
#pragma unroll
          for (int q = 0; q < kWordsPerLane; ++q) {
            pc += __popcll(X[q] & T[u][q]);
            nc += __popcll(M[q] & T[u][q]);
          }
          psum += (u64)pc << i;
          nsum += (u64)nc << i;
          if (i + kExprAhead < bit_depth) load_row(2u + i + kExprAhead, T[u]);  // this register set is free again
        }
      }
    }
    psum = wave_reduce_add_u64(psum);
    nsum = wave_reduce_add_u64(nsum);
    if (lane == 0) {
      if (psum) atomicAdd(&out[shard * 3 + 0], psum);
      if (nsum) atomicAdd(&out[shard * 3 + 1], nsum);
      atomicAdd(&out[shard * 3 + 2], (u64)cur);
    }
    return;
  }
  const bool is_min = agg == 1;  // FBK_AGG_MIN; otherwise FBK_AGG_MAX
  if (cur == 0) {
    if (lane == 0) {
      out[cell * 2] = 0;
      out[cell * 2 + 1] = 0;
    }
    return;
  }
  bool scan_max;
  {
    load_row(1, T[0]);  // sign: negatives decide a minimum, positives a maximum
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) M[q] = is_min ? (X[q] & T[0][q]) : (X[q] & ~T[0][q]);
    const uint32_t g = wave_reduce_add(frag_popcount(M));
    scan_max = g != 0;
    if (g != 0) {
      cur = g;
#pragma unroll
      for (int q = 0; q < kWordsPerLane; ++q) X[q] = M[q];
    }
  }
  u64 val = 0;
  if (bit_depth) load_row(2u + (bit_depth - 1), T[0]);
  for (int i = (int)bit_depth - 1; i >= 0; --i) {
    if (i > 0) load_row(2u + (uint32_t)(i - 1), T[1]);  // the next plane, whatever this one decides
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) T[0][q] = scan_max ? (X[q] & T[0][q]) : (X[q] & ~T[0][q]);
    const uint32_t c = wave_reduce_add(frag_popcount(T[0]));
    if (c > 0) {
#pragma unroll
      for (int q = 0; q < kWordsPerLane; ++q) X[q] = T[0][q];
      cur = c;
      if (scan_max) val += 1ull << i;
    } else if (!scan_max) {
      val += 1ull << i;
    }
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) T[0][q] = T[1][q];
  }
  if (lane == 0) {  // (the record of k_bsi_minmax_slot: bit 63 of the count word = maxUnsigned over the deciding sign)
    out[cell * 2] = val;
    out[cell * 2 + 1] = (u64)cur | (scan_max ? (1ull << 63) : 0ull);
  }
}

}  // namespace fbk
