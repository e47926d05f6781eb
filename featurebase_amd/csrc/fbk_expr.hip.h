// fbk_expr.hip.h — k_expr_slot: a whole bitmap call tree per (shard, slot) in one launch (fbk_expr_*; included by fbk.hip).
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

// X = f(X, t) for the instructions kLoad .. kAndnRev, t(q) the operand's word q
template <class F>
__device__ __forceinline__ void expr_apply_x(uint32_t op, u64 (&X)[kWordsPerLane], F t) {
  if (op == fbk_expr::kXor) {
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) X[q] ^= t(q);
  } else {
    // ((X ^ a) | k) & (T ^ b)) ^ c: uniform masks instead of one loop per operation
    const u64 a = (op == fbk_expr::kAndnRev || op == fbk_expr::kOr) ? ~0ull : 0ull;
    const u64 k = op == fbk_expr::kLoad ? ~0ull : 0ull;
    const u64 b = (op == fbk_expr::kAndn || op == fbk_expr::kOr) ? ~0ull : 0ull;
    const u64 c = op == fbk_expr::kOr ? ~0ull : 0ull;
#pragma unroll
    for (int q = 0; q < kWordsPerLane; ++q) X[q] = ((((X[q] ^ a) | k) & (t(q) ^ b)) ^ c);
  }
}

__global__ void __launch_bounds__(64) k_expr_slot(const ExprLeaf* __restrict__ leaves, const uint32_t* __restrict__ prog, uint32_t prog_len,
                                                 uint32_t n_shards, uint32_t n_saved, uint8_t* __restrict__ arenaO, Slot* __restrict__ outSlots,
                                                 uint32_t* __restrict__ outRuns, u64* __restrict__ out_counts, uint32_t encode) {
  extern __shared__ u64 expr_lds[];  // [0, kWords): decode scratch / encode staging; then 8 KiB per saved fragment
  u64* lds = expr_lds;
  u64* stack = expr_lds + kWords;
  const int lane = threadIdx.x;
  const uint64_t cell = blockIdx.x;
  const uint64_t shard = cell >> 4;
  const uint32_t slot = cell & 15;
  if (shard >= n_shards) return;
  constexpr int kAhead = 2;
  u64 X[kWordsPerLane], M[kWordsPerLane], T[kAhead][kWordsPerLane];
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

}  // namespace fbk
