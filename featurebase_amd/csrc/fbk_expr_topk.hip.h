// fbk_expr_topk.hip.h — k_expr_rows_vs_filter: counts[shard][i] = |A[shard][i] ∩ tree(shard)| for many rows of a field and a
// whole bitmap call tree, in one launch (fbk_expr_row_counts / fbk_expr_topk / fbk_expr_topn; included by fbk.hip).
//
// TopK(f, filter=<tree>), TopN(f, <tree>, n=) and GroupBy(Rows(f), filter=<tree>) evaluate the tree per shard
// (executeBitmapCallShard) and count every row of the field against the result (doTopK, executor.go:2705-2746; fragment.top,
// fragment.go:1317-1437).  The pair fbk_expr_eval + fbk_topk writes that result as 8 KiB cells and reads it back per (shard, slot,
// chunk of rows); here it never leaves the block.  The block has the shape of k_rows_vs_filter (fbk_topk_kernels.hip.h) — 256
// threads per (shard, slot, chunk of rows), the filter container as the 1024-word bitmap F plus its rank table in LDS, the rows
// streaming past it in their encoded form through rows_stream_past_filter — and the one difference that it COMPUTES F:
//
//   * expr_run_block runs the lowered instruction list of fbk_expr_plan.h (the same words k_expr_slot interprets) on one
//     container column with all 256 threads, 4 words per thread: X and M are 4 x u64, an operand 4 more.  The wavefront
//     evaluator expr_run holds 16 words per lane four times over (205 VGPRs in k_expr_slot); a kernel is allocated the maximum
//     over its phases, and the streaming phase needs 8 wavefronts per SIMD (fbk_fold_kernels.hip.h), that is 64 VGPRs.
//   * a bitmap operand: every thread loads its own 32 bytes.  Nil is zeros and n = 65536 ones, neither is loaded.
//   * an array / run operand: the threads zero the 8 KiB buffer T (each the words it is going to read), the four wavefronts
//     scatter the payload into it as 1 KiB chunks (scatter_chunk<1> of the n-way folds: one LDS OR per value, two masked ORs
//     and whole dwords per run), every thread reads its 4 words.  Two barriers per such operand.
//   * the descriptors of a window of 256 instructions (program word -> leaf -> shard's row -> descriptor: four dependent loads,
//     none of which depends on X) are resolved by the 256 threads side by side into F, which is free until the program ends, and
//     the bitmap payload of the next instruction is in flight while the current one is applied.
//   * saved values (kPush / kPop + op) live in dynamic LDS, 8 KiB each, Plan::slots of them; a thread reads back only what it
//     wrote, so they need no barrier.
//   * when the program ends X goes to F, the rank table is built as in k_rows_vs_filter; |F| = 0 ends the block before it reads
//     a row, |F| = 65536 takes the f_full path.  The chunk-0 block of a (shard, slot) adds |F| to d_src[shard] (TopN's Tanimoto
//     rule needs the per-shard filter count; fbk_expr_row_counts returns it).
// Nothing is written to memory before the counts.
//
// Static LDS: F 8 KiB + rank 4 KiB + T 8 KiB = 20 KiB exactly — 8 blocks per CU (160 KiB), 8 wavefronts per SIMD.  rank[kWords]
// (= |F|) and the four wave totals of the rank scan have no room of their own: they live in the head of T, which is dead by then.
// Each saved value adds 8 KiB and costs occupancy (one: 5 blocks per CU).
#pragma once
#include "fbk_expr.hip.h"
#include "fbk_fold_kernels.hip.h"
#include "fbk_topk_kernels.hip.h"

namespace fbk {

// The lowered program on one (shard, slot) with the whole block: thread t holds the 16-byte chunks t and 256 + t of the
// column (words 2t, 2t + 1, 512 + 2t, 513 + 2t).  X holds the tree's value when it returns.  T: 8 KiB of LDS for array / run
// operands; stack: 8 KiB per saved value, n_saved of them; win: 8 KiB the caller does not need before the program has ended (F).
// Every branch below is block-uniform.
//
// An operand hangs off a chain of five dependent loads (program word -> leaf -> the shard's row -> descriptor -> payload), none of
// which depends on X.  One operand after the other, that chain is the whole run time (a predicate over 64 planes: 70 operands).  So
// the program is taken in windows of 256 instructions: thread t resolves the descriptor of instruction pc0 + t — the first four
// loads of all 256 chains side by side — into `win`, and the loop over the window reads descriptors from LDS and keeps the bitmap
// payloads of the next kExprBlockAhead instructions in flight while it applies the current one.
constexpr int kExprBlockAhead = 1;  // 2: 18 vector registers spilled under the kernel's cap of 64, 3: 82
constexpr uint32_t kExprWindow = 256;
__device__ __forceinline__ void expr_run_block(const ExprLeaf* __restrict__ leaves, const uint32_t* __restrict__ prog, uint32_t prog_len, uint64_t shard,
                                               uint32_t slot, int t, int lane, int wv, uint32_t n_saved, u64* T, u64* stack, u64* win, u64 (&X)[4]) {
  constexpr int kAhead = kExprBlockAhead;
  u64 M[4] = {0, 0, 0, 0};
  u64 W[kAhead][4];
  X[0] = X[1] = X[2] = X[3] = 0;
  uint32_t sp = 0;
  ulonglong2* T2 = reinterpret_cast<ulonglong2*>(T);
  uint32_t* T32 = reinterpret_cast<uint32_t*>(T);
  Slot* wdesc = reinterpret_cast<Slot*>(win);                                 // [kExprWindow] 4 KiB
  const uint8_t** warena = reinterpret_cast<const uint8_t**>(win + kWords / 2);  // [kExprWindow] 2 KiB
  // instruction i of the window: its descriptor in scalar registers (tn = 0: no operand, or a nil container)
  auto window_desc = [&](uint32_t i, Slot& s, const uint8_t*& arena) {
    const Slot v = wdesc[i];
    s.off = ((u64)__builtin_amdgcn_readfirstlane((uint32_t)(v.off >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v.off);
    s.len = __builtin_amdgcn_readfirstlane(v.len);
    s.tn = __builtin_amdgcn_readfirstlane(v.tn);
    const u64 a = reinterpret_cast<u64>(warena[i]);
    arena = reinterpret_cast<const uint8_t*>(((u64)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a));
  };
  auto is_partial_bitmap = [](const Slot& s) { return slot_n(s) != 0 && slot_n(s) != 65536u && slot_type(s) == kTypeBitmap; };
  // the payload of instruction i of the window, if it is a bitmap that has to be read: every thread its own 32 bytes
  auto issue = [&](uint32_t i, uint32_t lim, u64 (&w)[4]) {
    if (i >= lim) return;
    Slot s;
    const uint8_t* arena;
    window_desc(i, s, arena);
    if (!is_partial_bitmap(s)) return;
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(arena + s.off);
    const ulonglong2 v0 = ld_stream(&q[t]), v1 = ld_stream(&q[256 + t]);
    w[0] = v0.x, w[1] = v0.y, w[2] = v1.x, w[3] = v1.y;
  };
  // operand words of a container that is not a bitmap to be read: nil, full, or an array / run decoded through T
  auto operand = [&](const Slot& s, const uint8_t* __restrict__ arena, u64 (&w)[4]) {
    const uint32_t n = slot_n(s), type = slot_type(s);
    if (n == 0) {
      w[0] = w[1] = w[2] = w[3] = 0;
    } else if (n == 65536u) {
      w[0] = w[1] = w[2] = w[3] = ~0ull;
    } else {
      ulonglong2 z;
      z.x = z.y = 0;
      T2[t] = z;  // (the words this thread read last time: no barrier before)
      T2[256 + t] = z;
      __syncthreads();
      // the payload as 1 KiB chunks dealt to the four wavefronts, whatever its size (an array of 65535 values: 128 chunks); lanes
      // past the end re-read its first 16 bytes, scatter_chunk masks them by len
      const uint32_t bytes = payload_bytes(type, s.len), nch = (bytes + 1023u) >> 10;
      const uint8_t* p = arena + s.off;
      for (uint32_t j = (uint32_t)wv; j < nch; j += 4) {
        const uint32_t b0 = j * 1024u + (uint32_t)lane * 16u;
        const uint4 v = *reinterpret_cast<const uint4*>(p + (b0 < bytes ? b0 : 0u));
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
        scatter_chunk<1>(d, type, s.len, j, lane, T32);
      }
      __syncthreads();
      const ulonglong2 v0 = T2[t], v1 = T2[256 + t];
      w[0] = v0.x, w[1] = v0.y, w[2] = v1.x, w[3] = v1.y;
    }
  };
  for (uint32_t pc0 = 0; pc0 < prog_len; pc0 += kExprWindow) {
    const uint32_t lim = min(kExprWindow, prog_len - pc0);
    if (pc0) __syncthreads();  // the previous window is read to its end
    {
      Slot s;
      s.off = 0;
      s.len = 0;
      s.tn = 0;
      const uint8_t* arena = nullptr;
      if ((uint32_t)t < lim) {
        const uint32_t ins = prog[pc0 + t];
        if ((ins >> 24) <= fbk_expr::kMorXAn) {
          const ExprLeaf& lf = leaves[(ins >> fbk_expr::kLeafShift) & 0xFFFu];
          const uint64_t row = (uint64_t)lf.rows[shard] + (ins & fbk_expr::kRowMask);
          s = lf.slots[row * kSlots + slot];
          arena = lf.arena;
        }
      }
      wdesc[t] = s;
      warena[t] = arena;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kAhead; ++u) issue((uint32_t)u, lim, W[u]);
    for (uint32_t i0 = 0; i0 < lim; i0 += kAhead) {
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const uint32_t i = i0 + (uint32_t)u;
        if (i < lim) {
          const uint32_t op = prog[pc0 + i] >> 24;
          if (op <= fbk_expr::kMorXAn) {
            Slot s;
            const uint8_t* ar;
            window_desc(i, s, ar);
            u64 w[4];
            if (is_partial_bitmap(s)) {
#pragma unroll
              for (int q = 0; q < 4; ++q) w[q] = W[u][q];
            } else {
              operand(s, ar, w);
            }
            if (op <= fbk_expr::kAndnRev) {
              expr_apply_x(op, X, [&](int q) { return w[q]; });
            } else {
              const u64 inv = op == fbk_expr::kMorXAn ? ~0ull : 0ull;
#pragma unroll
              for (int q = 0; q < 4; ++q) M[q] |= X[q] & (w[q] ^ inv);
            }
          } else if (op == fbk_expr::kMZero) {
            M[0] = M[1] = M[2] = M[3] = 0;
          } else if (op == fbk_expr::kXFromM) {
#pragma unroll
            for (int q = 0; q < 4; ++q) X[q] = M[q];
          } else if (op == fbk_expr::kZeroX) {
            X[0] = X[1] = X[2] = X[3] = 0;
          } else if (op == fbk_expr::kPush && sp < n_saved) {  // (n_saved: what the launch sized the stack for)
            ulonglong2* sv = reinterpret_cast<ulonglong2*>(stack + (size_t)sp * kWords);
            ulonglong2 v0, v1;
            v0.x = X[0], v0.y = X[1], v1.x = X[2], v1.y = X[3];
            sv[t] = v0;
            sv[256 + t] = v1;
            ++sp;
          } else if (op > fbk_expr::kPop && sp) {
            --sp;
            const ulonglong2* sv = reinterpret_cast<const ulonglong2*>(stack + (size_t)sp * kWords);
            const ulonglong2 v0 = sv[t], v1 = sv[256 + t];
            const u64 w[4] = {v0.x, v0.y, v1.x, v1.y};
            expr_apply_x(op - fbk_expr::kPop, X, [&](int q) { return w[q]; });
          }
          issue(i + kAhead, lim, W[u]);  // this register set is free again
        }
      }
    }
  }
  __syncthreads();  // the last window is read to its end: `win` is the caller's again
}

// shard0: the first shard of this pass — the leaves' row lists are indexed by the call's shard, rowsA / out_shard / d_src by
// the shard of the pass.  d_src may be NULL.
__global__ void __launch_bounds__(256, 8) k_expr_rows_vs_filter(const ExprLeaf* __restrict__ leaves, const uint32_t* __restrict__ prog, uint32_t prog_len,
                                                               uint32_t n_saved, uint32_t shard0, const Slot* __restrict__ slotsA,
                                                               const uint8_t* __restrict__ arenaA, const uint32_t* __restrict__ rowsA, uint32_t nA,
                                                               uint32_t n_shards, uint32_t rows_per_block, u64* __restrict__ out_shard,
                                                               u64* __restrict__ d_src) {
  // F | rank | T in one piece: rank[kWords] is T's first dword, the rank scan's wave totals the four after it
  __shared__ u64 s_lds[kWords + kWords / 2 + kWords];
  extern __shared__ u64 expr_rows_stack[];  // 8 KiB per saved value
  u64* F = s_lds;
  uint32_t* rank = reinterpret_cast<uint32_t*>(s_lds + kWords);
  u64* T = s_lds + kWords + kWords / 2;
  uint32_t* s_part = reinterpret_cast<uint32_t*>(T) + 4;
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t chunks = (nA + rows_per_block - 1) / rows_per_block;
  uint32_t b = xcd_swizzle(blockIdx.x, gridDim.x);  // (shard, slot, chunk of rows): a shard's blocks on one XCD
  const uint32_t chunk = b % chunks;
  b /= chunks;
  const uint32_t slot = b & 15u;
  const uint32_t shard = b >> 4;
  if (shard >= n_shards) return;
  // the descriptors of the block's first 64 rows: a chain of dependent loads that starts before the tree's
  const uint32_t i_begin = chunk * rows_per_block, i_end = min(nA, i_begin + rows_per_block);
  const uint32_t* arow = rowsA + (uint64_t)shard * nA;
  Slot first_mine;
  first_mine.off = 0;
  first_mine.len = 0;
  first_mine.tn = 0;
  if (i_begin + lane < i_end) first_mine = slotsA[(uint64_t)arow[i_begin + lane] * kSlots + slot];
  {
    u64 X[4];
    expr_run_block(leaves, prog, prog_len, (uint64_t)shard0 + shard, slot, t, lane, wv, n_saved, T, expr_rows_stack, F, X);
    ulonglong2 v0, v1;
    v0.x = X[0], v0.y = X[1], v1.x = X[2], v1.y = X[3];
    reinterpret_cast<ulonglong2*>(F)[t] = v0;
    reinterpret_cast<ulonglong2*>(F)[256 + t] = v1;
  }
  __syncthreads();  // F is complete, and nobody reads T any more
  rows_filter_rank(F, rank, s_part, t, lane, wv);
  const uint32_t nf = __builtin_amdgcn_readfirstlane(rank[kWords]);
  if (nf == 0) return;  // nothing can intersect at this slot (block-uniform)
  if (chunk == 0 && t == 0 && d_src) atomicAdd(&d_src[shard], (u64)nf);
  // (the lane id from v_mbcnt again instead of keeping threadIdx.x & 63 alive across the tree: with the old one the register
  // allocator ends two registers over the 64 of 8 wavefronts per SIMD and spills an address of the streaming phase)
  const int lane_s = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  rows_stream_past_filter(F, rank, nf == 65536u, nf, slotsA, arenaA, arow, (const Slot*)nullptr, nA, slot, shard, i_begin, i_end, first_mine, lane_s, wv,
                          out_shard);
}

}  // namespace fbk
