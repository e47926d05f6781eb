// fbk_matrix_cube.hip.h — GroupBy over three fields (groupByIterator.Next with three levels, executor.go:8829-8835, 8861-8867,
// 8893) as ONE contraction per shard on the matrix cores, for DENSE operands:
//
//   cube[p][i][j] = Σ_c P_p(c) · A_i(c) · B_j(c) · F(c)
//
// k_cube_mfma is k_msum_mfma's loop (plain global loads, (x >> k) & 0x01010101 turning bits into 0/1 bytes for
// v_mfma_i32_32x32x32_i8) with the third field on the A side: per 16 bytes of every row and per k the B operand is expanded ONCE,
// and for each of the block's PT rows of P the operand A & F & P_p is expanded and multiplied into its own accumulator.  The B
// expansion, the A / B / F loads and the loop are shared by PT planes of the cube; a plane costs one expansion and one matrix
// instruction per k.  A per-shard count is at most 2^20: exact in i32.
#pragma once
#include "fbk_kernels.hip.h"

namespace fbk {

typedef int mc_v4i __attribute__((ext_vector_type(4)));
typedef int mc_v16i __attribute__((ext_vector_type(16)));

// One block of four waves per (shard, slot group, 32 A rows, 32 B rows, PT P rows); block ids in that order, the P groups
// fastest.  out_shard: [n_shards][nP * nA * nB], added to with atomics (zeroed by the caller): the four waves of a block and the
// slot groups of a shard meet there.  PT * 16 accumulator registers; two blocks per CU (256 registers a wave).
template <int PT, bool HAS_F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_cube_mfma(const uint8_t* __restrict__ arenaP, const uint32_t* __restrict__ rowsP, uint32_t nP, const uint8_t* __restrict__ arenaA,
            const uint32_t* __restrict__ rowsA, uint32_t nA, const uint8_t* __restrict__ arenaB, const uint32_t* __restrict__ rowsB, uint32_t nB,
            const uint8_t* __restrict__ arenaF, const uint32_t* __restrict__ rowsF, uint32_t n_shards, uint32_t spb, u64* __restrict__ out_shard) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t pgroups = (nP + PT - 1) / PT, agroups = (nA + 31) / 32, btiles = (nB + 31) / 32, sgroups = kSlots / spb;
  uint32_t b = blockIdx.x;
  // The blocks of one (shard, slot group) read the same A, B and F rows.  Workgroups go to the 8 XCDs round robin and every XCD
  // has its own L2: with ids that differ by 8 those blocks share one and the rows come from HBM once (k_count_matrix_mfma).
  if (pgroups * agroups * btiles > 1 && (gridDim.x & 7u) == 0) b = (b & 7u) * (gridDim.x >> 3) + (b >> 3);
  const uint32_t pg = b % pgroups;
  b /= pgroups;
  const uint32_t bt = b % btiles;
  b /= btiles;
  const uint32_t ag = b % agroups;
  b /= agroups;
  const uint32_t sg = b % sgroups;
  const uint32_t shard = b / sgroups;
  if (shard >= n_shards) return;
  const uint32_t p0 = pg * PT, i0 = ag * 32, j0 = bt * 32;
  const uint64_t rowBytes = (uint64_t)kSlots * 8192;
  const uint32_t r = lane & 31, g = lane >> 5;
  // lane (r, g) holds bytes 64 g .. 64 g + 63 of every 128-byte piece of A row r and B row r; the P rows and F are the same for
  // every r (their row addresses are wave-uniform: scalar registers).  Rows past the end re-read the last row: their products are
  // never written out.
  const uint8_t* pa = arenaA + (uint64_t)rowsA[(uint64_t)shard * nA + min(i0 + r, nA - 1)] * rowBytes + g * 64;
  const uint8_t* pb = arenaB + (uint64_t)rowsB[(uint64_t)shard * nB + min(j0 + r, nB - 1)] * rowBytes + g * 64;
  const uint8_t* pf = HAS_F ? arenaF + (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(rowsF[shard]) * rowBytes : nullptr;
  const uint8_t* pp[PT];
#pragma unroll
  for (int q = 0; q < PT; ++q) pp[q] = arenaP + (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(rowsP[(uint64_t)shard * nP + min(p0 + q, nP - 1)]) * rowBytes;
  const uint32_t go = g * 64;

  mc_v16i acc[PT];
#pragma unroll
  for (int q = 0; q < PT; ++q) acc[q] = mc_v16i{};
  constexpr uint32_t M = 0x01010101u;
  // A step is 16 bytes of every row: one operand of the matrix instruction per k, 8 PT instructions.  The wave's steps: its
  // pieces (every fourth 128-byte piece of the block's slots: 64 per slot) times the four 16-byte parts of a piece.  The words of
  // the next step are loaded before this step's arithmetic (one step ahead is ~2000 cycles of matrix work: enough for HBM), so
  // the registers hold two steps of words and no more.
  const uint32_t n_steps = spb * 64, first = sg * spb * 64 + wv;
  uint4 wA = *reinterpret_cast<const uint4*>(pa + first * 128), wB = *reinterpret_cast<const uint4*>(pb + first * 128);
  uint4 wF = HAS_F ? *reinterpret_cast<const uint4*>(pf + (go + first * 128)) : make_uint4(0, 0, 0, 0);
  uint4 wP[PT];
#pragma unroll
  for (int q = 0; q < PT; ++q) wP[q] = *reinterpret_cast<const uint4*>(pp[q] + (go + first * 128));
#pragma unroll 1
  for (uint32_t s = 0; s < n_steps; ++s) {
    uint32_t af[4] = {wA.x, wA.y, wA.z, wA.w};
    if (HAS_F) af[0] &= wF.x, af[1] &= wF.y, af[2] &= wF.z, af[3] &= wF.w;
    const uint32_t bb[4] = {wB.x, wB.y, wB.z, wB.w};
    uint32_t a[PT][4];
#pragma unroll
    for (int q = 0; q < PT; ++q) a[q][0] = af[0] & wP[q].x, a[q][1] = af[1] & wP[q].y, a[q][2] = af[2] & wP[q].z, a[q][3] = af[3] & wP[q].w;
    const uint32_t sn = min(s + 1, n_steps - 1);  // (the last step loads its own words again)
    const uint32_t off = (first + 4 * (sn >> 2)) * 128 + 16 * (sn & 3);
    wA = *reinterpret_cast<const uint4*>(pa + off);
    wB = *reinterpret_cast<const uint4*>(pb + off);
    if (HAS_F) wF = *reinterpret_cast<const uint4*>(pf + (go + off));
#pragma unroll
    for (int q = 0; q < PT; ++q) wP[q] = *reinterpret_cast<const uint4*>(pp[q] + (go + off));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      mc_v4i ob;
#pragma unroll
      for (int d = 0; d < 4; ++d) ob[d] = (int)((bb[d] >> k) & M);
#pragma unroll
      for (int q = 0; q < PT; ++q) {
        mc_v4i oa;
#pragma unroll
        for (int d = 0; d < 4; ++d) oa[d] = (int)((a[q][d] >> k) & M);
        acc[q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(oa, ob, acc[q], 0, 0, 0);
        // at most two expanded operands ahead of their instructions: the scheduler would hoist the expansions of every P row and
        // every k (PT * 32 registers) and spill
        if (q & 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  const uint64_t plane = (uint64_t)nA * nB;
  u64* os = out_shard + (uint64_t)shard * nP * plane;
#pragma unroll
  for (int q = 0; q < PT; ++q) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint32_t i = i0 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), j = j0 + (lane & 31);
      if (p0 + q < nP && i < nA && j < nB && acc[q][e]) atomicAdd(&os[(p0 + q) * plane + (uint64_t)i * nB + j], (u64)(uint32_t)acc[q][e]);
    }
  }
}

}  // namespace fbk
