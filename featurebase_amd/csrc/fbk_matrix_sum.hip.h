// fbk_matrix_sum.hip.h — GroupBy with aggregate=Sum(field=v) (groupByIterator.Next -> executeSumCountShard per group,
// executor.go:8880-8913, 2155-2216) as ONE contraction per shard on the matrix cores, for DENSE operands:
//
//   sum[i][j]   = Σ_c A_i(c) · B_j(c) · F(c) · E(c) · v(c)        (E = exists row, v = signed BSI value of column c)
//   count[i][j] = Σ_c A_i(c) · B_j(c) · F(c) · E(c)
//
// The magnitude is split into 7-bit chunks, chunk m = bits 7m .. 7m+6, and each chunk carries the sign: an i8 in [-127, 127].
// v = Σ_m 2^(7m) · chunk_m, so per chunk the sum is an i8 x i8 matrix product (v_mfma_i32_32x32x32_i8):
//   A operand: the bit A_i ∩ F ∩ E of column c as a 0/1 byte;
//   B operand: B_j(c) ? chunk_m(c) : 0 — one per chunk — and B_j(c) as a 0/1 byte for the count.
// Per shard an accumulator holds at most 2^20 x 127 (exact in i32); it is flushed as (u64)(i64)acc << 7m with wrapping adds,
// which is fbk_bsi_sum's arithmetic modulo 2^64 whatever the order of the adds.  Bits of the sign or a plane outside E
// contribute nothing: E is on the A side.
//
// Two kernels:
//   k_msum_chunks  (HBM-bound) the chunk bytes of every column, from the sign and magnitude planes, into a scratch area in
//                  the order the matrix kernel consumes them: the chunk transpose is the same for every B row, done once;
//   k_msum_mfma    one block per (shard, slot group, 32 A rows, 32 B rows); its four waves split the row bytes, every lane
//                  expands its bits into bytes ((x >> k) & 0x01010101: byte b = bit 8b + k of the dword) and masks the chunk
//                  bytes of the same columns with the B bits ((m << 8) - m turns 0/1 bytes into 0x00 / 0xFF).
// Chunk record layout (per shard and chunk: 1 MiB = one byte per column): columns 128 sp .. 128 sp + 127 form record sp of
// 128 bytes, [k][d][b] = column 128 sp + 32 d + 8 b + k, i.e. exactly the bytes the expansion of dword d at step k produces.
#pragma once
#include "fbk_kernels.hip.h"

namespace fbk {

constexpr uint32_t kMsumChunkBits = 7;     // magnitude bits per i8 chunk
constexpr uint32_t kMsumPerLaunch = 3;     // chunks per matrix launch (more: further launches over the same rows)
constexpr uint64_t kMsumChunkBytes = 1ull << 20;  // chunk bytes of one shard and one chunk (2^20 columns)

typedef int ms_v4i __attribute__((ext_vector_type(4)));
typedef int ms_v16i __attribute__((ext_vector_type(16)));

// One thread per (shard, dword of a row): 32 columns.  bsi rows: base[shard] + 1 = sign, + 2 + p = magnitude plane p.
// out: [n_shards][n_chunks] records of kMsumChunkBytes.
__global__ void __launch_bounds__(256) k_msum_chunks(const uint8_t* __restrict__ arena, const uint32_t* __restrict__ base, uint32_t n_shards,
                                                     uint32_t depth, uint32_t n_chunks, uint8_t* __restrict__ out) {
  constexpr uint32_t kDwords = kSlots * 2048;  // dwords of a 128 KiB row
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t shard = uint32_t(gid / kDwords), w = uint32_t(gid % kDwords);
  if (shard >= n_shards) return;
  const uint64_t rowBytes = (uint64_t)kSlots * 8192;
  const uint8_t* r0 = arena + (uint64_t)base[shard] * rowBytes + (uint64_t)w * 4;
  constexpr uint32_t M = 0x01010101u;
  const uint32_t sign = *reinterpret_cast<const uint32_t*>(r0 + rowBytes);
  uint8_t* o = out + (uint64_t)shard * n_chunks * kMsumChunkBytes + (w >> 2) * 128u + (w & 3) * 4u;
  for (uint32_t m = 0; m < n_chunks; ++m) {
    uint32_t pl[kMsumChunkBits];
#pragma unroll
    for (uint32_t q = 0; q < kMsumChunkBits; ++q) {
      const uint32_t p = m * kMsumChunkBits + q;
      pl[q] = p < depth ? *reinterpret_cast<const uint32_t*>(r0 + (uint64_t)(2 + p) * rowBytes) : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      uint32_t x = 0;
#pragma unroll
      for (uint32_t q = 0; q < kMsumChunkBits; ++q) x |= ((pl[q] >> k) & M) << q;  // bytes in [0, 127]
      const uint32_t neg = (0x80808080u - x) ^ 0x80808080u;                           // -x per byte (no borrow: x <= 0x7F)
      const uint32_t s = (sign >> k) & M;
      const uint32_t smask = (s << 8) - s;                                            // 0xFF where the sign bit is set
      *reinterpret_cast<uint32_t*>(o + (uint64_t)m * kMsumChunkBytes + k * 16u) = (x & ~smask) | (neg & smask);
    }
  }
}

// out_shard: [n_shards][2][nA * nB] — the sums (u64, wrapping) then the counts; added to with atomics (zeroed by the caller).
// arenaB == nullptr: the one-field form (nB == 1, every B bit set).  chunks: the chunk records of the first of the CC chunks
// of this launch, record stride n_chunks * kMsumChunkBytes per shard; shift0 = 7 * (index of that chunk).  count: this launch
// also counts (the first launch over the rows).
template <int CC, bool HAS_F>
__global__ void __launch_bounds__(256) k_msum_mfma(const uint8_t* __restrict__ arenaA, const uint32_t* __restrict__ rowsA, uint32_t nA,
                                                   const uint8_t* __restrict__ arenaB, const uint32_t* __restrict__ rowsB, uint32_t nB,
                                                   const uint8_t* __restrict__ arenaF, const uint32_t* __restrict__ rowsF,
                                                   const uint8_t* __restrict__ arenaE, const uint32_t* __restrict__ rowsE,
                                                   const uint8_t* __restrict__ chunks, uint32_t n_chunks, uint32_t shift0, uint32_t count,
                                                   uint32_t n_shards, uint32_t spb, u64* __restrict__ out_shard) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t agroups = (nA + 31) / 32, btiles = (nB + 31) / 32, sgroups = kSlots / spb;
  uint32_t b = blockIdx.x;
  const uint32_t bt = b % btiles;
  b /= btiles;
  const uint32_t ag = b % agroups;
  b /= agroups;
  const uint32_t sg = b % sgroups;
  const uint32_t shard = b / sgroups;
  if (shard >= n_shards) return;
  const uint32_t i0 = ag * 32, j0 = bt * 32;
  const uint64_t rowBytes = (uint64_t)kSlots * 8192;
  const uint32_t r = lane & 31, g = lane >> 5;
  // lane (r, g) holds bytes 64 g .. 64 g + 63 of every 128-byte piece of row r (rows past the end re-read the last row: their
  // products are never written out); E and F are the same for every r
  const uint8_t* pa = arenaA + (uint64_t)rowsA[(uint64_t)shard * nA + min(i0 + r, nA - 1)] * rowBytes + g * 64;
  const uint8_t* pb = arenaB ? arenaB + (uint64_t)rowsB[(uint64_t)shard * nB + min(j0 + r, nB - 1)] * rowBytes + g * 64 : nullptr;
  const uint8_t* pe = arenaE + (uint64_t)rowsE[shard] * rowBytes + g * 64;
  const uint8_t* pf = HAS_F ? arenaF + (uint64_t)rowsF[shard] * rowBytes + g * 64 : nullptr;
  const uint8_t* pc = chunks + (uint64_t)shard * n_chunks * kMsumChunkBytes;

  ms_v16i accS[CC > 0 ? CC : 1], accC = ms_v16i{};
#pragma unroll
  for (int m = 0; m < (CC > 0 ? CC : 1); ++m) accS[m] = ms_v16i{};
  constexpr uint32_t M = 0x01010101u;
  const uint32_t p_end = (sg + 1) * spb * 64;  // 128-byte pieces of the shard row: 64 per slot
  for (uint32_t p = sg * spb * 64 + wv; p < p_end; p += 4) {
    const uint32_t off = p * 128;
    uint4 A[4], B[4], E[4], F[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      A[t] = *reinterpret_cast<const uint4*>(pa + off + 16 * t);
      B[t] = pb ? *reinterpret_cast<const uint4*>(pb + off + 16 * t) : make_uint4(~0u, ~0u, ~0u, ~0u);
      E[t] = *reinterpret_cast<const uint4*>(pe + off + 16 * t);
      if (HAS_F) F[t] = *reinterpret_cast<const uint4*>(pf + off + 16 * t);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint32_t a[4] = {A[t].x & E[t].x, A[t].y & E[t].y, A[t].z & E[t].z, A[t].w & E[t].w};
      if (HAS_F) {
        a[0] &= F[t].x;
        a[1] &= F[t].y;
        a[2] &= F[t].z;
        a[3] &= F[t].w;
      }
      const uint32_t bb[4] = {B[t].x, B[t].y, B[t].z, B[t].w};
      // the chunk record of these 128 columns (subpiece (off + 64 g + 16 t) / 16)
      const uint8_t* rec = pc + (uint64_t)((off + g * 64 + 16 * t) >> 4) * 128u;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ms_v4i oa, ob;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          oa[d] = (int)((a[d] >> k) & M);
          ob[d] = (int)((bb[d] >> k) & M);
        }
        if (count) accC = __builtin_amdgcn_mfma_i32_32x32x32_i8(oa, ob, accC, 0, 0, 0);
#pragma unroll
        for (int m = 0; m < CC; ++m) {
          const uint4 c = *reinterpret_cast<const uint4*>(rec + (uint64_t)m * kMsumChunkBytes + k * 16);
          const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
          ms_v4i oc;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const uint32_t mb = (uint32_t)ob[d];
            oc[d] = (int)(cw[d] & ((mb << 8) - mb));
          }
          accS[m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(oa, oc, accS[m], 0, 0, 0);
        }
      }
    }
  }
  // every wave adds its partial results (the four waves of a block and the slot groups of a shard meet in the atomics)
  const uint64_t width = (uint64_t)nA * nB;
  u64* os = out_shard + (uint64_t)shard * 2 * width;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const uint32_t i = i0 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5), j = j0 + (lane & 31);
    if (i < nA && j < nB) {
      u64 s = 0;
#pragma unroll
      for (int m = 0; m < CC; ++m) s += (u64)(long long)accS[m][q] << (shift0 + kMsumChunkBits * m);
      if (s) atomicAdd(&os[(uint64_t)i * nB + j], s);
      if (count && accC[q]) atomicAdd(&os[width + (uint64_t)i * nB + j], (u64)(uint32_t)accC[q]);
    }
  }
}

}  // namespace fbk
