// fbk_moments.hip.h — fbk_bsi_moments: n, Σx, Σy, Σx², Σy², Σxy of two int (BSI) fields over the columns
// E = exists_x ∩ exists_y ∩ F, as ONE Gram matrix on the matrix cores, for DENSE operands (SQL VAR / CORR,
// sql3/planner/expressionagg.go aggregateVar / aggregateCorr).
//
// The magnitude of a value is split into signed 7-bit chunks as in fbk_matrix_sum.hip.h (chunk m = bits 7m .. 7m+6, an i8 in
// [-127, 127] that carries the sign, v = Σ_m 2^(7m) chunk_m).  M is the byte matrix with a row per chunk of x, a row per chunk
// of y and a row holding the 0/1 mask E, every byte zero outside E (fbk_moments_plan.h: rows()); G = M · Mᵀ
// (v_mfma_i32_32x32x32_i8, one 32 x 32 tile) then holds n, the chunk sums of Σx and Σy and the chunk-pair sums of the three
// products; the host folds them (fbk_moments_plan.h: fold()).  Everything is integer: exact whatever the grid and the order.
//
// k_bsi_moments: every plane is read from HBM once and the chunk bytes exist in registers only.
//   stage    a block takes stripes of 1024 columns (128 bytes of a row; P times that with packing, below).  Its 256 threads copy
//            the stripe of ALL the call's rows
//            (exists, sign, planes of x; the same of y; the filter: depth_x + depth_y + 5 at most) into LDS with coalesced
//            16-byte loads; the loads of stripe t + 1 are in flight while stripe t is expanded.  Two constant rows follow the
//            staged ones: all zero (a plane beyond the depth, the planes of a padding row) and all ones (a mask the call lacks).
//   expand   wave w takes columns 256 w .. 256 w + 255 of the stripe.  Lane l holds row l % 32 of M for the 128 columns of half
//            l / 32: it reads ITS seven planes, its field's sign and the three mask rows from LDS (ds_read_b128 each), ANDs the
//            planes and the sign with E once, and for k = 0 .. 7 builds 16 chunk bytes ((x >> k) & 0x01010101: byte b = bit
//            8 b + k of a dword, as k_msum_chunks) that are the A AND the B operand of one matrix instruction: for this
//            instruction both operands of a lane are row l % 32 at the same 16 values of k, and G = M · Mᵀ needs nothing else.
//            The mask row is a "field" whose plane 0 is the ones row and whose sign is the zero row.
//   sums     an i32 accumulator cell grows by at most 32 x 127² per instruction; it is flushed into an i64 register every
//            kMomFlushStripes stripes (2^14 columns per wave; 2^17 would still be exact).  The i64 sums stay in registers over
//            all the stripes of a block; at the end the four waves meet in LDS and the block writes ONE partial matrix, which
//            k_reduce_shards sums.  No global atomics in this kernel.
//   packing  the expansion's vector instructions bound the kernel, and a lane of a padding row spends as many as any other.  A call
//            with at most 16 (8) rows of M therefore runs with P = 2 (4): a stripe is P times as wide, and the lanes of rows
//            32 / P .. of the tile hold the SAME rows of M for the next column block(s).  The P diagonal blocks of the tile are
//            then P partial results, added together at the end; the rest of the tile is ignored.
#pragma once
#include "fbk_kernels.hip.h"
#include "fbk_matrix_sum.hip.h"
#include "fbk_moments_plan.h"

namespace fbk {

constexpr uint32_t kMomUnitStripes = 16;    // stripes a block takes at a time
#ifndef FBK_MOM_BLOCKS_PER_CU  // (a variant build with another value: scripts/bench_bsi_moments.py under FBK_LIB_PATH, runs alternating)
#define FBK_MOM_BLOCKS_PER_CU 3
#endif
// blocks per CU of the launch: what is resident (__launch_bounds__(256, 3): three waves per SIMD, <= 30 KB of LDS per block), so that no
// tail of blocks runs at a third of the occupancy with the same share of units as the others
constexpr uint32_t kMomBlocksPerCU = FBK_MOM_BLOCKS_PER_CU;
constexpr uint32_t kMomFlushStripes = 64;   // i32 -> i64 after this many stripes: a cell covers 256 columns per stripe
constexpr uint64_t kMomFlushColumns = uint64_t(kMomFlushStripes) * 256;
static_assert(kMomFlushColumns <= fbk_moments_plan::kMaxColumnsPerI32, "an i32 accumulator cell must be flushed while it is exact");

// What depends on the packing P (fbk_moments_plan.h: packing()): P column blocks share the tile, each in 32 / P rows of it.
template <int P>
struct MomShape {
  static constexpr uint32_t kTileRows = 32 / P;             // rows of M a call may have
  static constexpr uint32_t kStripeBytes = 128 * P;         // bytes of a row per stripe: 1024 P columns
  static constexpr uint32_t kStripesPerRow = kSlots * 8192 / kStripeBytes;
  static constexpr uint32_t kLdsRow = kStripeBytes + 16;    // a staged row in LDS: one 16-byte slot of padding
  // the rows a call with at most kTileRows rows of M stages: the planes of kTileRows - 1 chunks, two exists, two signs, the filter
  static constexpr uint32_t kMaxRows = (P == 1 ? 2 * fbk_moments_plan::kMaxDepth : fbk_moments_plan::kChunkBits * (kTileRows - 1)) + 5;
  static constexpr uint32_t kPieces = (kMaxRows * 8 * P + 255) / 256;  // 16-byte pieces a thread stages per stripe, at most
  static constexpr uint32_t kLdsBytes = (kMaxRows + 2) * kLdsRow;
  static_assert(fbk_moments_plan::kCells * 8 <= kLdsBytes, "the waves' final reduction reuses the staging area");
  static_assert(kLdsBytes <= 32768, "three blocks per CU");
};

typedef uint32_t mom_u4 __attribute__((ext_vector_type(4)));
typedef const mom_u4 __attribute__((address_space(1))) * mom_gptr;  // a pointer into global memory

struct MomentsArgs {
  const uint8_t* arena_x;  // x: rows base_x[s] + 0 exists, + 1 sign, + 2 + k plane k
  const uint32_t* base_x;
  const uint8_t* arena_y;  // nullptr: the one-field form
  const uint32_t* base_y;
  const uint8_t* arena_f;  // nullptr: no filter
  const uint32_t* rows_f;
  uint32_t depth_x, depth_y, n_shards;
};

// partial: [gridDim.x][kCells] i64, every cell written.  Units of kMomUnitStripes stripes are dealt to the blocks round robin.
// P = fbk_moments_plan::packing(rows of M): the call's rows of M number at most 32 / P.
template <int P>
__global__ void __launch_bounds__(256, 3) k_bsi_moments(MomentsArgs a, long long* __restrict__ partial) {
  typedef MomShape<P> Sh;
  constexpr uint32_t kLdsRow = Sh::kLdsRow, kPieces = Sh::kPieces, kParts = 8 * P;  // kParts: 16-byte pieces of a row per stripe
  __shared__ __attribute__((aligned(16))) uint8_t lds[Sh::kLdsBytes];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t r = lane & 31, g = lane >> 5;
  const uint32_t blk = r / Sh::kTileRows, rr = r % Sh::kTileRows;  // this lane: row rr of M for column block blk
  const uint64_t rowBytes = (uint64_t)kSlots * 8192;
  const uint32_t dx = a.depth_x, dy = a.depth_y;
  const bool hasY = a.arena_y != nullptr, hasF = a.arena_f != nullptr;
  const uint32_t rowsX = dx + 2, rowsXY = rowsX + (hasY ? dy + 2 : 0), nrows = rowsXY + (hasF ? 1 : 0);
  const uint32_t rowZero = nrows, rowOnes = nrows + 1;

  // the two constant rows (the first barrier of the loop orders them before any read)
  if (tid < 2 * kLdsRow / 16) {
    const uint32_t v = tid < kLdsRow / 16 ? 0u : ~0u;
    *reinterpret_cast<uint4*>(lds + rowZero * kLdsRow + tid * 16) = make_uint4(v, v, v, v);
  }

  // what this lane reads of a staged stripe: byte offsets of its seven planes, its sign and the three mask rows
  const fbk_moments_plan::Rows mr = fbk_moments_plan::rows(dx, hasY ? dy : 0);
  const uint32_t col = 32 * P * wv + 32 * blk + 16 * g;
  uint32_t offP[kMsumChunkBits], offS, offEx, offEy, offF;
  {
    const bool isX = rr < mr.cx, isY = !isX && rr < mr.mask, isM = rr == mr.mask;
    const uint32_t m = isX ? rr : rr - mr.cx, depth = isX ? dx : dy, row0 = isX ? 0 : rowsX;
#pragma unroll
    for (uint32_t q = 0; q < kMsumChunkBits; ++q) {
      const uint32_t p = m * kMsumChunkBits + q;
      uint32_t row = rowZero;
      if ((isX || isY) && p < depth) row = row0 + 2 + p;
      if (isM && q == 0) row = rowOnes;
      offP[q] = row * kLdsRow + col;
    }
    offS = ((isX || isY) ? row0 + 1 : rowZero) * kLdsRow + col;
    offEx = col;
    offEy = (hasY ? rowsX : rowOnes) * kLdsRow + col;
    offF = (hasF ? nrows - 1 : rowOnes) * kLdsRow + col;
  }

  const uint32_t unitsPerShard = Sh::kStripesPerRow / kMomUnitStripes;
  const uint64_t units = (uint64_t)a.n_shards * unitsPerShard;
  const uint64_t myUnits = units > blockIdx.x ? (units - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  const uint64_t T = myUnits * kMomUnitStripes;  // stripes of this block

  // stripe t of this block: the 16-byte pieces this thread stages (a piece past the call's rows re-reads the last row and is not written)
  mom_u4 st[kPieces];
  auto request = [&](uint64_t t) {
    const uint64_t unit = blockIdx.x + (t / kMomUnitStripes) * gridDim.x;
    const uint32_t shard = uint32_t(unit / unitsPerShard);
    const uint32_t stripe = uint32_t(unit % unitsPerShard) * kMomUnitStripes + uint32_t(t % kMomUnitStripes);
    // (addresses as integers: a select between them is one v_cndmask per half, never a branch around a load; the load goes through
    // a pointer of the global address space, so that it is a global_load and counts on vmcnt alone, not a flat_load)
    const uint64_t px = (uint64_t)a.arena_x + (uint64_t)a.base_x[shard] * rowBytes;
    const uint64_t py = hasY ? (uint64_t)a.arena_y + ((uint64_t)a.base_y[shard] - rowsX) * rowBytes : px;
    const uint64_t pf = hasF ? (uint64_t)a.arena_f + ((uint64_t)a.rows_f[shard] - (nrows - 1)) * rowBytes : px;
    const uint64_t at = (uint64_t)stripe * Sh::kStripeBytes;
#pragma unroll
    for (uint32_t i = 0; i < kPieces; ++i) {
      const uint32_t piece = tid + 256 * i;
      const uint32_t row = min(piece / kParts, nrows - 1), part = piece % kParts;
      const uint64_t p = (row < rowsX ? px : row < rowsXY ? py : pf) + (uint64_t)row * rowBytes + at + part * 16;
      st[i] = *reinterpret_cast<mom_gptr>(p);
    }
  };

  ms_v16i acc = ms_v16i{};
  long long sum[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) sum[q] = 0;
  constexpr uint32_t M = 0x01010101u;

  if (T) request(0);
  for (uint64_t t = 0; t < T; ++t) {
#pragma unroll
    for (uint32_t i = 0; i < kPieces; ++i) {
      const uint32_t piece = tid + 256 * i;
      if (piece < nrows * kParts) *reinterpret_cast<mom_u4*>(lds + (piece / kParts) * kLdsRow + (piece % kParts) * 16) = st[i];
    }
    __syncthreads();
    request(t + 1 < T ? t + 1 : t);  // in flight while this stripe is expanded (the last one is requested twice)

    const uint4 ex = *reinterpret_cast<const uint4*>(lds + offEx), ey = *reinterpret_cast<const uint4*>(lds + offEy), ff = *reinterpret_cast<const uint4*>(lds + offF);
    const uint32_t E[4] = {ex.x & ey.x & ff.x, ex.y & ey.y & ff.y, ex.z & ey.z & ff.z, ex.w & ey.w & ff.w};
    uint32_t pl[kMsumChunkBits][4], sg[4];
#pragma unroll
    for (uint32_t q = 0; q < kMsumChunkBits; ++q) {
      const uint4 v = *reinterpret_cast<const uint4*>(lds + offP[q]);
      pl[q][0] = v.x & E[0], pl[q][1] = v.y & E[1], pl[q][2] = v.z & E[2], pl[q][3] = v.w & E[3];
    }
    {
      const uint4 v = *reinterpret_cast<const uint4*>(lds + offS);
      sg[0] = v.x & E[0], sg[1] = v.y & E[1], sg[2] = v.z & E[2], sg[3] = v.w & E[3];
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      ms_v4i o;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        uint32_t x = 0;
#pragma unroll
        for (uint32_t q = 0; q < kMsumChunkBits; ++q) x |= ((pl[q][d] >> k) & M) << q;  // bytes in [0, 127]
        const uint32_t neg = (0x80808080u - x) ^ 0x80808080u;                              // -x per byte (no borrow: x <= 0x7F)
        const uint32_t s = (sg[d] >> k) & M;
        const uint32_t smask = (s << 8) - s;                                               // 0xFF where the sign bit is set
        o[d] = (int)((x & ~smask) | (neg & smask));
      }
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(o, o, acc, 0, 0, 0);
    }
    if ((t + 1) % kMomFlushStripes == 0 || t + 1 == T) {
#pragma unroll
      for (int q = 0; q < 16; ++q) sum[q] += acc[q];
      acc = ms_v16i{};
    }
    __syncthreads();  // every wave has read the stripe before the next one is written over it
  }

  // The four waves' sums meet in LDS (the staging area is free: the loop ended on a barrier), one partial matrix per block.  Of the
  // tile only the P diagonal blocks of 32 / P rows are results (products of rows of DIFFERENT column blocks mean nothing): block b's
  // cell (i, j) is added to cell (i, j) of the matrix.  Once per block: LDS atomics are fine here.
  unsigned long long* cells = reinterpret_cast<unsigned long long*>(lds);
  for (uint32_t c = tid; c < fbk_moments_plan::kCells; c += 256) cells[c] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const uint32_t i = (q & 3) + 8 * (q >> 2) + 4 * g;
    if (i / Sh::kTileRows == blk && sum[q]) atomicAdd(&cells[(i % Sh::kTileRows) * 32 + rr], (unsigned long long)sum[q]);
  }
  __syncthreads();
  long long* out = partial + (uint64_t)blockIdx.x * fbk_moments_plan::kCells;
  for (uint32_t c = tid; c < fbk_moments_plan::kCells; c += 256) out[c] = (long long)cells[c];
}

}  // namespace fbk
