// fbk_moments_plan.h — host rules of fbk_bsi_moments (HIP-free: compiled into the library and into the stand-alone check of the
// tests, tests/cpp/moments_plan_check.cpp).  What fbk_moments_api.inc decides before it launches and after it reads back, and
// the constants k_bsi_moments (fbk_moments.hip.h) is built on, written once:
//   chunks_of()          the signed 7-bit chunks of a field of a given depth;
//   rows()               the row of the byte matrix M each chunk and the 0/1 mask take (G = M · Mᵀ is at most 21 x 21 of 32 x 32);
//   packing()            how many column blocks share the 32-row tile when the call has few rows;
//   kMaxColumnsPerI32    how many columns an i32 accumulator may cover before it is flushed into an i64;
//   densify_chunk()      the shards per pass when an operand goes through DenseOperands (fbk_dense_policy.h's even_chunk);
//   fold()               the i64 chunk-pair matrix -> n and the five sums, modulo 2^128.
#pragma once

#include <algorithm>
#include <cstdint>

#include "fbk_dense_policy.h"

namespace fbk_moments_plan {

constexpr uint32_t kChunkBits = 7;   // magnitude bits per i8 chunk (fbk_matrix_sum.hip.h's split: chunk bytes in [-127, 127])
constexpr uint32_t kTile = 32;       // G is one 32 x 32 tile of v_mfma_i32_32x32x32_i8
constexpr uint32_t kCells = kTile * kTile;
constexpr uint32_t kMaxDepth = 64;
constexpr uint32_t kMaxShards = 1u << 28;  // 2^28 shards x 2^20 columns x 127^2 < 2^62: a cell's sum over every shard fits an i64

inline constexpr uint32_t chunks_of(uint32_t depth) { return (depth + kChunkBits - 1) / kChunkBits; }

// Rows of M: chunk m of x is row m, chunk m of y is row cx + m, the mask E is row cx + cy; the rows from n on are zero.
struct Rows {
  uint32_t cx, cy, mask, n;
};
inline constexpr Rows rows(uint32_t depth_x, uint32_t depth_y) {
  return {chunks_of(depth_x), chunks_of(depth_y), chunks_of(depth_x) + chunks_of(depth_y), chunks_of(depth_x) + chunks_of(depth_y) + 1};
}
static_assert(rows(kMaxDepth, kMaxDepth).n == 21 && rows(kMaxDepth, kMaxDepth).n <= kTile, "two fields of depth 64 and the mask fit one tile");

// Spare rows: the expansion's vector instructions bound the kernel and a lane of a padding row spends as many as any other, so a
// call with at most 16 (8) rows of M puts 2 (4) column blocks into the tile, each in 32 / P rows; the P diagonal blocks of G are
// then partial results and the rest of G is ignored.  Measured (docs/history/DESIGN_moments_measurements.md, 1024 shards, the
// kernels' time, profiles/bsi_moments_unpacked_* against profiles/bsi_moments_1024sh_*): depths (20, 20), 7 rows, 6.02 ms
// unpacked -> 1.77 ms with P = 4; (32, 32), 11 rows, 6.15 -> 3.50 ms with P = 2.
inline constexpr uint32_t packing(uint32_t n_rows) { return n_rows <= kTile / 4 ? 4 : n_rows <= kTile / 2 ? 2 : 1; }
static_assert(packing(8) == 4 && packing(9) == 2 && packing(16) == 2 && packing(17) == 1 && packing(21) == 1, "");

// A product of two chunk bytes is at most 127^2 = 16 129 in magnitude, so an i32 accumulator cell is exact for this many columns
// (133 143); the kernel flushes far more often (fbk::kMomFlushColumns, checked against this there).
constexpr uint64_t kMaxByteProduct = 127ull * 127ull;
constexpr uint64_t kMaxColumnsPerI32 = ((1ull << 31) - 1) / kMaxByteProduct;
static_assert((1ull << 17) <= kMaxColumnsPerI32 && (1ull << 18) > kMaxColumnsPerI32, "2^17 columns are safe, 2^18 are not");

// Rows densified per shard: depth + 2 of a field whose batch is not dense, 1 of such a filter.  has_y == false: the one-field form.
inline uint64_t densified_rows(bool x_encoded, uint32_t depth_x, bool has_y, bool y_encoded, uint32_t depth_y, bool has_f, bool f_encoded) {
  return (x_encoded ? depth_x + 2 : 0) + (has_y && y_encoded ? depth_y + 2 : 0) + (has_f && f_encoded ? 1 : 0);
}
// Shards per pass: at most 2^30 / (2^17 * R) of them, dealt evenly over the fewest passes.
constexpr uint64_t kScratch = 1ull << 30;
inline uint32_t densify_chunk(uint32_t n_shards, uint64_t densified) { return fbk::even_chunk(n_shards, kScratch, fbk::kDenseRowBytes * densified); }

// n and the five sums modulo 2^128 (two's complement)
struct Sums {
  uint64_t n;
  unsigned __int128 x, y, xx, yy, xy;
};

// S: the kCells i64 cells of G summed over every column, row-major.  v = Σ_m 2^(7m) chunk_m, hence
//   Σ a = Σ_m S[mask][a_m] << 7m        Σ a·b = Σ_m Σ_m' S[a_m][b_m'] << 7(m + m')
// every term sign-extended to 128 bits and shifted and added with wrap-around (the largest shift is 7 * 18 = 126).
inline Sums fold(const int64_t* S, uint32_t depth_x, uint32_t depth_y) {
  typedef unsigned __int128 u128;
  const Rows r = rows(depth_x, depth_y);
  auto cell = [&](uint32_t i, uint32_t j) { return u128(__int128(S[i * kTile + j])); };
  auto linear = [&](uint32_t row0, uint32_t n) {
    u128 s = 0;
    for (uint32_t m = 0; m < n; ++m) s += cell(r.mask, row0 + m) << (kChunkBits * m);
    return s;
  };
  auto bilinear = [&](uint32_t a0, uint32_t na, uint32_t b0, uint32_t nb) {
    u128 s = 0;
    for (uint32_t m = 0; m < na; ++m)
      for (uint32_t k = 0; k < nb; ++k) s += cell(a0 + m, b0 + k) << (kChunkBits * (m + k));
    return s;
  };
  Sums out;
  out.n = uint64_t(S[r.mask * kTile + r.mask]);
  out.x = linear(0, r.cx);
  out.y = linear(r.cx, r.cy);
  out.xx = bilinear(0, r.cx, 0, r.cx);
  out.yy = bilinear(r.cx, r.cy, r.cx, r.cy);
  out.xy = bilinear(0, r.cx, r.cx, r.cy);
  return out;
}

}  // namespace fbk_moments_plan
