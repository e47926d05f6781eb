// fbk_group_quantile_plan.h — host rules of fbk_count_matrix_quantiles (HIP-free: compiled into the library and into the stand-alone
// check of the tests, tests/cpp/gquant_plan_check.cpp).  What fbk_group_quantile_api.inc decides before it launches, written once:
//   kLdsDigitBits / kGlobalDigitBits  the radix digit of each kernel path (fbk_group_quantile.hip.h);
//   key_bits(), passes()              the bits of the key (fbk_select_plan.h's SortKey) and the passes over the planes;
//   lds_pairs_cap()                   the most histograms (groups x max(1, n_q)) the LDS path keeps in a block's 64 KiB;
//   scratch_bytes(), kScratchBound    the histograms in device memory and the most a call may ask for;
//   path()                            the path of a call from its shape and its flags (0: the flags / shape are an error);
//   densify_chunk()                   the shards per walk when an operand goes through DenseOperands (fbk_dense_policy.h's even_chunk).
#pragma once

#include <algorithm>
#include <cstdint>

#include "fbk_dense_policy.h"
#include "fbk_select_plan.h"

namespace fbk_gquant_plan {

constexpr uint32_t kAuto = 0, kLds = 1, kGlobal = 2;  // FBK_GQUANT_AUTO / _LDS / _GLOBAL (include/fbk.h)

// The digits.  A build may override them (-DFBK_GQUANT_LDS_DIGIT=11 ...): scripts/bench_groupby_quantiles.py times such builds
// against each other through FBK_LIB_PATH.
#ifndef FBK_GQUANT_LDS_DIGIT
#define FBK_GQUANT_LDS_DIGIT 8
#endif
#ifndef FBK_GQUANT_GLOBAL_DIGIT
#define FBK_GQUANT_GLOBAL_DIGIT 8
#endif
// Fixed from the sweeps of scripts/bench_groupby_quantiles.py on an 8-bit and an 11-bit build (profiles/groupby_quantiles_d8_paths.json,
// groupby_quantiles_d11_paths.json; docs/history/DESIGN_group_quantiles_measurements.md), 128 shards of mutex-like rows, medians:
//  LDS     11 bits halve the passes (1 group, depth 20: 2.35 ms against 3.54) but hold 8 (group, request) pairs, 8 bits 64; from 9 to
//          64 pairs the 8-bit LDS path (2.0 .. 5.4 ms) is ahead of the GLOBAL path at either digit (6.0 .. 19.8 ms).  So 8.
//  GLOBAL  above 64 pairs, depth 20: 11 bits ahead by 7 .. 38 % (1024 groups: 7.6 ms against 10.5); depth 8: 8 bits ahead up to
//          2.5 x at 96 .. 384 pairs (192 pairs: 6.7 ms against 16.9), 11 bits ahead 1.3 .. 1.5 x from 256 groups on.  Neither wins
//          throughout, and 11 bits cost 8 x the scratch (2^16 pairs a call instead of 2^19).  So 8.
constexpr uint32_t kLdsDigitBits = FBK_GQUANT_LDS_DIGIT;
constexpr uint32_t kGlobalDigitBits = FBK_GQUANT_GLOBAL_DIGIT;
// 8 at least: k_quant_hist_sum adds the LDS path's partials 256 bins a block, k_gquant_resolve gives every lane bins / 64 of them
static_assert(kLdsDigitBits >= 8 && kLdsDigitBits <= 12 && kGlobalDigitBits >= 8 && kGlobalDigitBits <= 12, "");

inline constexpr uint32_t digit_bits(uint32_t path) { return path == kLds ? kLdsDigitBits : kGlobalDigitBits; }
using fbk::key_bits, fbk::passes;  // fbk_select_plan.h's key: bit_depth + 1 bits up to depth 62, else 64; ceil(key bits / digit) passes
// Pass p takes the key's bits [pass_low(p), pass_low(p) + pass_width(p)): whole digits from the top, the SHORT digit last.  A short
// first digit would send every column of a group to a handful of counters; in the last pass only the columns that still match a
// request's prefix add at all.
inline constexpr uint32_t pass_low(uint32_t bit_depth, uint32_t digit, uint32_t p) {
  const uint32_t hi = key_bits(bit_depth) - digit * p;
  return hi > digit ? hi - digit : 0;
}
inline constexpr uint32_t pass_width(uint32_t bit_depth, uint32_t digit, uint32_t p) { return key_bits(bit_depth) - digit * p - pass_low(bit_depth, digit, p); }

// The LDS path: 32-bit counters of every (group, request) pair in a block's 64 KiB (k_quant_hist's budget)
constexpr uint32_t kLdsBytes = 64u << 10;
inline constexpr uint32_t lds_pairs_cap() { return kLdsBytes / (4u << kLdsDigitBits); }
constexpr uint32_t kLdsBlocks = 1024;  // most blocks of an LDS launch; their partials: kLdsBlocks * kLdsBytes = 2^26 bytes at most

// Histograms in device memory: 64-bit counters, one histogram per (group, request) pair (pass 0 uses the first one of each group)
constexpr uint64_t kScratchBound = 1ull << 30;
inline constexpr uint64_t pairs_of(uint64_t n_a, uint64_t n_b, uint32_t n_q) { return n_a * n_b * std::max<uint32_t>(1, n_q); }
inline constexpr uint64_t scratch_bytes(uint64_t n_a, uint64_t n_b, uint32_t n_q, uint32_t digit) { return pairs_of(n_a, n_b, n_q) * (8ull << digit); }

// AUTO takes the LDS path up to this many pairs: the crossover of the same sweep (profiles/groupby_quantiles_d8_paths.json,
// "kAutoLdsPairs_from_sweep").  The pinned LDS path was ahead of the pinned GLOBAL path in every swept row it takes, 1 .. 64 pairs at
// depths 8 and 20 with 1 and 3 requests (closest: 48 pairs, depth 20, 5.2 ms against 7.8), so the rule is the LDS path's cap.
#ifndef FBK_GQUANT_AUTO_PAIRS
#define FBK_GQUANT_AUTO_PAIRS 64
#endif
constexpr uint32_t kAutoLdsPairs = FBK_GQUANT_AUTO_PAIRS;
static_assert(kAutoLdsPairs <= lds_pairs_cap(), "");

// kLds, kGlobal, or 0: unknown flags, or the LDS path pinned above its cap
inline constexpr uint32_t path(uint64_t n_a, uint64_t n_b, uint32_t n_q, uint32_t flags) {
  const uint64_t pairs = pairs_of(n_a, n_b, n_q);
  return flags == kAuto     ? (pairs <= kAutoLdsPairs ? kLds : kGlobal)
         : flags == kLds    ? (pairs <= lds_pairs_cap() ? kLds : 0u)
         : flags == kGlobal ? kGlobal
                            : 0u;
}

// Shards per walk: at most 2^30 / (2^17 * R) of them (R = the rows densified per shard), dealt evenly over the fewest walks.
constexpr uint64_t kDensifyScratch = 1ull << 30;
inline uint32_t densify_chunk(uint32_t n_shards, uint64_t densified) { return fbk::even_chunk(n_shards, kDensifyScratch, fbk::kDenseRowBytes * densified); }

// SQL PERCENTILE_DISC(num / den) over N >= 1 values: the ascending rank max(1, ceil(N * num / den)) - 1.  num <= den <= 2^20 and
// N <= 2^40 (2^20 shards of 2^20 columns) keep N * num + den within 2^61.
constexpr uint32_t kMaxDen = 1u << 20, kMaxRequests = 16;
inline constexpr uint64_t disc_rank(uint64_t N, uint32_t num, uint32_t den) {
  const uint64_t c = (N * num + den - 1) / den;
  return (c > 1 ? c : 1) - 1;
}

}  // namespace fbk_gquant_plan
