// fbk_compare_plan.h — host rules of fbk_bsi_compare (HIP-free: compiled into the library and into the stand-alone check of the
// tests, tests/cpp/compare_plan_check.cpp).  What fbk_compare_api.inc decides before it launches k_bsi_compare_slot
// (fbk_compare.hip.h), written once:
//   offset()       k = base_x - base_y, exact (a 65-bit signed number);
//   offset_bit()   bit i of k in two's complement, sign-extended for any i;
//   bitlen()       the bits of |k|;
//   general()      which instance a call takes;
//   steps()        the plane steps of that instance: W0 (sign-magnitude) or W (general);
//   combine()      the final combination of the lt / gt words for an operator.
#pragma once

#include <algorithm>
#include <cstdint>

namespace fbk_compare_plan {

constexpr uint32_t kMaxDepth = 64;
constexpr uint32_t kMaxShards = 1u << 27;  // one wavefront per (shard, slot): 16 * n_shards blocks must stay below 2^31
constexpr uint32_t kPathOffset = 0x100u;   // FBK_COMPARE_PATH_OFFSET (include/fbk.h)
constexpr int32_t kEQ = 1, kNEQ = 2, kLT = 3, kLTE = 4, kGT = 5, kGTE = 6;  // FBK_BSI_EQ .. FBK_BSI_GTE

// value_x op value_y  <=>  (sx ? -mx : mx) + k  op  (sy ? -my : my): only the difference of the bases matters.  Both bases are
// int64, so |k| <= 2^64 - 1: 65 bits of two's complement, held exactly by an __int128.
typedef __int128 Offset;
inline constexpr Offset offset(int64_t base_x, int64_t base_y) { return Offset(base_x) - Offset(base_y); }
inline constexpr uint32_t offset_bit(Offset k, uint32_t i) { return i >= 127 ? uint32_t(k < 0) : uint32_t((k >> i) & 1); }
inline constexpr uint64_t offset_low(Offset k) { return uint64_t(static_cast<unsigned __int128>(k)); }  // bits 0..63; every bit above is (k < 0)
inline constexpr uint32_t bitlen(Offset k) {
  unsigned __int128 a = k < 0 ? -static_cast<unsigned __int128>(k) : static_cast<unsigned __int128>(k);
  uint32_t n = 0;
  for (; a; a >>= 1) ++n;
  return n;
}

// The sign-magnitude instance compares magnitudes and signs directly, which is only the order of the values when nothing is added
// to either side.  FBK_COMPARE_PATH_OFFSET pins the general instance at k == 0 (tests, measurements).
inline constexpr bool general(Offset k, uint32_t flags) { return k != 0 || (flags & kPathOffset) != 0; }

// Plane steps.
//   sign-magnitude: W0 = max(depth_x, depth_y); a plane at or above a field's depth is zero.
//   general: both sides become W-bit two's complement numbers, X = ±mx + k and Y = ±my, compared as signed numbers.  Let
//     m = max(depth_x, depth_y, bitlen(|k|)).  Then mx, my, |k| <= 2^m - 1, so |X| <= mx + |k| <= 2^(m+1) - 2 and |Y| <= 2^m - 1:
//     both lie in [-2^(m+1), 2^(m+1) - 1], the range of an (m + 2)-bit two's complement number, so the streamed sums never
//     wrap and W = m + 2 is enough.  m + 1 bits are not: depth_x = 1, mx = 1, k = 1 gives X = 2, which wraps to -2 in two bits and
//     compares below Y = 0 (tests/test_bsi_compare_cpu.py plants that column).
inline constexpr uint32_t steps(uint32_t depth_x, uint32_t depth_y, Offset k, uint32_t flags) {
  const uint32_t w0 = std::max(depth_x, depth_y);
  return general(k, flags) ? std::max(w0, bitlen(k)) + 2 : w0;
}
static_assert(steps(64, 64, offset(INT64_MAX, INT64_MIN), 0) == 66 && steps(64, 3, 0, 0) == 64 && steps(0, 0, 0, kPathOffset) == 2, "");
static_assert(bitlen(offset(INT64_MIN, INT64_MAX)) == 64 && bitlen(offset(0, INT64_MIN)) == 64 && bitlen(0) == 0 && bitlen(-1) == 1, "");

// result = E & (((lt & take_lt) | (gt & take_gt)) ^ invert): lt / gt are the columns with value_x < / > value_y, E the participating ones
struct Combine {
  bool take_lt, take_gt, invert, ok;
};
inline constexpr Combine combine(int32_t op) {
  return op == kLT    ? Combine{true, false, false, true}
         : op == kGT  ? Combine{false, true, false, true}
         : op == kNEQ ? Combine{true, true, false, true}
         : op == kEQ  ? Combine{true, true, true, true}
         : op == kLTE ? Combine{false, true, true, true}
         : op == kGTE ? Combine{true, false, true, true}
                      : Combine{false, false, false, false};
}

}  // namespace fbk_compare_plan
