// fbk_group_select_plan.h — host rules of the GroupBy selection stage (HIP-free: compiled into the library, into the C++ mirror
// include/fbk_executor.hpp and into the stand-alone check of the tests, tests/cpp/group_select_check.cpp).  Written once:
//   check()   the argument rules of a fbk_groupby_select (include/fbk.h);
//   passes()  satisfiesCondition (executor.go:3787-3901) on order-preserving uint64 values: what the kernels evaluate too;
//   key()     the order-preserving uint64 of a sort term (sign bit flipped for the int64 aggregate, complemented for desc);
//   window()  offset, then limit, on a list of `matched` records;
//   select()  the whole stage on the host: the small-input path of the library and the blocked path of the mirror.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/fbk.h"

namespace fbk_group_select {

// At or below this many cells the library downloads the totals and selects on the host.  MEASURED on an MI355X
// (scripts/bench_groupby_select.py, docs/history/DESIGN_groupby_select_measurements.md), not taken from topn_order_locked's 4096:
// the device stage costs about 45 us without a sort and about 200 us with one (8 histogram + 8 digit launches per term), the
// host path 8 or 16 bytes per cell over the bus plus the host's pass.  Without a sort the two meet at 2^16 cells (169 against
// 172 us); with a sort at 2^15 (limit 1000) to 2^17 (limit 10) cells; at 2^17 the device wins every case measured.
constexpr uint64_t kHostCells = 1ull << 16;
constexpr uint64_t kMaxCells = 1ull << 24;
constexpr uint64_t kSignBit = 1ull << 63;

// nullptr, or what is wrong with the selection; has_agg: the call has an aggregate
inline const char* check(const fbk_groupby_select* s, bool has_agg) {
  if (!s) return "NULL selection";
  if (s->flags & ~uint32_t(FBK_GROUPSEL_DEVICE | FBK_GROUPSEL_HOST)) return "unknown flag";
  if ((s->flags & FBK_GROUPSEL_DEVICE) && (s->flags & FBK_GROUPSEL_HOST)) return "both path flags";
  if (s->n_sort > 2) return "more than two sort terms";
  for (uint32_t t = 0; t < s->n_sort; ++t) {
    if (s->sort[t].subject != FBK_GROUPSEL_COUNT && s->sort[t].subject != FBK_GROUPSEL_AGG) return "unknown sort subject";
    if (s->sort[t].desc > 1) return "unknown sort direction";
    if (s->sort[t].subject == FBK_GROUPSEL_AGG && !has_agg) return "sort on the aggregate of a call without one";
  }
  if (s->n_sort == 2 && s->sort[0].subject == s->sort[1].subject) return "the same sort subject twice";
  if (s->having_subject > FBK_GROUPSEL_AGG) return "unknown having subject";
  if (s->having_subject == FBK_GROUPSEL_AGG && !has_agg) return "having on the aggregate of a call without one";
  if (s->having_subject != FBK_GROUPSEL_NONE && (s->having_op < FBK_HAVING_EQ || s->having_op > FBK_HAVING_BTWN_LT_LT)) return "unknown having op";
  return nullptr;
}

// what the predicate and the keys are computed from, the same on the host and on the device
struct Rules {
  uint32_t having_subject = 0, having_op = 0;
  uint64_t lo = 0, hi = 0;  // order-preserving uint64 (the aggregate's with its sign bit flipped)
  uint32_t n_sort = 0;
  uint32_t subject[2] = {0, 0};
  uint64_t flip[2] = {0, 0};  // XORed onto the raw 64 bits: the sign bit for the aggregate, all bits more for desc
};

inline Rules rules_of(const fbk_groupby_select& s) {
  Rules r;
  r.having_subject = s.having_subject, r.having_op = s.having_op;
  const uint64_t f = s.having_subject == FBK_GROUPSEL_AGG ? kSignBit : 0;
  r.lo = uint64_t(s.having_lo) ^ f, r.hi = uint64_t(s.having_hi) ^ f;
  r.n_sort = s.n_sort;
  for (uint32_t t = 0; t < s.n_sort && t < 2; ++t) {
    r.subject[t] = s.sort[t].subject;
    r.flip[t] = (s.sort[t].subject == FBK_GROUPSEL_AGG ? kSignBit : 0) ^ (s.sort[t].desc ? ~0ull : 0);
  }
  return r;
}

#if defined(__HIPCC__)
#define FBK_GS_BOTH __host__ __device__
#else
#define FBK_GS_BOTH
#endif

// satisfiesCondition on x = the subject's order-preserving uint64
FBK_GS_BOTH inline bool compare(uint32_t op, uint64_t x, uint64_t lo, uint64_t hi) {
  switch (op) {
    case FBK_HAVING_EQ: return x == lo;
    case FBK_HAVING_NEQ: return x != lo;
    case FBK_HAVING_LT: return x < lo;
    case FBK_HAVING_LTE: return x <= lo;
    case FBK_HAVING_GT: return x > lo;
    case FBK_HAVING_GTE: return x >= lo;
    case FBK_HAVING_BETWEEN: return lo <= x && x <= hi;
    case FBK_HAVING_BTWN_LT_LTE: return lo < x && x <= hi;
    case FBK_HAVING_BTWN_LTE_LT: return lo <= x && x < hi;
    case FBK_HAVING_BTWN_LT_LT: return lo < x && x < hi;
  }
  return false;
}

// a group (count > 0, executor.go:8913) that passes having; agg is read only where a subject names it
FBK_GS_BOTH inline bool passes(const Rules& r, uint64_t count, uint64_t agg_bits) {
  if (count == 0) return false;
  if (r.having_subject == FBK_GROUPSEL_NONE) return true;
  return compare(r.having_op, r.having_subject == FBK_GROUPSEL_AGG ? agg_bits ^ kSignBit : count, r.lo, r.hi);
}

FBK_GS_BOTH inline uint64_t key(const Rules& r, uint32_t t, uint64_t count, uint64_t agg_bits) {
  return (r.subject[t] == FBK_GROUPSEL_AGG ? agg_bits : count) ^ r.flip[t];
}

#undef FBK_GS_BOTH

// offset, then limit, on a list of `matched` records: the ranks [lo, end)
struct Window {
  uint64_t lo = 0, end = 0;
  uint64_t n() const { return end - lo; }
};
inline Window window(uint64_t matched, uint64_t offset, uint64_t limit) {
  Window w;
  w.lo = std::min(offset, matched);
  w.end = w.lo + std::min(limit, matched - w.lo);
  return w;
}

// The stage on the host: the cells of the result in order; returns `matched`.  `s` has passed check().
inline uint64_t select(const uint64_t* counts, const int64_t* aggs, uint64_t n, const fbk_groupby_select& s, std::vector<uint32_t>& cells) {
  const Rules r = rules_of(s);
  const bool need_agg = aggs != nullptr;
  auto bits = [&](uint32_t c) { return need_agg ? uint64_t(aggs[c]) : 0; };
  std::vector<uint32_t> m;
  for (uint64_t c = 0; c < n; ++c)
    if (passes(r, counts[c], bits(uint32_t(c)))) m.push_back(uint32_t(c));
  const uint64_t matched = m.size();
  const Window w = window(matched, s.offset, s.limit);
  if (r.n_sort && w.n()) {
    // the cell index decides last: a total order that equals the stable sort of the ascending list
    auto less = [&](uint32_t x, uint32_t y) {
      for (uint32_t t = 0; t < r.n_sort; ++t) {
        const uint64_t kx = key(r, t, counts[x], bits(x)), ky = key(r, t, counts[y], bits(y));
        if (kx != ky) return kx < ky;
      }
      return x < y;
    };
    if (w.end < matched) std::partial_sort(m.begin(), m.begin() + w.end, m.end(), less);
    else std::sort(m.begin(), m.end(), less);
  }
  cells.assign(m.begin() + w.lo, m.begin() + w.end);
  return matched;
}

}  // namespace fbk_group_select
