// fbk_bsi_prog.h — the plane programs of the BSI range predicates, HIP-free (included by the kernels for the opcodes, by
// fbk_bsi_api.inc for the one-shot and prepared Range calls, by fbk_expr_plan.h for the BSI leaves of a call tree, and by
// the stand-alone planner check of the tests).
#pragma once

#include <climits>
#include <cstdint>
#include <vector>

#include "../../include/fbk.h"

namespace fbk {

enum BsiOp : uint32_t {
  kLoadX = 0,   // X = row[r]
  kAndX = 1,    // X &= row[r]            (Row.Intersect)
  kAndnX = 2,   // X &= ~row[r]           (Row.Difference)
  kMorXA = 3,   // M |= X & row[r]        (matched = matched.Union(remaining.Intersect(row)))
  kMorXAn = 4,  // M |= X & ~row[r]       (matched = matched.Union(remaining.Difference(row)))
  kMZero = 5,   // M = 0                  (NewRow())
  kXFromM = 6,  // X = M
  kZeroX = 7,   // X = 0
  kSaveX = 8,   // S = X
  kOrXS = 9,    // X |= S
  kAndnXS = 10, // X &= ~S
  kNop = 255
};

}  // namespace fbk

namespace fbk_bsi {

// ---- BSI plane program generator -------------------------------------------------------------
// Walks the reference's control flow once per query; see BsiOp above.
struct BsiProg {
  std::vector<uint32_t> v;
  void emit(uint32_t op, uint32_t row = 0) { v.push_back((op << 24) | row); }
};
constexpr uint32_t kEx = 0, kSg = 1;  // bsiExistsBit, bsiSignBit (fragment.go:62-65)
inline uint32_t plane(uint64_t i) { return uint32_t(2 + i); }  // bsiOffsetBit + i
inline uint64_t go_shl(uint64_t x, uint64_t s) { return s >= 64 ? 0 : x << s; }  // Go: shift >= width yields 0
inline uint64_t bits_len64(uint64_t x) { return x ? 64 - uint64_t(__builtin_clzll(x)) : 0; }
inline uint64_t abs_int64(int64_t v) {  // absInt64, fragment.go:952-961
  if (v > 0) return uint64_t(v);
  if (v == INT64_MIN) return 9223372036854775808ull;
  return uint64_t(-v);
}

inline void gen_eq(BsiProg& p, uint64_t depth, int64_t pred) {  // rangeEQ, fragment.go:963-1003
  const uint64_t up = abs_int64(pred);
  if (bits_len64(up) > depth) {
    p.emit(fbk::kZeroX);
    return;
  }
  p.emit(fbk::kLoadX, kEx);
  p.emit(pred < 0 ? fbk::kAndX : fbk::kAndnX, kSg);
  for (int i = int(depth) - 1; i >= 0; --i) p.emit(((up >> unsigned(i)) & 1) ? fbk::kAndX : fbk::kAndnX, plane(i));
}

inline void gen_neq(BsiProg& p, uint64_t depth, int64_t pred) {  // rangeNEQ, fragment.go:1005-1022
  gen_eq(p, depth, pred);
  p.emit(fbk::kSaveX);
  p.emit(fbk::kLoadX, kEx);
  p.emit(fbk::kAndnXS);
}

// rangeLTUnsigned, fragment.go:1070-1113: filter in X -> result in X (uses M)
inline void gen_ltu(BsiProg& p, uint64_t depth, uint64_t pred, bool eq) {
  const uint64_t all_ones = go_shl(1, depth) - 1;
  if (bits_len64(pred) > depth) return;
  if (pred == all_ones && eq) return;
  if (pred == all_ones && !eq) {
    p.emit(fbk::kMZero);
    for (uint64_t i = 0; i < depth; ++i) p.emit(fbk::kMorXAn, plane(i));
    p.emit(fbk::kXFromM);
    return;
  }
  if (eq) pred++;
  p.emit(fbk::kMZero);
  for (int i = int(depth) - 1; i >= 0 && pred > 0; --i) {
    if ((pred >> unsigned(i)) & 1) {
      p.emit(fbk::kMorXAn, plane(i));
      pred &= ~(1ull << unsigned(i));
    } else {
      p.emit(fbk::kAndnX, plane(i));
    }
  }
  p.emit(fbk::kXFromM);
}

// rangeGTUnsigned, fragment.go:1157-1208
inline void gen_gtu(BsiProg& p, uint64_t depth, uint64_t pred, bool eq) {
  for (;;) {
    if (pred == 0 && eq) return;
    if (pred == 0 && !eq) {
      p.emit(fbk::kMZero);
      for (uint64_t i = 0; i < depth; ++i) p.emit(fbk::kMorXA, plane(i));
      p.emit(fbk::kXFromM);
      return;
    }
    if (!eq && bits_len64(pred) > depth) {
      p.emit(fbk::kZeroX);
      return;
    }
    if (eq) {
      pred--;
      eq = false;
      continue;
    }
    break;
  }
  p.emit(fbk::kMZero);
  pred |= go_shl(~0ull, depth);
  for (int i = int(depth) - 1; i >= 0 && pred < ~0ull; --i) {
    if ((pred >> unsigned(i)) & 1) {
      p.emit(fbk::kAndX, plane(i));
    } else {
      p.emit(fbk::kMorXA, plane(i));
      pred |= 1ull << unsigned(i);
    }
  }
  p.emit(fbk::kXFromM);
}

inline void gen_lt(BsiProg& p, uint64_t depth, int64_t pred, bool eq) {  // rangeLT, fragment.go:1024-1067
  if (pred == 1 && !eq) {
    pred = 0;
    eq = true;
  }
  const uint64_t up = abs_int64(pred);
  if (pred == 0 && !eq) {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndX, kSg);
  } else if (pred == 0 && eq) {
    gen_eq(p, depth, 0);
    p.emit(fbk::kSaveX);
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndX, kSg);
    p.emit(fbk::kOrXS);
  } else if (pred < 0) {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndX, kSg);
    gen_gtu(p, depth, up, eq);
  } else {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndX, kSg);
    p.emit(fbk::kSaveX);
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndnX, kSg);
    gen_ltu(p, depth, up, eq);
    p.emit(fbk::kOrXS);
  }
}

inline void gen_gt(BsiProg& p, uint64_t depth, int64_t pred, bool eq) {  // rangeGT, fragment.go:1115-1155
  if (pred == -1 && !eq) {
    pred = 0;
    eq = true;
  }
  const uint64_t up = abs_int64(pred);
  if (pred == 0 && !eq) {
    gen_neq(p, depth, 0);
    p.emit(fbk::kAndnX, kSg);
  } else if (pred == 0 && eq) {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndnX, kSg);
  } else if (pred >= 0) {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndnX, kSg);
    gen_gtu(p, depth, up, eq);
  } else {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndnX, kSg);
    p.emit(fbk::kSaveX);
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndX, kSg);
    gen_ltu(p, depth, up, eq);
    p.emit(fbk::kOrXS);
  }
}

// rangeBetweenUnsigned, fragment.go:1262-1303: filter in X -> result in X
inline void gen_between_unsigned(BsiProg& p, uint64_t depth, uint64_t mn, uint64_t mx) {
  if (mx > go_shl(1, depth) - 1) {
    gen_gtu(p, depth, mn, true);
    return;
  }
  if (mn == 0) {
    gen_ltu(p, depth, mx, true);
    return;
  }
  const int diff = int(bits_len64(mx ^ mn));
  for (int i = int(depth) - 1; i >= diff; --i) p.emit(((mn >> unsigned(i)) & 1) ? fbk::kAndX : fbk::kAndnX, plane(i));
  const uint64_t mask = go_shl(~0ull, uint64_t(diff));
  mn &= ~mask;
  mx &= ~mask;
  gen_gtu(p, uint64_t(diff), mn, true);
  gen_ltu(p, uint64_t(diff), mx, true);
}

inline void gen_between(BsiProg& p, uint64_t depth, int64_t lo, int64_t hi) {  // rangeBetween, fragment.go:1213-1260
  const uint64_t ulo = abs_int64(lo), uhi = abs_int64(hi);
  if (lo == hi) {
    gen_eq(p, depth, lo);
  } else if (lo >= 0) {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndnX, kSg);
    gen_between_unsigned(p, depth, ulo, uhi);
  } else if (hi < 0) {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndX, kSg);
    gen_between_unsigned(p, depth, uhi, ulo);
  } else {
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndnX, kSg);
    gen_ltu(p, depth, uhi, true);
    p.emit(fbk::kSaveX);
    p.emit(fbk::kLoadX, kEx);
    p.emit(fbk::kAndX, kSg);
    gen_ltu(p, depth, ulo, true);
    p.emit(fbk::kOrXS);
  }
}

// rangeOp, fragment.go:937-950.  false: not a range operation (ErrInvalidRangeOperation)
inline bool gen_range_op(BsiProg& p, int32_t op, uint32_t depth, int64_t predicate) {
  switch (op) {
    case FBK_BSI_EQ: gen_eq(p, depth, predicate); break;
    case FBK_BSI_NEQ: gen_neq(p, depth, predicate); break;
    case FBK_BSI_LT: gen_lt(p, depth, predicate, false); break;
    case FBK_BSI_LTE: gen_lt(p, depth, predicate, true); break;
    case FBK_BSI_GT: gen_gt(p, depth, predicate, false); break;
    case FBK_BSI_GTE: gen_gt(p, depth, predicate, true); break;
    default: return false;
  }
  return true;
}

}  // namespace fbk_bsi
