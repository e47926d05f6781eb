// Executor::Moments / Var / Corr (fbk_bsi_moments) against
//   - the decimals of the reference's SQL tests (sql3/test/defs/defs_aggregate.go: var_test, corr_test; the tables and the five
//     expectations are those of tests/golden/sql_var_corr.json),
//   - a brute force in __int128 for fields with a nonzero Base, with and without a filter call tree,
//   - the reference's float procedure (aggregateVar / aggregateCorr, sql3/planner/expressionagg.go) written out below, on random
//     fields of values below 2^15 in magnitude: every float sum of CORR is then exact and the decimal must be equal; VAR is
//     compared where the exact variance x 10^6 lies at least 10^-3 from an integer, so that truncation cannot flip.
//     The float procedure's own VAR carries rounding error: n additions into a sum of at most n (2 span)^2, each good to 2^-53 of
//     the sum, i.e. up to (n + 8) 2^-53 4 span^2 in the variance (span = the largest magnitude).  The margin of 10^-3 decimal
//     units covers that only while (n + 8) 2^-53 4 span^2 10^6 <= 5 10^-4 (the other half is for the single division and the
//     multiplication by 10^6 on both sides), so the field VAR is compared on draws its values with span^2 <= 1.126 10^6 / (n + 8).
//     (Without that rule the comparison cannot hold: n = 2 495 values up to 32 767 gave 243759828583146 here and
//     243759828583145 by the float loop, whose error bound at that size is ~1 200 units.)  CORR uses the full range.
//   g++ -std=c++17 -I include tests/cpp/test_moments.cpp -L featurebase_amd/csrc -lfbk
#include <cmath>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "fbk_executor.hpp"

using namespace fbk;

static int failures = 0;
#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);    \
      std::printf("\n");           \
      ++failures;                  \
    }                              \
  } while (0)

static long long opt(const std::optional<int64_t>& v) { return v ? (long long)*v : -999999999999LL; }

// aggregateVar: Update + Eval as the reference writes them
static int64_t ref_var(const std::vector<int64_t>& xs) {
  double sum = 0;
  int64_t n = 0;
  std::vector<double> values;
  for (int64_t x : xs) {
    const double val = double(x);
    sum += val;
    n += 1;
    values.push_back(val);
  }
  const double mean = sum / double(n);
  double variance = 0;
  for (double v : values) variance += (v - mean) * (v - mean);
  variance = variance / double(n);
  return int64_t(variance * std::pow(10.0, 6.0));
}

// aggregateCorr: Update + Eval as the reference writes them
static int64_t ref_corr(const std::vector<int64_t>& xs, const std::vector<int64_t>& ys) {
  int64_t n = 0;
  double sum_X = 0, sum_Y = 0, sum_XY = 0, squareSum_X = 0, squareSum_Y = 0;
  for (size_t i = 0; i < xs.size(); ++i) {
    const double xVal = double(xs[i]), yVal = double(ys[i]);
    sum_X = sum_X + xVal;
    sum_Y = sum_Y + yVal;
    sum_XY = sum_XY + xVal * yVal;
    squareSum_X = squareSum_X + xVal * xVal;
    squareSum_Y = squareSum_Y + yVal * yVal;
    n += 1;
  }
  const double corr = double((double(n) * sum_XY - sum_X * sum_Y)) / (std::sqrt(double((double(n) * squareSum_X - sum_X * sum_X) * (double(n) * squareSum_Y - sum_Y * sum_Y))));
  return int64_t(corr * std::pow(10.0, 6.0));
}

static void golden() {
  const int64_t i1[6] = {10, 10, 11, 12, 12, 13}, d1[6] = {1000, 1000, 1100, 1200, 1200, 1300}, id1[6] = {10, 11, 12, 13, 14, 15};
  const int64_t len_corr[6] = {3, 4, 5, 5, 5, 8}, len_var[6] = {3, 3, 3, 3, 3, 3};
  for (int table = 0; table < 2; ++table) {  // 0 var_test, 1 corr_test
    Index idx;
    idx.CreateIntField("i1", 0, 1000);
    idx.CreateIntField("d1", -100000, 100000);
    idx.CreateIntField("id1", 0, 1000);
    idx.CreateIntField("len_s1", 0, 1000);
    for (uint64_t r = 0; r < 6; ++r) {
      const uint64_t col = r + 1;  // _id
      idx.SetValue("i1", col, i1[r]);
      idx.SetValue("d1", col, d1[r]);
      idx.SetValue("id1", col, id1[r]);
      idx.SetValue("len_s1", col, table ? len_corr[r] : len_var[r]);
    }
    Executor e(idx);
    if (table == 0) {
      EXPECT(opt(e.Var("i1")) == 1222222, "var(i1) = %lld", opt(e.Var("i1")));
      EXPECT(opt(e.Var("id1")) == 2916666, "var(id1) = %lld", opt(e.Var("id1")));
      EXPECT(opt(e.Var("len_s1")) == 0, "var(len(s1)) = %lld", opt(e.Var("len_s1")));
      EXPECT(!e.Corr("len_s1", "i1"), "corr with a constant column has no value");
    } else {
      EXPECT(opt(e.Corr("i1", "d1")) == 1000000, "corr(i1, d1) = %lld", opt(e.Corr("i1", "d1")));
      EXPECT(opt(e.Corr("len_s1", "i1")) == 888234, "corr(len(s1), i1) = %lld", opt(e.Corr("len_s1", "i1")));
    }
  }
  Index empty;
  empty.CreateIntField("v", 0, 10);
  Executor e(empty);
  EXPECT(!e.Var("v") && !e.Corr("v", "v") && e.Moments("v").n == 0, "an index without values has no VAR / CORR");
}

struct Brute {
  uint64_t n = 0;
  __int128 sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
};
static bool same(const Executor::MomentSums& m, const Brute& b, bool two) {
  return m.n == b.n && m.sum_x == b.sx && m.sum_xx == b.sxx && (!two || (m.sum_y == b.sy && m.sum_yy == b.syy && m.sum_xy == b.sxy));
}

// Fields with a nonzero Base against a brute force, with and without a filter call tree; VAR / CORR do not depend on the Base
static void with_base(uint32_t seed) {
  std::mt19937_64 rng(seed);
  Index idx, zero;  // `zero`: the same values minus the Base in fields whose Base is 0
  idx.CreateIntField("x", 1000, 90000);          // Base 1000
  idx.CreateIntField("y", -70000, -500);         // Base -500
  zero.CreateIntField("x", -90000, 90000);
  zero.CreateIntField("y", -90000, 90000);
  idx.CreateSetField("f");
  idx.CreateSetField("g");
  std::map<uint64_t, int64_t> xs, ys;
  std::set<uint64_t> f1, g2, g3;
  for (uint64_t s = 0; s < 5; ++s)
    for (int i = 0; i < 700; ++i) {
      const uint64_t col = (s == 3 ? 9 : s) * ShardWidth + rng() % ShardWidth;
      if (rng() % 8) {
        xs[col] = 1000 + int64_t(rng() % 89001);
        idx.SetValue("x", col, xs[col]);
        zero.SetValue("x", col, xs[col] - 1000);
      }
      if (rng() % 8) {
        ys[col] = -70000 + int64_t(rng() % 69501);
        idx.SetValue("y", col, ys[col]);
        zero.SetValue("y", col, ys[col] + 500);
      }
      if (rng() % 2) idx.SetBit("f", 1, col), f1.insert(col);
      if (rng() % 3 == 0) idx.SetBit("g", 2, col), g2.insert(col);
      if (rng() % 3 == 0) idx.SetBit("g", 3, col), g3.insert(col);
    }
  Executor e(idx), ez(zero);
  // Intersect(Row(f=1), Union(Row(g=2), Not(Row(g=3))))
  const Call tree = Call::Nary(Call::kIntersect, {Call::Row("f", 1), Call::Nary(Call::kUnion, {Call::Row("g", 2), Call::Not(Call::Row("g", 3))})});
  std::set<uint64_t> existence;  // Not() is relative to the index's existence: every column that holds anything
  for (auto& kv : xs) existence.insert(kv.first);
  for (auto& kv : ys) existence.insert(kv.first);
  existence.insert(f1.begin(), f1.end()), existence.insert(g2.begin(), g2.end()), existence.insert(g3.begin(), g3.end());
  for (int filtered = 0; filtered < 2; ++filtered) {
    Brute one, two;
    std::vector<int64_t> vx, vy, v1;
    for (auto& kv : xs) {
      const uint64_t c = kv.first;
      if (filtered && !(f1.count(c) && (g2.count(c) || (existence.count(c) && !g3.count(c))))) continue;
      const __int128 x = kv.second;
      ++one.n, one.sx += x, one.sxx += x * x;
      v1.push_back(kv.second);
      auto it = ys.find(c);
      if (it == ys.end()) continue;
      const __int128 y = it->second;
      ++two.n, two.sx += x, two.sy += y, two.sxx += x * x, two.syy += y * y, two.sxy += x * y;
      vx.push_back(kv.second), vy.push_back(it->second);
    }
    const Call* flt = filtered ? &tree : nullptr;
    const std::string y = "y";
    EXPECT(one.n > 100 && two.n > 100 && two.n < one.n, "degenerate data");
    EXPECT(same(e.Moments("x", nullptr, flt), one, false), "Moments(x) with Base, filter %d", filtered);
    EXPECT(same(e.Moments("x", &y, flt), two, true), "Moments(x, y) with Base, filter %d", filtered);
    if (!filtered) {  // the same VAR / CORR with and without a Base (the filter's fields live in idx only)
      EXPECT(opt(e.Var("x")) == opt(ez.Var("x")), "VAR depends on the Base: %lld / %lld", opt(e.Var("x")), opt(ez.Var("x")));
      EXPECT(opt(e.Corr("x", "y")) == opt(ez.Corr("x", "y")), "CORR depends on the Base: %lld / %lld", opt(e.Corr("x", "y")), opt(ez.Corr("x", "y")));
    }
    EXPECT(opt(e.Corr("x", "y", flt)) == ref_corr(vx, vy), "CORR(x, y) filter %d: %lld, the float procedure %lld", filtered, opt(e.Corr("x", "y", flt)), (long long)ref_corr(vx, vy));
  }
}

// Random fields against the reference's float procedure.  Returns whether the VAR case was kept.
static bool random_case(uint32_t seed) {
  std::mt19937_64 rng(seed);
  Index idx;
  idx.CreateIntField("x", -40000, 40000);
  idx.CreateIntField("y", -40000, 40000);
  idx.CreateIntField("v", -40000, 40000);
  const uint64_t n_cols = 2 + rng() % 3000, n_shards = 1 + rng() % 4;
  const int64_t span = 1 + int64_t(rng() % 32767);  // |x|, |y| <= span < 2^15
  // |v| <= span_v: the float loop's error stays below half the margin (the head of this file)
  const int64_t span_v = std::max<int64_t>(1, int64_t(std::sqrt(1.126e6 / double(n_cols + 8))));
  std::map<uint64_t, int64_t> xs, ys, vs;
  for (uint64_t i = 0; i < n_cols; ++i) {
    const uint64_t col = (rng() % n_shards) * ShardWidth + rng() % ShardWidth;
    if (rng() % 10) xs[col] = int64_t(rng() % uint64_t(2 * span + 1)) - span, idx.SetValue("x", col, xs[col]);
    if (rng() % 10) ys[col] = int64_t(rng() % uint64_t(2 * span + 1)) - span, idx.SetValue("y", col, ys[col]);
    if (rng() % 10) vs[col] = int64_t(rng() % uint64_t(2 * span_v + 1)) - span_v, idx.SetValue("v", col, vs[col]);
  }
  std::vector<int64_t> v1, vx, vy;
  for (auto& kv : vs) v1.push_back(kv.second);
  for (auto& kv : xs) {
    auto it = ys.find(kv.first);
    if (it != ys.end()) vx.push_back(kv.second), vy.push_back(it->second);
  }
  if (v1.size() < 2 || vx.size() < 2) return true;
  Executor e(idx);
  // CORR: every sum of the float procedure is an integer below 2^53, so both sides evaluate the same expression on the same doubles
  const std::optional<int64_t> corr = e.Corr("x", "y");
  EXPECT(corr && *corr == ref_corr(vx, vy), "seed %u: CORR %lld, the float procedure %lld", seed, opt(corr), (long long)ref_corr(vx, vy));
  // VAR: kept when the exact variance x 10^6 = num * 10^6 / n^2 lies at least 10^-3 from an integer
  __int128 n = __int128(v1.size()), sx = 0, sxx = 0;
  for (int64_t x : v1) sx += x, sxx += __int128(x) * x;
  const __int128 num = n * sxx - sx * sx, den = n * n, rem = (num * 1000000) % den;
  if (rem * 1000 < den || (den - rem) * 1000 < den) return false;
  const std::optional<int64_t> var = e.Var("v");
  EXPECT(var && *var == ref_var(v1), "seed %u: VAR %lld, the float procedure %lld", seed, opt(var), (long long)ref_var(v1));
  return true;
}

int main() {
  golden();
  with_base(11);
  int kept = 0;
  const int cases = 30;
  for (int k = 0; k < cases; ++k) kept += random_case(100 + k);
  EXPECT(kept * 10 >= cases * 9, "the generator kept %d of %d VAR cases", kept, cases);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("moments ok (%d of %d VAR cases kept)\n", kept, cases);
  return 0;
}
