// Call::Compare (fbk_bsi_compare) through Executor against a brute force over a small index: two int fields with different Base,
// all six operators, both fuse_calls settings; Count of the row alone and intersected with a set row, the row's columns, and the
// row as the filter of Sum and Sort.
//   g++ -std=c++17 -I include tests/cpp/test_compare.cpp -L featurebase_amd/csrc -lfbk
#include <algorithm>
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

static bool holds(int32_t op, int64_t x, int64_t y) {
  switch (op) {
    case FBK_BSI_EQ: return x == y;
    case FBK_BSI_NEQ: return x != y;
    case FBK_BSI_LT: return x < y;
    case FBK_BSI_LTE: return x <= y;
    case FBK_BSI_GT: return x > y;
    default: return x >= y;
  }
}

int main() {
  std::mt19937_64 rng(77);
  Index idx;
  idx.CreateIntField("a", 1000, 5000);    // Base 1000
  idx.CreateIntField("b", -3000, 4200);   // Base 0
  idx.CreateIntField("c", -9000, -2000);  // Base -2000: always below a
  idx.CreateSetField("f");
  std::map<uint64_t, int64_t> a, b, c;
  std::set<uint64_t> f1;
  for (uint64_t s = 0; s < 4; ++s)
    for (int i = 0; i < 600; ++i) {
      const uint64_t col = (s == 2 ? 7 : s) * ShardWidth + rng() % ShardWidth;
      if (rng() % 8) a[col] = 1000 + int64_t(rng() % 4001), idx.SetValue("a", col, a[col]);
      if (rng() % 8) b[col] = (rng() % 4 == 0 && a.count(col)) ? std::min<int64_t>(a[col], 4200) : -3000 + int64_t(rng() % 7201), idx.SetValue("b", col, b[col]);
      if (rng() % 8) c[col] = -9000 + int64_t(rng() % 7001), idx.SetValue("c", col, c[col]);
      if (rng() % 2) idx.SetBit("f", 1, col), f1.insert(col);
    }
  Executor e(idx);
  const int32_t ops[6] = {FBK_BSI_EQ, FBK_BSI_NEQ, FBK_BSI_LT, FBK_BSI_LTE, FBK_BSI_GT, FBK_BSI_GTE};
  for (int fuse = 0; fuse < 2; ++fuse) {
    e.fuse_calls = fuse != 0;
    for (int32_t op : ops) {
      std::vector<uint64_t> cols, cols_f;
      __int128 sum_a = 0;
      uint64_t n_ac = 0;
      for (auto& kv : a) {
        auto it = b.find(kv.first);
        if (it != b.end() && holds(op, kv.second, it->second)) {
          cols.push_back(kv.first);
          sum_a += kv.second;
          if (f1.count(kv.first)) cols_f.push_back(kv.first);
        }
        auto ic = c.find(kv.first);
        if (ic != c.end() && holds(op, kv.second, ic->second)) ++n_ac;
      }
      const Call cmp = Call::Compare("a", op, "b");
      EXPECT(!cols.empty() && !cols_f.empty() && cols_f.size() < cols.size(), "degenerate data, op %d", op);
      EXPECT(e.Count(cmp) == cols.size(), "fuse %d op %d: Count %llu, brute force %zu", fuse, op, (unsigned long long)e.Count(cmp), cols.size());
      EXPECT(e.Columns(cmp) == cols, "fuse %d op %d: Columns differ", fuse, op);
      const Call both = Call::Nary(Call::kIntersect, {cmp, Call::Row("f", 1)});
      EXPECT(e.Count(both) == cols_f.size(), "fuse %d op %d: Count(Intersect(Compare, Row)) %llu, brute force %zu", fuse, op, (unsigned long long)e.Count(both),
             cols_f.size());
      EXPECT(e.Columns(both) == cols_f, "fuse %d op %d: Columns(Intersect(Compare, Row)) differ", fuse, op);
      const ValCount s = e.Sum("a", &cmp);
      EXPECT(s.Count == int64_t(cols.size()) && __int128(s.Val) == sum_a, "fuse %d op %d: Sum(a, filter = Compare)", fuse, op);
      const SortedRow sorted = e.Sort("a", &cmp, false, UINT64_MAX, 0, true);  // (keep_zero: a == Base takes part)
      EXPECT(sorted.Columns.size() == cols.size() && std::is_sorted(sorted.Values.begin(), sorted.Values.end()), "fuse %d op %d: Sort(a, filter = Compare)", fuse, op);
      // a >= 1000 > -2000 >= c wherever both exist: different Base on both sides, nothing in common but the columns
      const uint64_t ac = e.Count(Call::Compare("a", op, "c"));
      EXPECT(ac == n_ac, "fuse %d op %d: Count(a op c) %llu, brute force %llu", fuse, op, (unsigned long long)ac, (unsigned long long)n_ac);
      // the same field on both sides
      const uint64_t aa = e.Count(Call::Compare("a", op, "a"));
      EXPECT(aa == (holds(op, 0, 0) ? a.size() : 0), "fuse %d op %d: Count(a op a) %llu", fuse, op, (unsigned long long)aa);
    }
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("compare ok\n");
  return 0;
}
