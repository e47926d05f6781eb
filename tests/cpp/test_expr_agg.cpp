// Executor::Sum / Min / Max with fuse_calls (the filter tree and the aggregate as ONE fbk_expr_bsi_agg) against the two steps they
// replace (the filter row, then fbk_bsi_sum / _min / _max): a seeded index — two set fields, an int field with negative values, one
// with a Base — over shards 0, 1 and 3; filters that are operator trees (rows, BSI conditions of the aggregated field and of
// another, Not, a Shift inside), plain rows, no filter.  Both settings must give the same ValCount; with fuse_calls an
// operator-tree filter costs exactly one device call.
//   g++ -std=c++17 -I include tests/cpp/test_expr_agg.cpp -L featurebase_amd/csrc -lfbk
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fbk_executor.hpp"

using namespace fbk;

static int failures = 0;
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

struct Three {
  ValCount sum, min, max;
  uint64_t calls[3] = {0, 0, 0};  // device calls of Sum, Min, Max with fuse_calls
};

// the three aggregates under both settings; what they give must be identical
static Three run_both(Executor& ex, const std::string& field, const Call* filter) {
  Three r;
  ex.fuse_calls = false;
  const ValCount s0 = ex.Sum(field, filter), lo0 = ex.Min(field, filter), hi0 = ex.Max(field, filter);
  ex.fuse_calls = true;
  uint64_t before = ex.library_calls;
  r.sum = ex.Sum(field, filter);
  r.calls[0] = ex.library_calls - before;
  before = ex.library_calls;
  r.min = ex.Min(field, filter);
  r.calls[1] = ex.library_calls - before;
  before = ex.library_calls;
  r.max = ex.Max(field, filter);
  r.calls[2] = ex.library_calls - before;
  EXPECT(r.sum == s0);
  EXPECT(r.min == lo0);
  EXPECT(r.max == hi0);
  EXPECT(r.sum.Count == 0 || (r.min.Val <= r.max.Val && r.min.Count <= r.sum.Count && r.max.Count <= r.sum.Count));
  return r;
}

int main() {
  try {
    const char* seed = std::getenv("FBK_TEST_SEED");
    std::mt19937_64 rng(seed ? std::strtoull(seed, nullptr, 0) : 4242);
    Index idx;
    idx.CreateSetField("a");
    idx.CreateSetField("b");
    idx.CreateIntField("v", -100000, 100000);
    idx.CreateIntField("based", 5000, 900000);  // Base 5000
    for (uint64_t sh : {0, 1, 3}) {
      for (int i = 0; i < 3000; ++i) idx.SetBit("a", rng() % 6, (sh << 20) + rng() % (1u << 20));
      for (int i = 0; i < 40000; ++i) idx.SetBit("a", 6, (sh << 20) + rng() % (1u << 18));  // a dense row
      for (uint64_t c = 1000; c < 30000; ++c) idx.SetBit("b", 1, (sh << 20) + c);           // runs
      for (int i = 0; i < 2000; ++i) idx.SetBit("b", 2 + rng() % 2, (sh << 20) + rng() % (1u << 20));
      for (int i = 0; i < 6000; ++i) {
        const uint64_t col = (sh << 20) + rng() % (1u << 18);
        idx.SetValue("v", col, int64_t(rng() % 200001) - 100000);
        if (i % 3 == 0) idx.SetValue("based", col, 5000 + int64_t(rng() % 800000));
      }
    }
    Executor ex(idx);
    auto A = [](uint64_t r) { return Call::Row("a", r); };
    auto B = [](uint64_t r) { return Call::Row("b", r); };
    auto N = [](Call::Kind k, std::vector<Call> ch) { return Call::Nary(k, std::move(ch)); };
    const Call gt = Call::Range("v", FBK_BSI_GT, 5), neq = Call::Range("v", FBK_BSI_NEQ, -7), lte = Call::Range("based", FBK_BSI_LTE, 300000);
    const Call btw = Call::Between("v", -500, 70000);

    // SELECT SUM / MIN / MAX ... WHERE <the WHERE clause of the design note>: one call each
    const Call where = N(Call::kIntersect, {N(Call::kUnion, {A(1), A(6)}), Call::Not(B(3)), gt});
    for (const char* field : {"v", "based"}) {
      const Three t = run_both(ex, field, &where);
      EXPECT(t.calls[0] == 1 && t.calls[1] == 1 && t.calls[2] == 1);
      EXPECT(t.sum.Count > 0);
    }
    {  // the node-by-node path of the same statement: five calls for the filter alone
      ex.fuse_calls = false;
      const uint64_t before = ex.library_calls;
      (void)ex.Sum("v", &where);
      EXPECT(ex.library_calls - before == 5);
      ex.fuse_calls = true;
    }
    const std::vector<Call> trees = {
        N(Call::kIntersect, {A(6), B(1), btw}),
        N(Call::kUnion, {A(6), lte}),
        N(Call::kDifference, {A(6), B(1), neq}),
        N(Call::kXor, {N(Call::kIntersect, {gt, A(6)}), N(Call::kUnion, {neq, N(Call::kDifference, {B(1), lte})})}),
        Call::Not(A(6)),
        N(Call::kIntersect, {A(77), A(6), gt}),                                  // a row nobody set: nothing qualifies, (0, 0)
        N(Call::kIntersect, {Call::Range("v", FBK_BSI_LT, 1 << 30), B(1)}),      // covers everything: the not-null row
        N(Call::kUnion, {A(0), A(1), A(2), A(3), A(4), A(5), A(6), B(1), A(2)}),  // two fields: the interpreter
    };
    for (const Call& t : trees)
      for (const char* field : {"v", "based"}) {
        const Three r = run_both(ex, field, &t);
        EXPECT(r.calls[0] == 1 && r.calls[1] == 1 && r.calls[2] == 1);
      }
    {  // nothing qualifies
      const Call none = N(Call::kIntersect, {A(77), A(6), gt});
      const Three r = run_both(ex, "v", &none);
      EXPECT(r.sum == ValCount{} && r.min == ValCount{} && r.max == ValCount{});
    }
    {  // Shift inside the tree: the shifts are calls of their own, their result a row leaf of the one fused call
      const Call t = N(Call::kIntersect, {Call::Shift(A(6), 2), btw});
      const Three r = run_both(ex, "v", &t);
      EXPECT(r.calls[0] == 2 + 1 && r.calls[1] == 2 + 1 && r.calls[2] == 2 + 1);
    }
    {  // a plain row, a bare condition and no filter keep today's calls: nothing of the filter is evaluated by a tree
      const Call row = A(6);
      const Three p = run_both(ex, "v", &row);
      EXPECT(p.calls[0] == 0 && p.calls[1] == 0 && p.calls[2] == 0 && p.sum.Count > 0);
      const Three c = run_both(ex, "based", &gt);
      EXPECT(c.calls[0] == 1 && c.calls[1] == 1 && c.calls[2] == 1);  // fbk_bsi_range, then the aggregate
      const Three n = run_both(ex, "v", nullptr);
      EXPECT(n.calls[0] == 0 && n.sum.Count > 0);
      // plain rows of one field: fbk_fold_n, then the aggregate
      const Call fold = N(Call::kUnion, {A(0), A(1), A(6)});
      const Three f = run_both(ex, "v", &fold);
      EXPECT(f.calls[0] == 1 && f.calls[1] == 1 && f.calls[2] == 1);
    }
  } catch (const Error& e) {
    std::printf("FAIL fbk error %d: %s\n", e.code, e.what());
    ++failures;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("expr agg ok\n");
  return 0;
}
