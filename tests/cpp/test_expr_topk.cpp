// Executor::TopK / TopN with fuse_calls (the filter tree and the counting as ONE fbk_expr_topk) against the two steps they replace
// (the filter row, then fbk_topk): a seeded index — the set fields "f" of 150 rows and "g" of 40 rows to group by, two set fields and
// an int field for the filters — over shards 0, 1 and 3; filters that are operator trees (rows, a BSI condition, Not, a Shift
// inside), a plain row, plain rows of one field, no filter.  Both settings must give the same pairs.  With fuse_calls an operator-tree
// filter costs exactly one device call beyond the ordering: fbk_expr_topk for "g" (up to 64 rows: the tree is evaluated once per
// shard and slot), fbk_expr_eval before fbk_topk for "f" (Executor::fuses_topk).
//   g++ -std=c++17 -I include tests/cpp/test_expr_topk.cpp -L featurebase_amd/csrc -lfbk
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

struct Both {
  std::vector<Pair> all, top;  // k = 0 and k = 5
  uint64_t calls = 0;          // device calls of TopK(k = 5) with fuse_calls beyond fbk_topk itself
};

static Both run_both(Executor& ex, const Call* filter, const char* f = "f") {
  Both r;
  ex.fuse_calls = false;
  const std::vector<Pair> all0 = ex.TopK(f, 0, filter), top0 = ex.TopK(f, 5, filter), n0 = ex.TopN(f, 3, filter);
  ex.fuse_calls = true;
  r.all = ex.TopK(f, 0, filter);
  const uint64_t before = ex.library_calls;
  r.top = ex.TopK(f, 5, filter);
  r.calls = ex.library_calls - before;
  const std::vector<Pair> n1 = ex.TopN(f, 3, filter);
  EXPECT(r.all == all0);
  EXPECT(r.top == top0);
  EXPECT(n1 == n0);
  EXPECT(r.top.size() <= 5 && r.top.size() <= r.all.size());
  for (size_t i = 0; i < r.top.size(); ++i) EXPECT(r.top[i] == r.all[i]);
  for (size_t i = 1; i < r.all.size(); ++i)
    EXPECT(r.all[i - 1].Count > r.all[i].Count || (r.all[i - 1].Count == r.all[i].Count && r.all[i - 1].ID < r.all[i].ID));
  return r;
}

int main() {
  try {
    const char* seed = std::getenv("FBK_TEST_SEED");
    std::mt19937_64 rng(seed ? std::strtoull(seed, nullptr, 0) : 4242);
    Index idx;
    idx.CreateSetField("f");
    idx.CreateSetField("g");
    idx.CreateSetField("a");
    idx.CreateSetField("b");
    idx.CreateIntField("v", -100000, 100000);
    for (uint64_t sh : {0, 1, 3}) {
      for (int i = 0; i < 30000; ++i) idx.SetBit("f", rng() % 150, (sh << 20) + rng() % (1u << 19));  // sparse rows: arrays
      for (uint64_t c = 2000; c < 9000; ++c) idx.SetBit("f", 7, (sh << 20) + c);                      // a run
      for (int i = 0; i < 30000; ++i) idx.SetBit("f", 8, (sh << 20) + rng() % (1u << 17));             // dense: bitmaps
      for (int i = 0; i < 20000; ++i) idx.SetBit("g", rng() % 40, (sh << 20) + rng() % (1u << 19));
      for (uint64_t c = 500; c < 70000; ++c) idx.SetBit("g", 3, (sh << 20) + c);  // a run and a full container
      for (int i = 0; i < 3000; ++i) idx.SetBit("a", rng() % 6, (sh << 20) + rng() % (1u << 20));
      for (int i = 0; i < 40000; ++i) idx.SetBit("a", 6, (sh << 20) + rng() % (1u << 18));
      for (uint64_t c = 1000; c < 30000; ++c) idx.SetBit("b", 1, (sh << 20) + c);
      for (int i = 0; i < 2000; ++i) idx.SetBit("b", 2 + rng() % 2, (sh << 20) + rng() % (1u << 20));
      for (int i = 0; i < 6000; ++i) idx.SetValue("v", (sh << 20) + rng() % (1u << 18), int64_t(rng() % 200001) - 100000);
    }
    Executor ex(idx);
    auto A = [](uint64_t r) { return Call::Row("a", r); };
    auto B = [](uint64_t r) { return Call::Row("b", r); };
    auto N = [](Call::Kind k, std::vector<Call> ch) { return Call::Nary(k, std::move(ch)); };
    const Call gt = Call::Range("v", FBK_BSI_GT, 5), neq = Call::Range("v", FBK_BSI_NEQ, -7), btw = Call::Between("v", -500, 70000);

    const std::vector<Call> trees = {
        N(Call::kIntersect, {N(Call::kUnion, {A(1), A(6)}), Call::Not(B(3)), gt}),
        N(Call::kIntersect, {A(6), B(1), btw}),
        N(Call::kUnion, {A(6), B(1)}),
        N(Call::kDifference, {A(6), B(1), neq}),
        N(Call::kXor, {N(Call::kIntersect, {gt, A(6)}), N(Call::kUnion, {neq, N(Call::kDifference, {B(1), A(2)})})}),
        Call::Not(A(6)),
        N(Call::kUnion, {A(0), A(1), A(2), A(3), A(4), A(5), A(6), B(1), A(2)}),
    };
    for (const Call& t : trees)
      for (const char* field : {"f", "g"}) {
        const Both r = run_both(ex, &t, field);
        EXPECT(r.calls == 1);
        EXPECT(!r.all.empty());
      }
    {  // the node-by-node path of the first statement: five calls for the filter alone
      ex.fuse_calls = false;
      const uint64_t before = ex.library_calls;
      (void)ex.TopK("f", 5, &trees[0]);
      EXPECT(ex.library_calls - before == 5);
      ex.fuse_calls = true;
    }
    {  // nothing qualifies: a row nobody set
      const Call none = N(Call::kIntersect, {A(77), A(6), gt});
      for (const char* field : {"f", "g"}) {
        const Both r = run_both(ex, &none, field);
        EXPECT(r.calls == 1 && r.all.empty() && r.top.empty());
      }
    }
    {  // Shift inside the tree: the shifts are calls of their own, their result a row leaf of the one fused call
      const Call t = N(Call::kIntersect, {Call::Shift(A(6), 2), btw});
      for (const char* field : {"f", "g"}) {
        const Both r = run_both(ex, &t, field);
        EXPECT(r.calls == 2 + 1 && !r.all.empty());
      }
    }
    {  // a plain row, plain rows of one field and no filter keep today's calls
      const Call row = A(6);
      const Both p = run_both(ex, &row);
      EXPECT(p.calls == 0 && !p.all.empty());
      const Call fold = N(Call::kUnion, {A(0), A(1), A(6)});
      const Both f = run_both(ex, &fold);
      EXPECT(f.calls == 1 && !f.all.empty());  // fbk_fold_n, then fbk_topk
      const Both n = run_both(ex, nullptr);
      EXPECT(n.calls == 0 && n.all.size() == 150);
      const Both pg = run_both(ex, &row, "g"), ng = run_both(ex, nullptr, "g");
      EXPECT(pg.calls == 0 && !pg.all.empty() && ng.calls == 0 && ng.all.size() == 40);
    }
  } catch (const Error& e) {
    std::printf("FAIL fbk error %d: %s\n", e.code, e.what());
    ++failures;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("expr topk ok\n");
  return 0;
}
