// Executor::DistinctRows / Call::Precomputed (fbk_bsi_distinct_rows) — Distinct() as a device row and the foreign-key join of
// TestExecutor_ForeignIndex (executor_test.go:5877-5978, numeric ids for the string keys: one = 1, two = 2, twenty-one = 21 ...):
// two Index objects, the child on a fork of the parent's context; then the columns of DistinctRows against Distinct on a seeded
// field with negative values and a Base, with and without a filter, and a field too wide for a row that takes the list path.
//   g++ -std=c++17 -I include tests/cpp/test_distinct_rows.cpp -L featurebase_amd/csrc -lfbk
#include <cstdio>
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

int main() {
  try {
    Index parent;
    Index child(parent);  // (declared after the parent: closed before it)
    parent.CreateSetField("general");
    for (uint64_t id : {1, 2, 3}) parent.SetBit("general", 1, id);
    for (uint64_t id : {21, 22, 23}) parent.SetBit("general", 2, id);
    for (uint64_t id : {1, 21}) parent.SetBit("general", ShardWidth, id);
    child.CreateIntField("parent_id", 0, INT64_MAX);
    child.CreateSetField("color");
    const uint64_t cols[4] = {1, 2, ShardWidth, 4};
    const int64_t pid[4] = {1, 2, 1, 21};
    const uint64_t color[4] = {1, 2, 2, 1};  // red = 1, blue = 2
    for (int i = 0; i < 4; ++i) {
      child.SetValue("parent_id", cols[i], pid[i]);
      child.SetBit("color", color[i], cols[i]);
    }
    Executor pe(parent), ce(child);
    {
      const SignedRows every = ce.DistinctRows("parent_id");
      EXPECT(every.PosShards == std::vector<uint64_t>{0} && every.NegShards.empty() && every.EmptyRow == 1);
      EXPECT(ce.Values(every) == (std::vector<int64_t>{1, 2, 21}));
      EXPECT(ce.Values(every) == ce.Distinct("parent_id"));
      const Call blue = Call::Row("color", 2);
      const SignedRows joined = ce.DistinctRows("parent_id", &blue);
      EXPECT(ce.Values(joined) == (std::vector<int64_t>{1, 2}));
      const Call join = Call::Nary(Call::kIntersect, {Call::Row("general", ShardWidth), Call::Precomputed(joined)});
      EXPECT(pe.Count(join) == 1);
      EXPECT(pe.Columns(join) == std::vector<uint64_t>{1});
      EXPECT(pe.Count(Call::Nary(Call::kIntersect, {Call::Row("general", 1), Call::Precomputed(every)})) == 2);
      EXPECT(pe.Count(Call::Nary(Call::kIntersect, {Call::Row("general", 2), Call::Precomputed(joined)})) == 0);
      // a selection that holds nothing: an empty SignedRow, and the join with it is empty
      const Call green = Call::Row("color", 3);
      child.SetBit("color", 3, 5 * ShardWidth);  // (a column without a parent_id, in a shard of its own)
      const SignedRows none = ce.DistinctRows("parent_id", &green);
      EXPECT(none.PosShards.empty() && none.NegShards.empty() && none.EmptyRow == 0 && ce.Values(none).empty());
      EXPECT(pe.Count(Call::Nary(Call::kIntersect, {Call::Row("general", 1), Call::Precomputed(none)})) == 0);
    }

    // seeded data with negative values, a Base, and shards without a value
    std::mt19937_64 rng(9990);
    Index idx(parent);
    idx.CreateIntField("v", -3000000, 3000000);
    idx.CreateIntField("based", 5000, 9000000);  // Base 5000
    idx.CreateIntField("wide", INT64_MIN / 2, INT64_MAX / 2);
    idx.CreateSetField("s");
    for (uint64_t sh : {0, 1, 3})
      for (int i = 0; i < 500; ++i) {
        const uint64_t col = (sh << 20) + rng() % (1u << 20);
        if (rng() % 4) idx.SetValue("v", col, int64_t(rng() % 6000001) - 3000000);
        if (rng() % 4) idx.SetValue("based", col, 5000 + int64_t(rng() % 8995001));
        if (i < 10) idx.SetValue("wide", col, (int64_t(rng() % 5) - 2) * (int64_t(1) << 50) + int64_t(rng() % 1000));
        idx.SetBit("s", rng() % 3, col);
      }
    Executor ex(idx);
    const Call f1 = Call::Row("s", 1);
    for (const char* field : {"v", "based", "wide"})
      for (const Call* filter : {static_cast<const Call*>(nullptr), &f1}) {
        const SignedRows r = ex.DistinctRows(field, filter);
        const std::vector<int64_t> want = ex.Distinct(field, filter);
        EXPECT(!want.empty() && ex.Values(r) == want);
        EXPECT(std::is_sorted(r.PosShards.begin(), r.PosShards.end()) && std::is_sorted(r.NegShards.begin(), r.NegShards.end()));
        if (field[0] == 'v') EXPECT(!r.NegShards.empty() && r.PosShards.size() == 3);
        if (field[0] == 'b') EXPECT(r.NegShards.empty());
      }
  } catch (const Error& e) {
    std::printf("FAIL: fbk error %d: %s\n", e.code, e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf("distinct rows ok\n");
  return 0;
}
