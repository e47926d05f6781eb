// Executor::GroupByQuantiles (fbk_count_matrix_quantiles for the last one or two levels) against a brute force: a by-hand index
// first, then random indexes of 1, 2 and 3 set fields over 16 shards and three int fields — "v" with values of both signs (Base 0),
// "w" below zero throughout (Base = its max, -100: every stored value is negative or 0) and "p" above zero (Base = its min, 500) —
// with and without a filter and a limit, and a field of more rows than one call takes per side; a set field as the aggregate field
// is an error.  Count = |group ∩ filter|; N = the columns of the group with a value; per fraction num / den the value at the
// ascending rank max(1, ceil(N * num / den)) - 1 and the number of columns holding it; zeros for a group without a value.
//   g++ -std=c++17 -I include tests/cpp/test_groupby_quantiles.cpp -L featurebase_amd/csrc -lfbk
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "fbk_executor.hpp"

using namespace fbk;
typedef std::map<uint64_t, std::set<uint64_t>> Rows;

static int failures = 0;
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

typedef std::vector<std::pair<uint32_t, uint32_t>> Fractions;
static const Fractions kFr = {{0, 1}, {1, 2}, {1, 1}, {1, 4}, {99, 100}, {1, 2}};  // (one of them twice)

static GroupQuantiles G(std::vector<FieldRow> group, uint64_t count, uint64_t n, std::vector<int64_t> values, std::vector<uint64_t> counts) {
  GroupQuantiles g;
  g.Group = std::move(group);
  g.Count = count, g.N = n, g.Values = std::move(values), g.Counts = std::move(counts);
  return g;
}

static void by_hand() {
  const uint64_t SW = ShardWidth;
  Index idx;
  idx.CreateSetField("general");
  idx.CreateSetField("sub");
  idx.CreateIntField("v", -1000, 1000);
  const uint64_t gen[][2] = {{10, 0}, {10, 1}, {10, SW + 1}, {11, 2}, {11, SW + 2}, {12, 2}, {12, SW + 2}};
  for (auto& b : gen) idx.SetBit("general", b[0], b[1]);
  const uint64_t sub[][2] = {{100, 0}, {100, 1}, {100, 3}, {100, SW + 1}, {110, 2}, {110, 0}};
  for (auto& b : sub) idx.SetBit("sub", b[0], b[1]);
  idx.SetValue("v", 0, 10);
  idx.SetValue("v", 1, -100);
  idx.SetValue("v", SW + 1, -100);
  idx.SetValue("v", SW + 10, 7);
  Executor e(idx);
  const Fractions fr = {{0, 1}, {1, 2}, {1, 1}};
  // (10, 100) = {0, 1, SW + 1}: -100, -100, 10 over two shards; (10, 110) = {0}; (11, 110) = (12, 110) = {2}: no value
  EXPECT(e.GroupByQuantiles({"general", "sub"}, nullptr, "v", fr) ==
         (std::vector<GroupQuantiles>{G({{"general", 10}, {"sub", 100}}, 3, 3, {-100, -100, 10}, {2, 2, 1}), G({{"general", 10}, {"sub", 110}}, 1, 1, {10, 10, 10}, {1, 1, 1}),
                                      G({{"general", 11}, {"sub", 110}}, 1, 0, {0, 0, 0}, {0, 0, 0}), G({{"general", 12}, {"sub", 110}}, 1, 0, {0, 0, 0}, {0, 0, 0})}));
  EXPECT(e.GroupByQuantiles({"general"}, nullptr, "v", fr) ==
         (std::vector<GroupQuantiles>{G({{"general", 10}}, 3, 3, {-100, -100, 10}, {2, 2, 1}), G({{"general", 11}}, 2, 0, {0, 0, 0}, {0, 0, 0}),
                                      G({{"general", 12}}, 2, 0, {0, 0, 0}, {0, 0, 0})}));
  EXPECT(e.GroupByQuantiles({"general"}, nullptr, "v", {}) ==
         (std::vector<GroupQuantiles>{G({{"general", 10}}, 3, 3, {}, {}), G({{"general", 11}}, 2, 0, {}, {}), G({{"general", 12}}, 2, 0, {}, {})}));
  Call neg = Call::Range("v", FBK_BSI_LT, 0);  // filter=Row(v < 0)
  EXPECT(e.GroupByQuantiles({"general", "sub"}, &neg, "v", fr) ==
         (std::vector<GroupQuantiles>{G({{"general", 10}, {"sub", 100}}, 2, 2, {-100, -100, -100}, {2, 2, 2})}));
  EXPECT(e.GroupByQuantiles({"general", "sub"}, nullptr, "v", fr, 2).size() == 2);
  bool threw = false;
  try {
    e.GroupByQuantiles({"general", "sub"}, nullptr, "sub", fr);
  } catch (const Error& err) {
    threw = err.code == FBK_E_INVALID;
  }
  EXPECT(threw);
  threw = false;
  try {
    e.GroupByQuantiles({"general"}, nullptr, "v", {{3, 2}});  // num > den: the library's error comes through
  } catch (const Error& err) {
    threw = err.code == FBK_E_INVALID;
  }
  EXPECT(threw);
  EXPECT(e.GroupByQuantiles({"general"}, nullptr, "v", fr).size() == 3);  // and the executor goes on
}

// the groups of fields[level..] whose columns lie in `cols`, appended in odometer order
static void brute(const std::vector<const Rows*>& f, size_t level, const std::set<uint64_t>& cols, const std::vector<std::string>& names,
                  const std::map<uint64_t, int64_t>& values, std::vector<FieldRow>& group, std::vector<GroupQuantiles>& out) {
  for (const auto& kv : *f[level]) {
    std::set<uint64_t> x;
    for (uint64_t c : kv.second)
      if (cols.count(c)) x.insert(c);
    group.push_back({names[level], kv.first});
    if (level + 1 < f.size()) {
      brute(f, level + 1, x, names, values, group, out);
    } else if (!x.empty()) {
      GroupQuantiles g;
      g.Group = group;
      g.Count = x.size();
      std::vector<int64_t> sorted;
      for (uint64_t c : x) {
        auto it = values.find(c);
        if (it != values.end()) sorted.push_back(it->second);
      }
      std::sort(sorted.begin(), sorted.end());
      g.N = sorted.size();
      for (const auto& fr : kFr) {
        if (sorted.empty()) {
          g.Values.push_back(0), g.Counts.push_back(0);
          continue;
        }
        const uint64_t c = (uint64_t(sorted.size()) * fr.first + fr.second - 1) / fr.second, k = std::max<uint64_t>(1, c) - 1;
        g.Values.push_back(sorted[k]);
        g.Counts.push_back(uint64_t(std::count(sorted.begin(), sorted.end(), sorted[k])));
      }
      out.push_back(g);
    }
    group.pop_back();
  }
}

// n_rows[k]: the rows of field k (ids 10 (k + 1) + 0 .. n_rows[k] - 1)
static void run(const std::vector<uint64_t>& n_rows, uint32_t seed, uint64_t per_shard = 600) {
  std::mt19937_64 rng(seed);
  const int n_fields = int(n_rows.size());
  const uint64_t n_shards = 16;
  Index idx;
  std::vector<std::string> names;
  std::vector<Rows> rows(n_fields);
  for (int k = 0; k < n_fields; ++k) {
    names.push_back("f" + std::to_string(k));
    idx.CreateSetField(names.back());
  }
  idx.CreateIntField("v", -5000, 100000);  // Base 0
  idx.CreateIntField("w", -9000, -100);    // Base -100: stored values <= 0
  idx.CreateIntField("p", 500, 9000);      // Base 500
  const char* ints[3] = {"v", "w", "p"};
  std::map<uint64_t, int64_t> values[3];
  for (uint64_t s = 0; s < n_shards; ++s)
    for (uint64_t i = 0; i < per_shard; ++i) {
      const uint64_t col = s * ShardWidth + rng() % ShardWidth;
      for (int k = 0; k < n_fields; ++k) {
        if (rng() % 4 == 0) continue;
        const uint64_t r = 10 * (k + 1) + rng() % n_rows[k];
        idx.SetBit(names[k], r, col);
        rows[k][r].insert(col);
      }
      if (rng() % 3) {
        const int64_t t = int64_t(rng() % 41);  // few values: groups and shards share them, the counts exceed 1
        const int64_t v[3] = {t * 5 - 100, -100 - t * 3, 500 + t * 7};
        for (int q = 0; q < 3; ++q) {
          idx.SetValue(ints[q], col, v[q]);
          values[q][col] = v[q];
        }
      }
    }
  Executor e(idx);
  std::vector<const Rows*> f;
  for (auto& r : rows) f.push_back(&r);
  std::set<uint64_t> all;
  for (auto& r : rows)
    for (auto& kv : r) all.insert(kv.second.begin(), kv.second.end());
  for (int q = 0; q < 3; ++q)
    for (int filtered = 0; filtered < 2; ++filtered) {
      std::set<uint64_t> cols = all;
      Call filt = Call::Row(names[0], 11);
      if (filtered) cols = rows[0][11];
      std::vector<GroupQuantiles> want;
      std::vector<FieldRow> group;
      brute(f, 0, cols, names, values[q], group, want);
      for (uint64_t limit : {uint64_t(0), uint64_t(5)}) {
        std::vector<GroupQuantiles> got = e.GroupByQuantiles(names, filtered ? &filt : nullptr, ints[q], kFr, limit);
        std::vector<GroupQuantiles> exp = want;
        if (limit && exp.size() > limit) exp.resize(limit);
        if (got != exp) {
          std::printf("FAIL fields=%d field=%s filter=%d limit=%llu: %zu groups, expected %zu\n", n_fields, ints[q], filtered, (unsigned long long)limit,
                      got.size(), exp.size());
          for (size_t i = 0; i < got.size() && i < exp.size(); ++i)
            if (!(got[i] == exp[i])) {
              std::printf("  first difference at %zu: count %llu / %llu, N %llu / %llu\n", i, (unsigned long long)got[i].Count, (unsigned long long)exp[i].Count,
                          (unsigned long long)got[i].N, (unsigned long long)exp[i].N);
              for (size_t k = 0; k < kFr.size() && k < got[i].Values.size(); ++k)
                std::printf("    %u / %u: %lld x %llu / %lld x %llu\n", kFr[k].first, kFr[k].second, (long long)got[i].Values[k], (unsigned long long)got[i].Counts[k],
                            (long long)exp[i].Values[k], (unsigned long long)exp[i].Counts[k]);
              break;
            }
          ++failures;
        }
        bool spread = false, shared = false;
        for (const GroupQuantiles& g : exp) spread = spread || (g.N && g.Values[0] < g.Values[1] && g.Values[1] < g.Values[2]), shared = shared || (g.N && g.Counts[1] > 1);
        if (!filtered && !limit && n_rows[0] < 100 && !(spread && shared)) {
          std::printf("FAIL fields=%d: no group with three different answers or none with a shared median (the test data is degenerate)\n", n_fields);
          ++failures;
        }
      }
    }
}

int main() {
  by_hand();
  run({5, 7}, 1);
  run({5, 7, 7}, 2);  // three levels: the first one fixed row by row, the last two one call
  run({5}, 4);        // one field: the last level alone
  // more rows than one call takes per side (4096): the executor splits the field into blocks of rows
  run({5000, 3}, 6, 1500);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("groupby quantiles ok\n");
  return 0;
}
