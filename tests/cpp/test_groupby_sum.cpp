// Executor::GroupBy with aggregate=Sum(field) (fbk_count_matrix_sum for the last one or two levels) against a brute force
// over the index's own columns: random indexes of 1, 2 and 3 set fields (one of them wider than a call takes: 5000 rows) and
// one int field over 16 shards, with and without a filter and a limit.  Groups in odometer order over ascending row ids,
// Count = columns WITH a value, Agg = their sum.
//   g++ -std=c++17 -I include tests/cpp/test_groupby_sum.cpp -L featurebase_amd/csrc -lfbk
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "fbk_executor.hpp"

using namespace fbk;
typedef std::map<uint64_t, std::set<uint64_t>> Rows;

static int failures = 0;

// the groups of fields[level..] whose columns lie in `cols`, appended in odometer order
static void brute(const std::vector<const Rows*>& f, size_t level, const std::set<uint64_t>& cols, const std::vector<std::string>& names,
                  const std::map<uint64_t, int64_t>& values, std::vector<FieldRow>& group, std::vector<GroupCount>& out) {
  for (const auto& kv : *f[level]) {
    std::set<uint64_t> x;
    for (uint64_t c : kv.second)
      if (cols.count(c)) x.insert(c);
    group.push_back({names[level], kv.first});
    if (level + 1 < f.size()) {
      brute(f, level + 1, x, names, values, group, out);
    } else {
      GroupCount g;
      g.Group = group;
      for (uint64_t c : x) {
        auto it = values.find(c);
        if (it == values.end()) continue;
        ++g.Count;
        g.Agg += it->second;
      }
      if (g.Count) out.push_back(g);
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
  idx.CreateIntField("v", -5000, 100000);
  std::map<uint64_t, int64_t> values;
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
        const int64_t v = int64_t(rng() % 105001) - 5000;
        idx.SetValue("v", col, v);
        values[col] = v;
      }
    }
  Executor e(idx);
  std::vector<const Rows*> f;
  for (auto& r : rows) f.push_back(&r);
  std::set<uint64_t> all;
  for (auto& r : rows)
    for (auto& kv : r) all.insert(kv.second.begin(), kv.second.end());
  for (int filtered = 0; filtered < 2; ++filtered) {
    std::set<uint64_t> cols = all;
    Call filt = Call::Row(names[0], 11);
    if (filtered) cols = rows[0][11];
    std::vector<GroupCount> want;
    std::vector<FieldRow> group;
    brute(f, 0, cols, names, values, group, want);
    for (uint64_t limit : {uint64_t(0), uint64_t(5)}) {
      std::vector<GroupCount> got = e.GroupBy(names, filtered ? &filt : nullptr, "v", limit);
      std::vector<GroupCount> exp = want;
      if (limit && exp.size() > limit) exp.resize(limit);
      if (got != exp) {
        std::printf("FAIL fields=%d filter=%d limit=%llu: %zu groups, expected %zu\n", n_fields, filtered, (unsigned long long)limit, got.size(), exp.size());
        for (size_t i = 0; i < got.size() && i < exp.size(); ++i)
          if (!(got[i] == exp[i])) {
            std::printf("  first difference at %zu: count %llu / %llu, agg %lld / %lld\n", i, (unsigned long long)got[i].Count,
                        (unsigned long long)exp[i].Count, (long long)got[i].Agg, (long long)exp[i].Agg);
            break;
          }
        ++failures;
      }
      if (exp.empty() && !filtered) {
        std::printf("FAIL fields=%d filter=%d: the brute force found no group (the test data is degenerate)\n", n_fields, filtered);
        ++failures;
      }
    }
  }
}

int main() {
  run({5, 7}, 1);
  run({5, 7, 7}, 2);
  run({5, 7}, 3);
  run({5}, 4);  // one field: the last level alone, A rows against no B rows
  // more rows than one call takes per side (4096): the executor splits the field into blocks of rows
  run({5000}, 5, 1500);
  run({5000, 1}, 6, 1500);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("groupby sum ok\n");
  return 0;
}
