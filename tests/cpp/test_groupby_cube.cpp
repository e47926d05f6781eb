// Executor::GroupBy over three and four set fields (fbk_count_cube for the last three levels) against a brute force over the
// index's own columns: random indexes over 16 shards, with and without a filter and a limit; a leading field wide enough to need
// two blocks of rows under the call's 2^24 groups; and a count of the fbk_setop calls a three-field GroupBy issues (none: the
// filter goes into the call, no prefix ∩ row is materialised).  Groups in odometer order over ascending row ids.
//   g++ -std=c++17 -I include tests/cpp/test_groupby_cube.cpp -L featurebase_amd/csrc -lfbk
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "fbk.h"

// every fbk_setop the mirror issues goes through this wrapper
static int n_setop = 0;
static inline int32_t counted_setop(fbk_ctx* ctx, int32_t op, const fbk_batch* a, const uint32_t* rows_a, const fbk_batch* b, const uint32_t* rows_b,
                                    uint64_t n_pairs, uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts) {
  ++n_setop;
  return fbk_setop(ctx, op, a, rows_a, b, rows_b, n_pairs, flags, out_batch, out_counts);
}
#define fbk_setop counted_setop
#include "fbk_executor.hpp"
#undef fbk_setop

using namespace fbk;
typedef std::map<uint64_t, std::set<uint64_t>> Rows;

static int failures = 0;

// the groups of fields[level..] whose columns lie in `cols`, appended in odometer order (an empty prefix has no groups)
static void brute(const std::vector<const Rows*>& f, size_t level, const std::set<uint64_t>& cols, const std::vector<std::string>& names,
                  std::vector<FieldRow>& group, std::vector<GroupCount>& out) {
  for (const auto& kv : *f[level]) {
    std::set<uint64_t> x;
    for (uint64_t c : kv.second)
      if (cols.count(c)) x.insert(c);
    if (x.empty()) continue;
    group.push_back({names[level], kv.first});
    if (level + 1 < f.size()) {
      brute(f, level + 1, x, names, group, out);
    } else {
      GroupCount g;
      g.Group = group;
      g.Count = x.size();
      out.push_back(g);
    }
    group.pop_back();
  }
}

// n_rows[k]: the rows of field k (ids 10 (k + 1) + 0 .. n_rows[k] - 1)
static void run(const std::vector<uint64_t>& n_rows, uint32_t seed, uint64_t n_shards = 16, uint64_t per_shard = 600) {
  std::mt19937_64 rng(seed);
  const int n_fields = int(n_rows.size());
  Index idx;
  std::vector<std::string> names;
  std::vector<Rows> rows(n_fields);
  for (int k = 0; k < n_fields; ++k) {
    names.push_back("f" + std::to_string(k));
    idx.CreateSetField(names.back());
  }
  for (uint64_t s = 0; s < n_shards; ++s)
    for (uint64_t i = 0; i < per_shard; ++i) {
      const uint64_t col = s * ShardWidth + rng() % ShardWidth;
      for (int k = 0; k < n_fields; ++k) {
        if (rng() % 8 == 0) continue;
        const uint64_t r = 10 * (k + 1) + rng() % n_rows[k];
        idx.SetBit(names[k], r, col);
        rows[k][r].insert(col);
      }
    }
  Executor e(idx);
  std::vector<const Rows*> f;
  for (auto& r : rows) f.push_back(&r);
  std::set<uint64_t> all;
  for (auto& r : rows)
    for (auto& kv : r) all.insert(kv.second.begin(), kv.second.end());
  const uint64_t filter_row = rows[n_fields - 1].begin()->first;
  for (int filtered = 0; filtered < 2; ++filtered) {
    std::set<uint64_t> cols = all;
    Call filt = Call::Row(names[n_fields - 1], filter_row);
    if (filtered) cols = rows[n_fields - 1][filter_row];
    std::vector<GroupCount> want;
    std::vector<FieldRow> group;
    brute(f, 0, cols, names, group, want);
    for (uint64_t limit : {uint64_t(0), uint64_t(5)}) {
      n_setop = 0;
      std::vector<GroupCount> got = e.GroupBy(names, filtered ? &filt : nullptr, "", limit);
      std::vector<GroupCount> exp = want;
      if (limit && exp.size() > limit) exp.resize(limit);
      if (got != exp) {
        std::printf("FAIL fields=%d rows0=%llu filter=%d limit=%llu: %zu groups, expected %zu\n", n_fields, (unsigned long long)n_rows[0], filtered,
                    (unsigned long long)limit, got.size(), exp.size());
        for (size_t i = 0; i < got.size() && i < exp.size(); ++i)
          if (!(got[i] == exp[i])) {
            std::printf("  first difference at %zu: count %llu / %llu\n", i, (unsigned long long)got[i].Count, (unsigned long long)exp[i].Count);
            break;
          }
        ++failures;
      }
      if (n_fields == 3 && n_setop) {
        std::printf("FAIL fields=3 filter=%d limit=%llu: GroupBy issued %d fbk_setop calls, expected none\n", filtered, (unsigned long long)limit, n_setop);
        ++failures;
      }
      if (exp.empty()) {
        std::printf("FAIL fields=%d filter=%d: the brute force found no group (the test data is degenerate)\n", n_fields, filtered);
        ++failures;
      }
    }
  }
}

int main() {
  run({5, 7, 7}, 1);
  run({9, 33, 2}, 2);
  run({3, 4, 5, 6}, 3);  // four fields: the leading one fixed a row at a time, the last three one cube each
  run({1, 1, 1}, 4);
  // 600 x 300 x 100 groups are more than a call takes (2^24): the leading field goes in two blocks of rows (559 + 41)
  run({600, 300, 100}, 5, 2, 2000);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("groupby cube ok\n");
  return 0;
}
