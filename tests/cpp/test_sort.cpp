// Executor::Sort and Executor::ExtractSorted (fbk_bsi_sort, fbk_extract_open_columns + the per-field extract calls): the int query
// of the reference's TestExecutor_Sort (tests/golden/sort_vectors.json, handed over as a text file by tests/test_cpp_sort.py), then
// a seeded index — an int field with negative values and many ties, one with a Base, a set field — over shards 0, 1, 3 and 7
// against a std::stable_sort on the host: ascending and descending, with and without a filter, limit / offset, stored zeros
// dropped (the reference) or kept.  Equal values come in ascending column id.
//   g++ -std=c++17 -I include tests/cpp/test_sort.cpp -L featurebase_amd/csrc -lfbk
#include <cstdio>
#include <fstream>
#include <map>
#include <random>
#include <set>
#include <sstream>
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

// lines: value COL V | query PREDICATE LIMIT OFFSET DESC | want COL V
static void golden(const char* path) {
  std::ifstream in(path);
  EXPECT(bool(in));
  Index idx;
  idx.CreateIntField("bsint", INT64_MIN, INT64_MAX);
  int64_t pred = 0;
  uint64_t limit = 0, offset = 0;
  int desc = 0;
  std::vector<std::pair<uint64_t, int64_t>> want;
  std::string line, w;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    ss >> w;
    uint64_t c;
    int64_t v;
    if (w == "value") {
      ss >> c >> v;
      idx.SetValue("bsint", c, v);
    } else if (w == "query") {
      ss >> pred >> limit >> offset >> desc;
    } else if (w == "want") {
      ss >> c >> v;
      want.push_back({c, v});
    }
  }
  EXPECT(want.size() == 2);
  Executor ex(idx);
  const Call filter = Call::Range("bsint", FBK_BSI_GT, pred);
  const SortedRow sr = ex.Sort("bsint", &filter, desc != 0, limit, offset);
  EXPECT(sr.Columns.size() == want.size());
  for (size_t k = 0; k < want.size() && k < sr.Columns.size(); ++k) EXPECT(sr.Columns[k] == want[k].first && sr.Values[k] == want[k].second);
  const ExtractedIDMatrix m = ex.ExtractSorted("bsint", &filter, desc != 0, {"bsint"}, limit, offset);
  EXPECT(m.Columns.size() == want.size());
  for (size_t k = 0; k < want.size() && k < m.Columns.size(); ++k) {
    EXPECT(m.Columns[k].ColumnID == want[k].first);
    EXPECT(m.Columns[k].Rows.size() == 1 && m.Columns[k].Rows[0] && *m.Columns[k].Rows[0] == std::vector<uint64_t>{uint64_t(want[k].second)});
  }
}

struct Rec {
  uint64_t col;
  int64_t val;
};

static std::vector<Rec> brute(const std::map<uint64_t, int64_t>& values, const std::set<uint64_t>* filter, int64_t base, bool desc, bool keep_zero,
                              uint64_t limit, uint64_t offset) {
  std::vector<Rec> all;
  for (const auto& kv : values)  // ascending column
    if ((!filter || filter->count(kv.first)) && (keep_zero || kv.second != base)) all.push_back({kv.first, kv.second});
  std::stable_sort(all.begin(), all.end(), [&](const Rec& a, const Rec& b) { return desc ? a.val > b.val : a.val < b.val; });
  const size_t lo = std::min<uint64_t>(offset, all.size());
  const size_t hi = lo + std::min<uint64_t>(limit, all.size() - lo);
  return std::vector<Rec>(all.begin() + lo, all.begin() + hi);
}

static void seeded() {
  std::mt19937_64 rng(9100);
  Index idx;
  idx.CreateIntField("v", -1000, 1000);
  idx.CreateIntField("b", 10, 100000);  // Base 10: a stored 10 has magnitude 0
  idx.CreateSetField("s");
  std::map<uint64_t, int64_t> v, b;
  std::map<uint64_t, std::set<uint64_t>> srows;  // column -> rows of s
  std::set<uint64_t> in_s1;
  const uint64_t shards[] = {0, 1, 3, 7};
  for (uint64_t sh : shards)
    for (int i = 0; i < 700; ++i) {
      const uint64_t col = (sh << 20) + (i < 200 ? uint64_t(i) : rng() % (1u << 20));
      if (rng() % 4) {
        v[col] = int64_t(rng() % 11) - 5;  // many ties, zeros among them
        idx.SetValue("v", col, v[col]);
      }
      if (rng() % 3) {
        b[col] = 10 + int64_t(rng() % 3 ? rng() % 50000 : 0);
        idx.SetValue("b", col, b[col]);
      }
      const uint64_t r = rng() % 3;
      idx.SetBit("s", r, col);
      srows[col].insert(r);
      if (r == 1) in_s1.insert(col);
    }
  Executor ex(idx);
  const Call f1 = Call::Row("s", 1);
  const uint64_t cuts[][2] = {{UINT64_MAX, 0}, {10, 0}, {25, 130}, {1, 699}, {UINT64_MAX, 1500}, {0, 3}, {7, 100000}};
  for (int fld = 0; fld < 2; ++fld)
    for (int desc = 0; desc < 2; ++desc)
      for (int kz = 0; kz < 2; ++kz)
        for (int flt = 0; flt < 2; ++flt)
          for (const auto& cut : cuts) {
            const std::map<uint64_t, int64_t>& vals = fld ? b : v;
            const std::vector<Rec> want = brute(vals, flt ? &in_s1 : nullptr, fld ? 10 : 0, desc, kz, cut[0], cut[1]);
            const SortedRow got = ex.Sort(fld ? "b" : "v", flt ? &f1 : nullptr, desc, cut[0], cut[1], kz);
            bool same = got.Columns.size() == want.size();
            for (size_t k = 0; same && k < want.size(); ++k) same = got.Columns[k] == want[k].col && got.Values[k] == want[k].val;
            EXPECT(same);
            if (cut[0] > 100) continue;
            const ExtractedIDMatrix m = ex.ExtractSorted(fld ? "b" : "v", flt ? &f1 : nullptr, desc, {"s", "v", "b"}, cut[0], cut[1], kz);
            same = m.Columns.size() == want.size();
            for (size_t k = 0; same && k < want.size(); ++k) {
              const ExtractedIDColumn& c = m.Columns[k];
              same = c.ColumnID == want[k].col && c.Rows[0] && *c.Rows[0] == std::vector<uint64_t>(srows[c.ColumnID].begin(), srows[c.ColumnID].end());
              for (int q = 0; q < 2 && same; ++q) {
                const std::map<uint64_t, int64_t>& mm = q ? b : v;
                auto it = mm.find(c.ColumnID);
                same = it == mm.end() ? !c.Rows[1 + q] : (c.Rows[1 + q] && *c.Rows[1 + q] == std::vector<uint64_t>{uint64_t(it->second)});
              }
            }
            EXPECT(same);
          }
}

int main(int argc, char** argv) {
  try {
    if (argc > 1) golden(argv[1]);
    seeded();
  } catch (const Error& e) {
    std::printf("FAIL: fbk error %d: %s\n", e.code, e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf("sort ok\n");
  return 0;
}
