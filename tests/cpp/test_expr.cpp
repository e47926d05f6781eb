// Executor::eval with fuse_calls (a call tree as ONE fbk_expr_eval / fbk_expr_count) against the node-by-node path it replaces:
// the set-operation and Count cases of tests/golden/executor_vectors.json (handed over as a text file by tests/test_cpp_expr.py),
// then a seeded index — two set fields, an int field with negative values, one with a Base — over shards 0, 1 and 3 with trees of
// Intersect / Union / Difference / Xor / Not / All, Row with a BSI condition (scans, BETWEEN, the clamped forms), Shift inside a
// tree, Precomputed, a union of 300 rows and a nesting of 12 (both beyond the limits of one program).  Both paths must give the
// same columns and counts; with fuse_calls the number of device calls per query is asserted.
//   g++ -std=c++17 -I include tests/cpp/test_expr.cpp -L featurebase_amd/csrc -lfbk
#include <cstdio>
#include <fstream>
#include <random>
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

using V = std::vector<uint64_t>;

struct Both {
  V columns;
  uint64_t count = 0;
  uint64_t calls_bitmap = 0, calls_count = 0;  // device calls of Bitmap(c) and of Count(c) with fuse_calls
};

// the query under both settings; what they give must be identical
static Both run_both(Executor& ex, const Call& c) {
  Both r;
  ex.fuse_calls = false;
  const V cols_nodes = ex.Columns(c);
  const uint64_t count_nodes = ex.Count(c);
  ex.fuse_calls = true;
  r.columns = ex.Columns(c);
  uint64_t before = ex.library_calls;
  { RowSet rows = ex.Bitmap(c); }
  r.calls_bitmap = ex.library_calls - before;
  before = ex.library_calls;
  r.count = ex.Count(c);
  r.calls_count = ex.library_calls - before;
  EXPECT(r.columns == cols_nodes);
  EXPECT(r.count == count_nodes);
  EXPECT(r.count == r.columns.size());
  return r;
}

// lines: case NAME | bit FIELD ROW COL | query OP FIELD ROW [ROW] | columns C... | count N
static void golden(const char* path) {
  std::ifstream in(path);
  EXPECT(bool(in));
  std::string line, w;
  std::unique_ptr<Index> idx;
  int cases = 0;
  Call query;
  bool is_count = false;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    ss >> w;
    if (w == "case") {
      idx.reset(new Index());
    } else if (w == "bit") {
      std::string f;
      uint64_t r, c;
      ss >> f >> r >> c;
      idx->CreateSetField(f);
      idx->SetBit(f, r, c);
    } else if (w == "query") {
      std::string op, f;
      uint64_t r;
      ss >> op >> f;
      std::vector<Call> rows;
      while (ss >> r) rows.push_back(Call::Row(f, r));
      is_count = op == "Count";
      if (is_count) query = rows[0];
      else query = Call::Nary(op == "Intersect" ? Call::kIntersect : op == "Union" ? Call::kUnion : op == "Xor" ? Call::kXor : Call::kDifference, rows);
    } else if (w == "columns" || w == "count") {
      Executor ex(*idx);
      const Both b = run_both(ex, query);
      if (w == "columns") {
        V want;
        uint64_t c;
        while (ss >> c) want.push_back(c);
        EXPECT(b.columns == want);
        EXPECT(b.calls_bitmap == 1 && b.calls_count == 1);  // one tree, one call
      } else {
        uint64_t n = 0;
        ss >> n;
        EXPECT(is_count && b.count == n);
      }
      ++cases;
    }
  }
  EXPECT(cases == 5);
}

int main(int argc, char** argv) {
  try {
    if (argc > 1) golden(argv[1]);

    std::mt19937_64 rng(4242);
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
      for (int i = 0; i < 2500; ++i) {
        const uint64_t col = (sh << 20) + rng() % (1u << 20);
        idx.SetValue("v", col, int64_t(rng() % 200001) - 100000);
        if (i % 3 == 0) idx.SetValue("based", col, 5000 + int64_t(rng() % 800000));
      }
    }
    Executor ex(idx);
    auto A = [](uint64_t r) { return Call::Row("a", r); };
    auto B = [](uint64_t r) { return Call::Row("b", r); };
    auto N = [](Call::Kind k, std::vector<Call> ch) { return Call::Nary(k, std::move(ch)); };
    const Call gt = Call::Range("v", FBK_BSI_GT, 5), neq = Call::Range("v", FBK_BSI_NEQ, -7), lte = Call::Range("based", FBK_BSI_LTE, 300000);
    const Call btw = Call::Between("v", -500, 70000), btw_based = Call::Between("based", 6000, 200000);

    // the WHERE clause of the design note: five calls node by node, one here
    const Call where = N(Call::kIntersect, {N(Call::kUnion, {A(1), A(2)}), Call::Not(B(3)), gt});
    {
      const Both b = run_both(ex, where);
      EXPECT(b.calls_bitmap == 1 && b.calls_count == 1 && b.count > 0);
      ex.fuse_calls = false;
      const uint64_t before = ex.library_calls;
      { RowSet r = ex.Bitmap(where); }
      EXPECT(ex.library_calls - before == 5);  // Union, Not, Row(v > 5), and two set operations for the Intersect of three
      ex.fuse_calls = true;
    }
    std::vector<Call> trees = {
        N(Call::kIntersect, {A(0), A(6), B(1)}),
        N(Call::kUnion, {A(0), A(1), A(2), A(3), A(4), A(5)}),
        N(Call::kDifference, {A(6), B(1), A(1), gt}),
        N(Call::kXor, {A(6), B(1), N(Call::kXor, {A(1), A(6)})}),
        Call::Not(A(6)),
        Call::Not(N(Call::kUnion, {gt, lte})),
        N(Call::kIntersect, {Call::All(), btw}),
        N(Call::kUnion, {neq, btw_based}),
        N(Call::kXor, {N(Call::kIntersect, {gt, A(6)}), N(Call::kUnion, {neq, N(Call::kDifference, {B(1), lte})})}),
        N(Call::kIntersect, {A(77), A(6)}),                                        // a row nobody set: empty
        N(Call::kUnion, {Call::Range("v", FBK_BSI_GT, 1 << 30), A(1)}),            // out of range: the empty row
        N(Call::kIntersect, {Call::Range("v", FBK_BSI_LT, 1 << 30), A(6)}),        // covers everything: the not-null row
        N(Call::kDifference, {Call::Between("v", -1000000, 1000000), Call::Between("v", 10, 5)}),
        N(Call::kUnion, {N(Call::kIntersect, {A(6)}), N(Call::kXor, {B(2)})}),     // fan-out 1
        N(Call::kUnion, {A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(0), A(77), A(2)}),  // plain rows of one field, 8 or more: fbk_fold_n
        N(Call::kDifference, {A(6), A(0), A(1), A(2), A(3), A(4), A(5), A(0), A(1)}),
        N(Call::kUnion, {A(0), A(1), A(2), A(3), A(4), A(5), A(6), B(1), A(2)}),   // two fields: the interpreter
    };
    for (const Call& t : trees) {
      const Both b = run_both(ex, t);
      EXPECT(b.calls_bitmap == 1 && b.calls_count == 1);
    }
    {  // Shift inside a tree: the shift is a call of its own (one per column shifted), its input tree one more, the outer tree one
      const Call t = N(Call::kIntersect, {Call::Shift(N(Call::kUnion, {A(1), A(2)}), 2), A(6)});
      const Both b = run_both(ex, t);
      EXPECT(b.calls_bitmap == 1 + 2 + 1);
      const Both plain = run_both(ex, N(Call::kUnion, {Call::Shift(A(6), 1), B(1)}));
      EXPECT(plain.calls_bitmap == 1 + 1);
    }
    {  // Precomputed: a Distinct evaluated beforehand enters as a row
      const SignedRows d = ex.DistinctRows("based");
      const Both b = run_both(ex, N(Call::kIntersect, {A(6), Call::Precomputed(d)}));
      EXPECT(b.calls_bitmap == 1);
      (void)run_both(ex, N(Call::kDifference, {Call::Precomputed(d), gt, Call::Not(A(6))}));
    }
    {  // beyond the limits of one program: evaluated in pieces that enter as ROW leaves
      std::vector<Call> many;
      for (int i = 0; i < 300; ++i) many.push_back(i % 50 == 7 ? B(1) : A(uint64_t(i) % 7));
      const Both wide = run_both(ex, N(Call::kUnion, many));
      EXPECT(wide.calls_bitmap == 2);  // FBK_EXPR_MAX_LEAVES leaves, then the rest
      Call deep = A(0);
      for (int i = 1; i <= 12; ++i) deep = N(i % 3 == 0 ? Call::kDifference : i % 3 == 1 ? Call::kUnion : Call::kXor, {i % 4 == 0 ? gt : A(uint64_t(i) % 7), deep});
      const Both nested = run_both(ex, deep);
      EXPECT(nested.calls_bitmap >= 2 && nested.calls_bitmap < 12);
    }
    bool threw = false;
    try {
      ex.Count(N(Call::kIntersect, {}));
    } catch (const Error&) {
      threw = true;
    }
    EXPECT(threw);
  } catch (const Error& e) {
    std::printf("FAIL fbk error %d: %s\n", e.code, e.what());
    ++failures;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("expr ok\n");
  return 0;
}
