// fbk_executor.hpp — C++ host-side mirror of the reference's per-query operators for the hot
// path, layered on the C ABI (fbk.h) and on fbk_roaring.hpp.  The Go toolchain is absent in this
// image, so this is the compiled-language host side the Go executor would be: same operator
// names, argument meaning and result ordering as
//   executeCount / executeBitmapCall(Shard)     executor.go:5839-5892, 1782-1900
//   executeIntersect/Union/Difference/XorShard  executor.go:5357, 5382, 2950, 5513 (left folds)
//   executeRowBSIGroupShard (Row(v > k) ...)     executor.go:5249-5355, field.go:2412-2482
//   executeSum / Min / Max (+ ValCount)          executor.go:2155-2275, 8438-8548
//   executePercentile                            executor.go:1310-1595
//   executeTopK (doTopK + PivotDescending)       executor.go:2357-2412, 2705-2746, bsi.go:18-62
//   executeTopN (counts; the rank cache is not mirrored)   executor.go:2776-2868
//   executeGroupBy (groupByIterator odometer)    executor.go:3918-3990, 8617-8934
//   executeExtract (+ executeLimitCall)          executor.go:4711-5046, 1027-1100
//   executeSort (+ Extract(Sort(...), ...))      executor.go:9321-9385, 4686-4700, 4762-4769
//   executeDistinct as a bitmap call + handlePreCalls (joins over a foreign index)   executor.go:1170-1230, 1809, 362-449
// Every shard of a query is evaluated in ONE device call per operator (the reference maps a
// closure over shards, executor.go:6449); the cross-shard reduce is the same associative
// arithmetic (sum of counts, ValCount.Add/Smaller/Larger, concatenation of row segments).
// A tiny in-memory Index (set fields and int fields) stands in for Holder/Field/fragment: it
// only exists to make the operators testable with the reference's own test vectors.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <optional>
#include <set>
#include <string>
#include <vector>

#include "../featurebase_amd/csrc/fbk_group_select_plan.h"  // the host rules of GroupBy's having / sort / offset / limit
#include "fbk_roaring.hpp"

namespace fbk {

struct Pair {  // cache.go Pair
  uint64_t ID = 0, Count = 0;
  bool operator==(const Pair& o) const { return ID == o.ID && Count == o.Count; }
};
struct FieldRow {  // executor.go FieldRow
  std::string Field;
  uint64_t RowID = 0;
  bool operator==(const FieldRow& o) const { return Field == o.Field && RowID == o.RowID; }
};
struct GroupCount {  // executor.go GroupCount
  std::vector<FieldRow> Group;
  uint64_t Count = 0;
  int64_t Agg = 0;
  bool operator==(const GroupCount& o) const { return Group == o.Group && Count == o.Count && Agg == o.Agg; }
};
struct GroupMinMax {  // a GroupBy record with the Min / Max of an int field (SQL MIN(x), MAX(x) ... GROUP BY): Executor::GroupByMinMax
  std::vector<FieldRow> Group;
  uint64_t Count = 0;                   // |group ∩ filter|, as GroupBy's
  int64_t Min = 0, Max = 0;             // Base added; (0, 0) when no column of the group has a value
  uint64_t MinCount = 0, MaxCount = 0;  // the columns holding Min / Max; 0: no column of the group has a value
  bool operator==(const GroupMinMax& o) const {
    return Group == o.Group && Count == o.Count && Min == o.Min && Max == o.Max && MinCount == o.MinCount && MaxCount == o.MaxCount;
  }
};
struct GroupQuantiles {  // a GroupBy record with percentiles of an int field (SQL PERCENTILE_DISC(x, p) ... GROUP BY): Executor::GroupByQuantiles
  std::vector<FieldRow> Group;
  uint64_t Count = 0;            // |group ∩ filter|, as GroupBy's
  uint64_t N = 0;                // the columns of the group that have a value
  std::vector<int64_t> Values;   // per fraction: the value at rank max(1, ceil(N * num / den)) - 1, Base added; 0 when N == 0
  std::vector<uint64_t> Counts;  // per fraction: the columns holding exactly that value; 0 when N == 0
  bool operator==(const GroupQuantiles& o) const { return Group == o.Group && Count == o.Count && N == o.N && Values == o.Values && Counts == o.Counts; }
};
struct GroupByCondition {  // having=Condition(count|sum <op> v): satisfiesCondition (executor.go:3787-3901)
  std::string subject;    // "count" | "sum"
  uint32_t op = 0;        // FBK_HAVING_*
  int64_t lo = 0, hi = 0;  // hi: the BETWEEN forms only
};
struct GroupByOptions {  // GroupBy(..., having=, sort=, offset=, limit=) (executor.go:3176-3459)
  std::optional<GroupByCondition> having;
  std::string sort;  // getSorter's string ("count desc, sum asc"); empty: no sort
  std::optional<uint64_t> offset, limit;
};
// getSorter (executor.go:3130-3162): terms split on commas, `count` | `sum` | `aggregate`, then `asc` | `desc` (default desc)
inline std::vector<fbk_groupby_term> ParseGroupBySort(const std::string& spec) {
  std::vector<fbk_groupby_term> out;
  size_t at = 0;
  for (;;) {
    const size_t comma = spec.find(',', at);
    std::string term = spec.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
    const size_t b = term.find_first_not_of(" \t\n\r"), e = term.find_last_not_of(" \t\n\r");
    term = b == std::string::npos ? "" : term.substr(b, e - b + 1);
    std::vector<std::string> parts;
    for (size_t i = 0; i < term.size();) {
      const size_t w = term.find_first_not_of(" \t\n\r", i);
      if (w == std::string::npos) break;
      const size_t we = term.find_first_of(" \t\n\r", w);
      parts.push_back(term.substr(w, we == std::string::npos ? std::string::npos : we - w));
      i = we == std::string::npos ? term.size() : we;
    }
    fbk_groupby_term t{FBK_GROUPSEL_COUNT, 1};
    if (parts.empty()) throw Error(FBK_E_INVALID, "invalid sorting directive: '" + term + "'");
    if (parts[0] == "count") t.subject = FBK_GROUPSEL_COUNT;
    else if (parts[0] == "aggregate" || parts[0] == "sum") t.subject = FBK_GROUPSEL_AGG;
    else throw Error(FBK_E_INVALID, "sorting is only supported on count, aggregate, or sum, not '" + parts[0] + "'");
    if (parts.size() > 2) throw Error(FBK_E_INVALID, "parsing sort directive: '" + term + "': too many elements");
    if (parts.size() == 2) {
      if (parts[1] == "asc") t.desc = 0;
      else if (parts[1] != "desc") throw Error(FBK_E_INVALID, "unknown sort direction '" + parts[1] + "'");
    }
    out.push_back(t);
    if (comma == std::string::npos) break;
    at = comma + 1;
  }
  return out;
}
struct ValCount {  // executor.go:8380; integer fields only
  int64_t Val = 0, Count = 0;
  ValCount Add(const ValCount& o) const { return {Val + o.Val, Count + o.Count}; }  // :8438
  ValCount Smaller(const ValCount& o) const {                                       // :8446-8468
    if (Count == 0 || (o.Val < Val && o.Count > 0)) return o;
    return {Val, Count + (Val == o.Val ? o.Count : 0)};
  }
  ValCount Larger(const ValCount& o) const {  // :8526-8548
    if (Count == 0 || (o.Val > Val && o.Count > 0)) return o;
    return {Val, Count + (Val == o.Val ? o.Count : 0)};
  }
  bool operator==(const ValCount& o) const { return Val == o.Val && Count == o.Count; }
};

// Extract's result (executor.go ExtractedIDMatrix / ExtractedIDColumn): per column one entry per field, null (no value) or a list
struct ExtractedIDColumn {
  uint64_t ColumnID = 0;
  std::vector<std::optional<std::vector<uint64_t>>> Rows;
};
struct ExtractedIDMatrix {
  std::vector<std::string> Fields;
  std::vector<ExtractedIDColumn> Columns;
};

// Sort's result (executor.go SortedRow.RowKVs): the columns in sort order and their values (Base added)
struct SortedRow {
  std::vector<uint64_t> Columns;
  std::vector<int64_t> Values;
};

// Distinct's result as rows (SignedRow{Neg, Pos}, executor.go:2034-2153): the COLUMNS of Pos are the values v >= 0, those of Neg
// the -v of the values v < 0.  Rows [0, PosShards.size()) of the batch are Pos's shards, the next NegShards.size() Neg's, EmptyRow
// has no containers.  The batch lives on the context of the Index that made it: a SignedRows (and every Call that holds one) must
// not outlive that Index.
struct SignedRows {
  std::shared_ptr<fbk_batch> batch;
  std::vector<uint64_t> PosShards, NegShards;  // ascending
  uint32_t EmptyRow = 0;
  uint32_t PosRow(uint64_t shard) const {  // the row of Pos's shard, EmptyRow where Pos has none
    auto it = std::lower_bound(PosShards.begin(), PosShards.end(), shard);
    return it != PosShards.end() && *it == shard ? uint32_t(it - PosShards.begin()) : EmptyRow;
  }
};

// A PQL bitmap call (the subset on the hot path).
struct Call {
  enum Kind { kRow, kRange, kBetween, kIntersect, kUnion, kDifference, kXor, kNot, kAll, kShift, kPrecomputed, kCompare } kind = kRow;
  std::string field;
  std::string field2;  // Compare: the right-hand int field
  uint64_t row = 0;    // Row(field=row)
  int32_t op = 0;      // FBK_BSI_* for Row(field <op> value)
  int64_t value = 0, value2 = 0;
  std::vector<Call> children;
  std::shared_ptr<const SignedRows> pre;  // Precomputed
  static Call Row(std::string f, uint64_t r) {
    Call c;
    c.kind = kRow;
    c.field = std::move(f);
    c.row = r;
    return c;
  }
  static Call Range(std::string f, int32_t op, int64_t v) {
    Call c;
    c.kind = kRange;
    c.field = std::move(f);
    c.op = op;
    c.value = v;
    return c;
  }
  // Row(field_x <op> field_y): the columns where both int fields have a value and value_x op value_y — SQL WHERE x < y, which the
  // reference's planner leaves to a row-by-row filter on the host (sql3/planner/opfilter.go:107).  One fbk_bsi_compare.
  static Call Compare(std::string fx, int32_t op, std::string fy) {
    Call c;
    c.kind = kCompare;
    c.field = std::move(fx);
    c.op = op;
    c.field2 = std::move(fy);
    return c;
  }
  static Call Between(std::string f, int64_t lo, int64_t hi) {
    Call c;
    c.kind = kBetween;
    c.field = std::move(f);
    c.value = lo;
    c.value2 = hi;
    return c;
  }
  static Call Not(Call child) {  // Not(x) = existence row \ x (executeNotShard, executor.go:5554-5604)
    Call c;
    c.kind = kNot;
    c.children.push_back(std::move(child));
    return c;
  }
  static Call All() {  // All(): the existence row (executeAllCallShard, executor.go:5606)
    Call c;
    c.kind = kAll;
    return c;
  }
  static Call Shift(Call child, int64_t n) {  // Shift(x, n=n): executeShiftShard, executor.go:5818-5836
    Call c;
    c.kind = kShift;
    c.value = n;
    c.children.push_back(std::move(child));
    return c;
  }
  // A Distinct evaluated beforehand, possibly on another index, as a leaf: row = r.Pos (handlePreCalls, executor.go:428-429).  It
  // evaluates to Pos on the evaluating index's shards, to the empty row where Pos has none.
  static Call Precomputed(const SignedRows& r) {
    Call c;
    c.kind = kPrecomputed;
    c.pre = std::make_shared<const SignedRows>(r);
    return c;
  }
  bool ContainsShift() const {
    if (kind == kShift) return true;
    for (const Call& ch : children)
      if (ch.ContainsShift()) return true;
    return false;
  }
  static Call Nary(Kind k, std::vector<Call> ch) {
    Call c;
    c.kind = k;
    c.children = std::move(ch);
    return c;
  }
};

class Index;

// One evaluated bitmap call: for every shard of the index, a row of a device batch.
class RowSet {
 public:
  RowSet() = default;
  RowSet(fbk_ctx* ctx, const fbk_batch* b, std::vector<uint32_t> rows, bool owned) : ctx_(ctx), batch_(b), rows_(std::move(rows)), owned_(owned) {}
  RowSet(RowSet&& o) noexcept { *this = std::move(o); }
  RowSet& operator=(RowSet&& o) noexcept {
    reset();
    ctx_ = o.ctx_;
    batch_ = o.batch_;
    rows_ = std::move(o.rows_);
    owned_ = o.owned_;
    o.batch_ = nullptr;
    o.owned_ = false;
    return *this;
  }
  RowSet(const RowSet&) = delete;
  RowSet& operator=(const RowSet&) = delete;
  ~RowSet() { reset(); }
  const fbk_batch* batch() const { return batch_; }
  const std::vector<uint32_t>& rows() const { return rows_; }

 private:
  void reset() {
    if (owned_ && batch_) fbk_batch_free(ctx_, const_cast<fbk_batch*>(batch_));
    batch_ = nullptr;
    owned_ = false;
  }
  fbk_ctx* ctx_ = nullptr;
  const fbk_batch* batch_ = nullptr;
  std::vector<uint32_t> rows_;
  bool owned_ = false;
};

// In-memory stand-in for Holder / Index / Field / fragment storage.
class Index {
 public:
  explicit Index(int device = 0) { check(fbk_open(device, 0, &ctx_)); }
  // A second index on a fork of `root`'s context (fbk_ctx_fork): the two share batches, so a call on one may name rows the other
  // computed (Call::Precomputed).  It is closed before `root`.
  explicit Index(Index& root) { check(fbk_ctx_fork(root.ctx_, &ctx_)); }
  ~Index() {
    for (auto& kv : sets_) fbk_batch_free(ctx_, kv.second.batch);
    for (auto& kv : ints_) fbk_batch_free(ctx_, kv.second.batch);
    fbk_close(ctx_);
  }
  Index(const Index&) = delete;
  Index& operator=(const Index&) = delete;

  void CreateSetField(const std::string& name) { sets_[name]; }
  void CreateIntField(const std::string& name, int64_t min, int64_t max) {  // OptFieldTypeInt
    IntField& f = ints_[name];
    f.min = min;
    f.max = max;
    f.base = min > 0 ? min : (max < 0 ? max : 0);  // bsiBase, field.go:2384-2391
  }
  void SetBit(const std::string& field, uint64_t row, uint64_t col) {  // Set(col, field=row)
    sets_.at(field).bits[row].insert(col);
    sets_[kExistence].bits[0].insert(col);  // IndexOptions.TrackExistence: the "_exists" field, row 0
    dirty_ = true;
  }
  void SetValue(const std::string& field, uint64_t col, int64_t value) {  // Set(col, field=value), field.go:1497-1543
    IntField& f = ints_.at(field);
    if (value < f.min || value > f.max) throw Error(FBK_E_INVALID, "value out of range");  // ErrBSIGroupValueTooLow/High
    f.values[col] = value;
    const int64_t bv = value - f.base;
    const uint64_t mag = bv < 0 ? uint64_t(-bv) : uint64_t(bv);
    const uint32_t need = mag ? 64u - uint32_t(__builtin_clzll(mag)) : 0u;  // bitDepthInt64, field.go:2507
    f.bit_depth = std::max(f.bit_depth, need);
    sets_[kExistence].bits[0].insert(col);
    dirty_ = true;
  }
  fbk_ctx* ctx() { return ctx_; }
  static constexpr const char* kExistence = "_exists";  // existenceFieldName, index.go

 private:
  friend class Executor;
  struct SetField {
    std::map<uint64_t, std::set<uint64_t>> bits;  // row id -> columns
    fbk_batch* batch = nullptr;
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> ordinal;  // (shard, row id) -> batch row
    std::vector<uint64_t> row_ids;                               // ascending (Rows(field))
    uint32_t empty_row = 0;                                      // a row with no containers
  };
  struct IntField {
    int64_t min = 0, max = 0, base = 0;
    uint32_t bit_depth = 0;
    std::map<uint64_t, int64_t> values;  // column -> value
    fbk_batch* batch = nullptr;
    std::map<uint64_t, uint32_t> base_row;  // shard -> batch row of the exists plane
    uint32_t empty_base = 0;                // an all-empty BSI fragment for shards without values
  };

  static void append_row(const std::vector<uint64_t>& cols_in_shard, uint64_t key_base, uint32_t row,
                         std::vector<fbk_container_desc>& descs, std::vector<uint8_t>& payload) {
    Bitmap bm = Bitmap::NewBitmap(cols_in_shard);
    for (size_t k = 0; k < bm.keys.size(); ++k) {
      const Container& c = bm.containers[k];
      fbk_container_desc d;
      std::memset(&d, 0, sizeof(d));
      d.key = key_base + bm.keys[k];
      d.off = payload.size();
      d.row = row;
      d.len = c.len();
      d.n = c.N();
      d.type = c.typ;
      const uint8_t* src = static_cast<const uint8_t*>(c.payload());
      payload.insert(payload.end(), src, src + c.payload_bytes());
      descs.push_back(d);
    }
  }

  // (re)build the device-resident fragments: what fragment storage + fbk_batch_upload_rbf give
  // the real system
  void Sync() {
    if (!dirty_) return;
    std::set<uint64_t> shards;
    for (auto& kv : sets_)
      for (auto& rb : kv.second.bits)
        for (uint64_t c : rb.second) shards.insert(c / ShardWidth);
    for (auto& kv : ints_)
      for (auto& cv : kv.second.values) shards.insert(cv.first / ShardWidth);
    shards_.assign(shards.begin(), shards.end());
    for (auto& kv : sets_) {
      SetField& f = kv.second;
      if (f.batch) fbk_batch_free(ctx_, f.batch);
      f.batch = nullptr;
      f.ordinal.clear();
      f.row_ids.clear();
      std::vector<fbk_container_desc> descs;
      std::vector<uint8_t> payload;
      uint32_t n_rows = 0;
      for (auto& rb : f.bits) {
        if (rb.second.empty()) continue;
        f.row_ids.push_back(rb.first);
        std::map<uint64_t, std::vector<uint64_t>> by_shard;
        for (uint64_t c : rb.second) by_shard[c / ShardWidth].push_back(c % ShardWidth);
        for (auto& sc : by_shard) {
          f.ordinal[{sc.first, rb.first}] = n_rows;
          append_row(sc.second, sc.first * 16, n_rows, descs, payload);  // keys rebased to shard*16+slot, fragment.go:318
          ++n_rows;
        }
      }
      f.empty_row = n_rows++;
      if (payload.empty()) payload.push_back(0);
      check(fbk_batch_upload(ctx_, descs.data(), descs.size(), n_rows, payload.data(), payload.size(), &f.batch));
    }
    for (auto& kv : ints_) {
      IntField& f = kv.second;
      if (f.batch) fbk_batch_free(ctx_, f.batch);
      f.batch = nullptr;
      f.base_row.clear();
      std::vector<fbk_container_desc> descs;
      std::vector<uint8_t> payload;
      uint32_t n_rows = 0;
      std::map<uint64_t, std::vector<std::pair<uint64_t, int64_t>>> by_shard;
      for (auto& cv : f.values) by_shard[cv.first / ShardWidth].push_back({cv.first % ShardWidth, cv.second - f.base});
      for (auto& sv : by_shard) {
        f.base_row[sv.first] = n_rows;
        // fragment.positionsForValue, fragment.go:619-657: exists, sign, magnitude planes
        std::vector<std::vector<uint64_t>> planes(f.bit_depth + 2);
        for (auto& cv : sv.second) {
          planes[0].push_back(cv.first);
          if (cv.second < 0) planes[1].push_back(cv.first);
          const uint64_t mag = cv.second < 0 ? uint64_t(-cv.second) : uint64_t(cv.second);
          for (uint32_t i = 0; i < f.bit_depth; ++i)
            if ((mag >> i) & 1) planes[2 + i].push_back(cv.first);
        }
        for (auto& p : planes) append_row(p, 0, n_rows++, descs, payload);
      }
      f.empty_base = n_rows;
      n_rows += f.bit_depth + 2;
      if (payload.empty()) payload.push_back(0);
      check(fbk_batch_upload(ctx_, descs.data(), descs.size(), n_rows, payload.data(), payload.size(), &f.batch));
    }
    dirty_ = false;
  }

  fbk_ctx* ctx_ = nullptr;
  std::map<std::string, SetField> sets_;
  std::map<std::string, IntField> ints_;
  std::vector<uint64_t> shards_;
  bool dirty_ = true;
};

class Executor {
 public:
  explicit Executor(Index& idx) : idx_(idx) {}

  // A call tree (Intersect / Union / Difference / Xor / Not over rows, BSI conditions and subtrees) is compiled into leaves plus a
  // postfix program and evaluated in ONE fbk_expr_eval / fbk_expr_count / fbk_expr_bsi_agg launch; false: node by node, one fbk_setop / fbk_bsi_range
  // per node as the reference's recursion does (executeBitmapCallShard, executor.go:1782).  Both give the same rows.
  bool fuse_calls = true;
  // device calls issued so far to evaluate bitmap calls (set operations, range scans, shifts, fused trees, row counts)
  uint64_t library_calls = 0;

 private:
  // The shards a query is evaluated over: the index's shards — plus, when the query contains a
  // Shift, the successor of every shard.  The reference lets the bit shifted out of a shard's last
  // column fall into a container keyed one past the segment, which Row.Columns() reports as the
  // first column of the next shard whether or not that shard holds data (row.go:366-373); here
  // that bit needs a row to land in.  (A shift moves a bit by one column, so the successor shards
  // are enough for any n < ShardWidth.)
  const std::vector<uint64_t>& shards() const { return cur_ ? *cur_ : idx_.shards_; }
  struct Scope {
    Executor& e;
    bool mine = false;
    Scope(Executor& ex, std::initializer_list<const Call*> calls) : e(ex) {
      e.idx_.Sync();
      if (e.cur_) return;
      bool shift = false;
      for (const Call* c : calls) shift = shift || (c && c->ContainsShift());
      if (!shift) return;
      std::set<uint64_t> u(e.idx_.shards_.begin(), e.idx_.shards_.end());
      for (uint64_t sh : e.idx_.shards_) u.insert(sh + 1);
      e.ext_.assign(u.begin(), u.end());
      e.cur_ = &e.ext_;
      mine = true;
    }
    ~Scope() {
      if (mine) e.cur_ = nullptr;
    }
  };
  std::vector<uint64_t> ext_;
  const std::vector<uint64_t>* cur_ = nullptr;

 public:

  // ---- bitmap calls --------------------------------------------------------------------------
  // (a RowSet of a query containing Shift has one row per shard AND successor shard: use Count /
  // Columns rather than the raw rows)
  RowSet Bitmap(const Call& c) {
    Scope sc(*this, {&c});
    return eval(c);
  }
  uint64_t Count(const Call& c) {  // executeCount: sum over shards of Row.Count()
    Scope sc(*this, {&c});
    if (fuse_calls && is_operator(c.kind)) {  // Count(tree): nothing is materialised
      std::vector<uint64_t> counts(shards().size());
      uint64_t n = 0;
      if (plain_rows_of_one_field(c)) {
        const std::vector<uint32_t> g = fold_groups(c);
        ++library_calls;
        check(fbk_fold_n_intersection_count(idx_.ctx_, fold_op(c.kind), idx_.sets_.at(c.children[0].field).batch, g.data(), counts.size(), uint32_t(c.children.size()), nullptr,
                                            nullptr, counts.data()));
        for (uint64_t x : counts) n += x;
        return n;
      }
      ExprBuild b;
      compile_root(c, b);
      ++library_calls;
      check(fbk_expr_count(idx_.ctx_, b.leaves.data(), uint32_t(b.leaves.size()), b.prog.data(), uint32_t(b.prog.size()), uint32_t(counts.size()), counts.data()));
      for (uint64_t x : counts) n += x;
      return n;
    }
    if (c.kind == Call::kCompare && !shards().empty()) {  // SELECT COUNT(*) ... WHERE x < y: the count-only form
      uint64_t n = 0;
      (void)compare(c, &n);
      return n;
    }
    RowSet r = eval(c);
    return count_rows(r);
  }
  std::vector<uint64_t> Columns(const Call& c) {  // Row.Columns() of the result, ascending
    Scope sc(*this, {&c});
    RowSet r = eval(c);
    return columns(r);
  }

  // ---- Sum / Min / Max -----------------------------------------------------------------------
  ValCount Sum(const std::string& field, const Call* filter = nullptr) {
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    const size_t n = shards().size();
    if (n == 0) return {};
    std::vector<uint32_t> base = base_rows(f);
    std::vector<int64_t> sums(n);
    std::vector<uint64_t> counts(n);
    if (filter && fuses_aggregate(*filter)) {  // Sum(tree, field=): the filter row is never materialised
      expr_aggregate(FBK_AGG_SUM, *filter, f, base, sums, counts);
    } else if (filter) {
      RowSet fr = eval(*filter);
      check(fbk_bsi_sum(idx_.ctx_, f.batch, base.data(), uint32_t(n), f.bit_depth, fr.batch(), fr.rows().data(), sums.data(), counts.data()));
    } else {
      check(fbk_bsi_sum(idx_.ctx_, f.batch, base.data(), uint32_t(n), f.bit_depth, nullptr, nullptr, sums.data(), counts.data()));
    }
    ValCount out;
    for (size_t s = 0; s < n; ++s)  // executeSumCountShard: Val = vsum + vcount*Base (executor.go:2205), reduce = Add
      out = out.Add({sums[s] + int64_t(counts[s]) * f.base, int64_t(counts[s])});
    return out;
  }
  ValCount Min(const std::string& field, const Call* filter = nullptr) { return minmax(field, filter, true); }
  ValCount Max(const std::string& field, const Call* filter = nullptr) { return minmax(field, filter, false); }

  // ---- SQL VAR / CORR ------------------------------------------------------------------------
  // aggregateVar / aggregateCorr (sql3/planner/expressionagg.go:1110-1195, 949-1047) fold every selected record into float64
  // accumulators on the planner.  Here ONE fbk_bsi_moments call gives n and the five integer sums over the columns where
  // both fields have a value (a row with a nil value is skipped, :978-981) and the filter holds; Base is applied with the
  // four identities of fbk.h in __int128 (exact while the true sums fit an int128).
  struct MomentSums {
    uint64_t n = 0;
    __int128 sum_x = 0, sum_y = 0, sum_xx = 0, sum_yy = 0, sum_xy = 0;
  };
  MomentSums Moments(const std::string& field_x, const std::string* field_y = nullptr, const Call* filter = nullptr) {
    Scope sc(*this, {filter});
    const Index::IntField& fx = idx_.ints_.at(field_x);
    const Index::IntField* fy = field_y ? &idx_.ints_.at(*field_y) : nullptr;
    const size_t n = shards().size();
    MomentSums out;
    if (n == 0) return out;
    const std::vector<uint32_t> bx = base_rows(fx), by = fy ? base_rows(*fy) : std::vector<uint32_t>();
    fbk_moments m;
    if (filter) {  // the filter goes through eval(), as Sum's non-fused path
      RowSet fr = eval(*filter);
      check(fbk_bsi_moments(idx_.ctx_, fx.batch, bx.data(), fx.bit_depth, fy ? fy->batch : nullptr, fy ? by.data() : nullptr, fy ? fy->bit_depth : 0, fr.batch(),
                            fr.rows().data(), uint32_t(n), &m));
    } else {
      check(fbk_bsi_moments(idx_.ctx_, fx.batch, bx.data(), fx.bit_depth, fy ? fy->batch : nullptr, fy ? by.data() : nullptr, fy ? fy->bit_depth : 0, nullptr,
                            nullptr, uint32_t(n), &m));
    }
    auto wide = [](const fbk_i128& v) { return __int128((unsigned __int128)(uint64_t)v.hi << 64 | v.lo); };
    const __int128 cnt = __int128(m.n), sx = wide(m.sum_x), sy = wide(m.sum_y), b = fx.base, c = fy ? fy->base : 0;
    out.n = m.n;
    out.sum_x = sx + cnt * b;
    out.sum_xx = wide(m.sum_xx) + 2 * b * sx + cnt * b * b;
    if (fy) {
      out.sum_y = sy + cnt * c;
      out.sum_yy = wide(m.sum_yy) + 2 * c * sy + cnt * c * c;
      out.sum_xy = wide(m.sum_xy) + c * sx + b * sy + cnt * b * c;
    }
    return out;
  }
  // VAR(field): the population variance as a decimal of scale 6.  n·Σx² − (Σx)² is exact in __int128, ONE division by n² in
  // double, then int64(f * 1e6): truncation toward zero (pql.FromFloat64WithScale, pql/decimal.go:370-373).  The reference sums
  // (v − mean)² in double over the records, so its own result carries that loop's rounding error (up to ~n·2^-53 of the
  // variance): the two agree to the digit on the reference's SQL tests and on small values, and may differ by a unit in the last
  // digit where the variance x 10^6 needs more than the ~16 digits a double holds.  This one is the nearer to the exact value.
  // No value when n == 0: the reference converts NaN to int64 there, which Go leaves unspecified.  (A decimal field of scale s
  // stores value * 10^s: its VAR is this one times 10^(-2s); CORR does not depend on the scale.)  Where n·Σx² or (Σx)² does not
  // fit an __int128 (deep fields with very many rows) the numerator is formed in double instead (moments_var of roaring.py stays
  // exact there: the two mirrors may differ in that range only).
  std::optional<int64_t> Var(const std::string& field, const Call* filter = nullptr) {
    const MomentSums m = Moments(field, nullptr, filter);
    if (m.n == 0) return std::nullopt;
    const __int128 cnt = __int128(m.n);
    __int128 a, b, num;
    double f;
    if (__builtin_mul_overflow(cnt, m.sum_xx, &a) || __builtin_mul_overflow(m.sum_x, m.sum_x, &b) || __builtin_sub_overflow(a, b, &num))
      f = (double(m.n) * double(m.sum_xx) - double(m.sum_x) * double(m.sum_x)) / (double(m.n) * double(m.n));
    else
      f = double(num) / (double(m.n) * double(m.n));
    return int64_t(f * 1e6);
  }
  // CORR(fx, fy): the expression of aggregateCorr.Eval (expressionagg.go:1040) in double, in its order of operations, from
  // the moments converted to double.  No value when n == 0 or when n·Σx² − (Σx)² or its y counterpart is zero (a constant
  // column): the reference converts NaN or Inf to int64 there, which Go leaves unspecified.
  std::optional<int64_t> Corr(const std::string& field_x, const std::string& field_y, const Call* filter = nullptr) {
    const MomentSums m = Moments(field_x, &field_y, filter);
    if (m.n == 0) return std::nullopt;
    const double n = double(m.n), sx = double(m.sum_x), sy = double(m.sum_y), sxy = double(m.sum_xy), sxx = double(m.sum_xx), syy = double(m.sum_yy);
    const double under = (n * sxx - sx * sx) * (n * syy - sy * sy);
    if (!(under > 0) || std::isinf(under)) return std::nullopt;
    return int64_t((n * sxy - sx * sy) / std::sqrt(under) * 1e6);
  }

  // ---- Percentile ----------------------------------------------------------------------------
  // executePercentile, executor.go:1310-1595 (integer fields).  Returns false for the "median of
  // nothing is NULL" case (:1399-1402).  One fbk_bsi_percentile call after the filter: the device
  // selects the four order statistics that fix the reference's bisection and the call replays it
  // (fbk.h) — same results as PercentileBySearch below, the reference's own procedure.
  bool Percentile(const std::string& field, double nth, const Call* filter, ValCount* out) {
    const std::vector<ValCount> r = Percentiles(field, {nth}, filter);
    if (r[0].Count == 0) return false;
    *out = r[0];
    return true;
  }
  // Percentile for a list of nth in ONE call (one select over the planes); Count == 0: the median of nothing.
  std::vector<ValCount> Percentiles(const std::string& field, const std::vector<double>& nth, const Call* filter = nullptr) {
    for (double x : nth)
      if (!(x >= 0 && x <= 100.0)) throw Error(FBK_E_INVALID, "Percentile(): invalid nth value, should be a number between 0 and 100 inclusive");
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    const size_t n = shards().size();
    std::vector<ValCount> out(nth.size());
    if (n == 0 || nth.empty()) return out;
    const std::vector<uint32_t> base = base_rows(f);
    std::optional<RowSet> fr;
    if (filter) fr.emplace(eval(*filter));
    std::vector<int64_t> vals(nth.size());
    std::vector<uint64_t> cnts(nth.size());
    uint64_t total = 0;
    check(fbk_bsi_percentile(idx_.ctx_, f.batch, base.data(), f.bit_depth, fr ? fr->batch() : nullptr, fr ? fr->rows().data() : nullptr, uint32_t(n), f.base,
                             nth.data(), uint32_t(nth.size()), vals.data(), cnts.data(), &total));
    for (size_t i = 0; i < nth.size(); ++i) out[i] = ValCount{cnts[i] ? vals[i] : 0, int64_t(cnts[i])};
    return out;
  }
  // The values (Base added) at ascending ranks of exists ∩ filter, FBK_RANK_FROM_TOP | k counting from the largest, and the
  // number of columns holding each; a rank past the end gives {0, 0}.  One fbk_bsi_quantiles call.  Stored zeros take part.
  std::vector<ValCount> Quantiles(const std::string& field, const std::vector<uint64_t>& ranks, const Call* filter = nullptr, uint64_t* out_total = nullptr) {
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    const size_t n = shards().size();
    std::vector<ValCount> out(ranks.size());
    if (out_total) *out_total = 0;
    if (n == 0) return out;
    const std::vector<uint32_t> base = base_rows(f);
    std::optional<RowSet> fr;
    if (filter) fr.emplace(eval(*filter));
    std::vector<int64_t> vals(ranks.size());
    std::vector<uint64_t> cnts(ranks.size());
    uint64_t total = 0;
    check(fbk_bsi_quantiles(idx_.ctx_, f.batch, base.data(), f.bit_depth, fr ? fr->batch() : nullptr, fr ? fr->rows().data() : nullptr, uint32_t(n),
                            ranks.data(), uint32_t(ranks.size()), vals.data(), cnts.data(), &total));
    if (out_total) *out_total = total;
    for (size_t i = 0; i < ranks.size(); ++i) out[i] = ValCount{cnts[i] ? vals[i] + f.base : 0, int64_t(cnts[i])};
    return out;
  }
  // The reference's procedure itself: binary search between Min and Max on Count(Row(field < x) ∩ filter) /
  // Count(Row(field > x) ∩ filter), one or two fbk_bsi_range calls per step.  The in-tree cross-check of Percentile.
  bool PercentileBySearch(const std::string& field, double nth, const Call* filter, ValCount* out) {
    if (nth < 0 || nth > 100.0) throw Error(FBK_E_INVALID, "Percentile(): invalid nth value, should be a number between 0 and 100 inclusive");
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    auto count_of = [&](RowSet&& r) {
      if (!filter) return count_rows(r);
      RowSet fr = eval(*filter);
      RowSet both = setop(FBK_OP_AND, r, fr);
      return count_rows(both);
    };
    const uint64_t total = count_of(not_null(f));  // Count(Intersect(filter, Row(field != null)))
    if (total == 0) return false;
    const uint64_t desired_less = uint64_t((double(total) * nth) / 100.0);
    const uint64_t desired_greater = uint64_t((double(total) * (100 - nth)) / 100.0);
    ValCount mn;
    if (desired_greater != 0) {
      mn = Min(field, filter);
      if (desired_less == 0) {
        *out = mn;
        return true;
      }
    }
    const ValCount mx = Max(field, filter);
    if (desired_greater == 0) {
      *out = mx;
      return true;
    }
    int64_t lo = mn.Val, hi = mx.Val, guess = mn.Val;
    while (lo < hi) {
      guess = (lo / 2) + (hi / 2) + (((lo % 2) + (hi % 2)) / 2);  // average without overflow (:1497-1501)
      const uint64_t left = count_of(range(Call::Range(field, FBK_BSI_LT, guess)));
      if (left > desired_less) {
        hi = guess - 1;
        continue;
      }
      const uint64_t right = count_of(range(Call::Range(field, FBK_BSI_GT, guess)));
      if (right > desired_greater) {
        lo = guess + 1;
        continue;
      }
      break;
    }
    *out = ValCount{guess, 1};
    return true;
  }

  // ---- Distinct -----------------------------------------------------------------------------
  // Distinct(field=int field, filter): the distinct values (Base added) in ascending order —
  // the SignedRow{Neg, Pos} of executeDistinct (executor.go:1170-1230, 2034-2153) flattened.
  std::vector<int64_t> Distinct(const std::string& field, const Call* filter = nullptr) {
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    std::vector<int64_t> out;
    const size_t n = shards().size();
    if (n == 0) return out;
    std::vector<uint32_t> base = base_rows(f);
    uint64_t cnt = 0, cap = 1024;
    for (;;) {
      out.assign(cap, 0);
      int32_t rc;
      if (filter) {
        RowSet fr = eval(*filter);
        rc = fbk_bsi_distinct(idx_.ctx_, f.batch, base.data(), uint32_t(n), f.bit_depth, fr.batch(), fr.rows().data(), out.data(), cap, &cnt);
      } else {
        rc = fbk_bsi_distinct(idx_.ctx_, f.batch, base.data(), uint32_t(n), f.bit_depth, nullptr, nullptr, out.data(), cap, &cnt);
      }
      if (rc == FBK_E_CAPACITY) {
        cap = cnt;
        continue;
      }
      check(rc);
      break;
    }
    out.resize(cnt);
    for (int64_t& v : out) v += f.base;  // value += int64(offset), executor.go:2126
    return out;
  }

  // Distinct(field=int field, filter) as a bitmap call: SignedRow{Neg, Pos} left on the device (fbk_bsi_distinct_rows), the operand
  // of a join (Call::Precomputed).  A field whose values span more shards of a row than the call takes (or of bit depth 64) goes
  // through Distinct() and an upload instead.
  SignedRows DistinctRows(const std::string& field, const Call* filter = nullptr) {
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    const size_t n = shards().size();
    std::vector<uint32_t> base = base_rows(f);
    std::optional<RowSet> fr;
    if (filter) fr.emplace(eval(*filter));
    SignedRows out;
    fbk_batch* b = nullptr;
    uint32_t n_pos = 0, n_neg = 0;
    std::vector<uint64_t> ids(64);
    for (;;) {
      const int32_t rc = fbk_bsi_distinct_rows(idx_.ctx_, f.batch, base.data(), f.bit_depth, f.base, fr ? fr->batch() : nullptr, fr ? fr->rows().data() : nullptr,
                                               uint32_t(n), FBK_SETOP_OPTIMIZE, &b, ids.data(), ids.size(), &n_pos, &n_neg, nullptr);
      if (rc == FBK_E_CAPACITY) {
        ids.assign(size_t(n_pos) + n_neg, 0);
        continue;
      }
      if (rc == FBK_E_INVALID && std::string(fbk_last_error(nullptr)).find("fbk_bsi_distinct") != std::string::npos) {  // (the message names the way out)
        b = nullptr;
        break;
      }
      check(rc);
      break;
    }
    if (!b) {
      std::map<uint64_t, std::vector<uint64_t>> by_shard[2];  // Pos, Neg
      for (int64_t v : Distinct(field, filter)) {
        const uint64_t p = v < 0 ? 0 - uint64_t(v) : uint64_t(v);
        by_shard[v < 0][p / ShardWidth].push_back(p % ShardWidth);
      }
      std::vector<fbk_container_desc> descs;
      std::vector<uint8_t> payload;
      ids.clear();
      for (auto& sign : by_shard)
        for (auto& sc2 : sign) {
          Index::append_row(sc2.second, sc2.first * 16, uint32_t(ids.size()), descs, payload);
          ids.push_back(sc2.first);
        }
      n_pos = uint32_t(by_shard[0].size()), n_neg = uint32_t(by_shard[1].size());
      if (payload.empty()) payload.push_back(0);
      check(fbk_batch_upload(idx_.ctx_, descs.data(), descs.size(), n_pos + n_neg + 1, payload.data(), payload.size(), &b));
    }
    fbk_ctx* ctx = idx_.ctx_;
    out.batch = std::shared_ptr<fbk_batch>(b, [ctx](fbk_batch* x) { fbk_batch_free(ctx, x); });
    out.PosShards.assign(ids.begin(), ids.begin() + n_pos);
    out.NegShards.assign(ids.begin() + n_pos, ids.begin() + n_pos + n_neg);
    out.EmptyRow = n_pos + n_neg;
    return out;
  }
  // the values a DistinctRows result stands for, ascending (Neg's columns negated): what Distinct() lists
  std::vector<int64_t> Values(const SignedRows& r) {
    std::vector<int64_t> out;
    const size_t n_pos = r.PosShards.size(), n = n_pos + r.NegShards.size();
    if (n == 0) return out;
    std::vector<uint32_t> rows(n);
    for (size_t i = 0; i < n; ++i) rows[i] = uint32_t(i);
    for_each_bit(r.batch.get(), rows, [&](uint32_t i, uint64_t p) {
      out.push_back(i < n_pos ? int64_t(r.PosShards[i] * ShardWidth + p) : int64_t(0 - (r.NegShards[i - n_pos] * ShardWidth + p)));
    });
    std::sort(out.begin(), out.end());
    return out;
  }

  // ---- TopK / TopN ---------------------------------------------------------------------------
  // TopK(field, k, filter): per-row |row ∩ filter| over all shards (doTopK), then the rows in
  // descending count order, ascending id inside one count, zero counts dropped
  // (BSIData.PivotDescending, bsi.go:18-62).  k == 0: no limit.
  // Counting, the reduce over shards and the ordering all happen on the device (fbk_topk): only
  // the k winners come back.
  std::vector<Pair> TopK(const std::string& field, uint64_t k, const Call* filter = nullptr) {
    Scope sc(*this, {filter});
    const Index::SetField& f = idx_.sets_.at(field);
    const size_t n = shards().size(), nr = f.row_ids.size();
    std::vector<Pair> out;
    if (n == 0 || nr == 0) return out;
    const std::vector<uint32_t> rows_a = field_rows(f);
    const uint32_t cap = uint32_t(k && k < nr ? k : nr);
    std::vector<uint32_t> idx(cap);
    std::vector<uint64_t> cnt(cap);
    uint32_t got = 0;
    if (filter && fuses_topk(*filter, n, nr)) {  // TopK(field, filter=tree): the filter row is never materialised (fbk_expr_topk)
      ExprBuild b;
      compile_root(*filter, b);
      ++library_calls;
      check(fbk_expr_topk(idx_.ctx_, b.leaves.data(), uint32_t(b.leaves.size()), b.prog.data(), uint32_t(b.prog.size()), f.batch, rows_a.data(), uint32_t(nr),
                          uint32_t(n), uint32_t(cap == nr ? 0 : cap), idx.data(), cnt.data(), cap, &got));
    } else if (filter) {
      RowSet fr = eval(*filter);
      check(fbk_topk(idx_.ctx_, f.batch, rows_a.data(), uint32_t(nr), fr.batch(), fr.rows().data(), uint32_t(n), uint32_t(cap == nr ? 0 : cap),
                     idx.data(), cnt.data(), cap, &got));
    } else {
      check(fbk_topk(idx_.ctx_, f.batch, rows_a.data(), uint32_t(nr), nullptr, nullptr, uint32_t(n), uint32_t(cap == nr ? 0 : cap), idx.data(),
                     cnt.data(), cap, &got));
    }
    for (uint32_t i = 0; i < got; ++i) out.push_back({f.row_ids[idx[i]], cnt[i]});  // row_ids ascending: index order = id order
    return out;
  }
  // TopN(field, n, src): the same counts ordered by Pairs.Less (count descending; the reference's
  // tie order is unspecified, cache.go:436, here ascending id); the rank-cache thresholds of
  // fragment.top (fragment.go:1340-1426) are approximations the GPU path does not need.
  std::vector<Pair> TopN(const std::string& field, uint64_t n, const Call* src = nullptr) { return TopK(field, n, src); }

  // ---- GroupBy -------------------------------------------------------------------------------
  // GroupBy(Rows(f0), Rows(f1), ..., filter, aggregate=Sum(field=agg)): odometer order over the
  // ascending row ids of each field (last field fastest), groups with Count == 0 skipped
  // (groupByIterator.Next, executor.go:8880-8934); limit == 0: no limit.
  std::vector<GroupCount> GroupBy(const std::vector<std::string>& fields, const Call* filter = nullptr,
                                  const std::string& agg_field = "", uint64_t limit = 0) {
    if (fields.empty()) throw Error(FBK_E_INVALID, "need at least one child call");  // executor.go:3927
    Scope sc(*this, {filter});
    std::vector<GroupCount> out;
    const size_t n = shards().size();
    if (n == 0) return out;
    std::unique_ptr<RowSet> prefix;  // filter ∩ rows of the fields before the last two
    if (filter) prefix.reset(new RowSet(eval(*filter)));
    std::vector<FieldRow> group;
    GroupAgg agg;
    agg.sum_field = agg_field;
    group_by_rec(fields, 0, prefix.get(), agg, limit, group, out);
    return out;
  }

  // GroupBy(..., having=Condition(...), sort="...", offset=, limit=) (executeGroupBy, executor.go:3176-3459).  When the whole GroupBy
  // fits ONE library call — one to three fields of at most kSumBlock rows within the cube's 2^24 groups, or aggregate=Sum over one
  // or two fields whose Base is 0 (the call's aggregate is the sum without Base) — the matching fbk_*_select call selects on the
  // device and only the winners come back; otherwise today's blocked path runs and fbk_group_select::select picks on the host.
  // Two quirks of the reference are reproduced HERE (the C ABI has neither): with neither sort nor having the limit is applied
  // while merging and then offset and limit again (:3302, :3331: limit=L, offset=O yields the groups O .. L-1), and an offset >=
  // the number of results is ignored (:3446).  A negative literal in a count condition matches nothing (:3792-3795).
  std::vector<GroupCount> GroupBy(const std::vector<std::string>& fields, const Call* filter, const std::string& agg_field, const GroupByOptions& opt) {
    if (fields.empty()) throw Error(FBK_E_INVALID, "need at least one child call");  // executor.go:3927
    fbk_groupby_select sel{};
    if (!opt.sort.empty())
      for (const fbk_groupby_term& t : ParseGroupBySort(opt.sort)) {
        bool seen = false;
        for (uint32_t k = 0; k < sel.n_sort; ++k) seen = seen || sel.sort[k].subject == t.subject;
        if (!seen) sel.sort[sel.n_sort++] = t;  // (a repeated subject never decides; count and sum: at most two terms stay)
      }
    if (opt.having) {
      const GroupByCondition& h = *opt.having;
      if (h.subject != "count" && h.subject != "sum") throw Error(FBK_E_INVALID, "Condition() only supports count or sum");
      if (h.op < FBK_HAVING_EQ || h.op > FBK_HAVING_BTWN_LT_LT) throw Error(FBK_E_INVALID, "Condition(): unknown operator");
      sel.having_subject = h.subject == "count" ? FBK_GROUPSEL_COUNT : FBK_GROUPSEL_AGG;
      sel.having_op = h.op, sel.having_lo = h.lo, sel.having_hi = h.hi;
      if (h.subject == "count" && (h.lo < 0 || (h.op >= FBK_HAVING_BETWEEN && h.hi < 0))) return {};  // Uint64Value fails: nothing matches
    }
    const bool plain = sel.n_sort == 0 && !opt.having;
    uint64_t offset = opt.offset.value_or(0), limit = opt.limit.value_or(UINT64_MAX);
    if (plain && opt.limit) {  // the merge kept the first L groups; offset and limit again on those
      if (offset >= limit) offset = 0;
      else limit -= offset;
    }
    Scope sc(*this, {filter});
    std::vector<GroupCount> out;
    const size_t n = shards().size();
    if (n == 0) return out;
    std::unique_ptr<RowSet> prefix;
    if (filter) prefix.reset(new RowSet(eval(*filter)));
    const fbk_batch* fb_ = prefix ? prefix->batch() : nullptr;
    const uint32_t* fr_ = prefix ? prefix->rows().data() : nullptr;
    std::vector<const Index::SetField*> fs;
    uint64_t cells = 1;
    bool fits = fields.size() <= 3;
    for (const std::string& name : fields) {
      fs.push_back(&idx_.sets_.at(name));
      const uint64_t nr = fs.back()->row_ids.size();
      if (nr == 0) return out;
      fits = fits && nr <= kSumBlock;
      cells *= std::min<uint64_t>(nr, uint64_t(1) << 25);
      fits = fits && cells <= kCubeCells;
    }
    const Index::IntField* af = agg_field.empty() ? nullptr : &idx_.ints_.at(agg_field);
    if (af) fits = fits && fields.size() <= 2 && af->base == 0;
    if (!af && fields.size() == 1 && !prefix) fits = false;  // (the one-field count form takes the filter row as its B: without one, fbk_count's totals)
    sel.offset = offset, sel.limit = limit;
    // measured (docs/history/DESIGN_groupby_select_measurements.md): under 2^17 cells a sort that keeps a handful of groups is faster on
    // the host (251 against 362 us at 2^16 cells, limit 10; even at 2^17): the radix select's 16 launches per term cost more than the transfer
    if (sel.n_sort && cells <= (uint64_t(1) << 17) && limit <= 64 && offset <= 64) sel.flags = FBK_GROUPSEL_HOST;
    if (const char* what = fbk_group_select::check(&sel, af != nullptr)) throw Error(FBK_E_INVALID, std::string("GroupBy: ") + what);

    std::vector<uint32_t> cell;
    std::vector<uint64_t> cnt;
    std::vector<int64_t> agg;
    if (fits) {
      std::vector<std::vector<uint32_t>> rows;
      for (const Index::SetField* f : fs) rows.push_back(field_rows(*f));
      const std::vector<uint32_t> base = af ? base_rows(*af) : std::vector<uint32_t>();
      auto call = [&](uint64_t cap, uint64_t* out_n, uint64_t* matched) -> int32_t {
        cell.assign(cap, 0), cnt.assign(cap, 0);
        if (af) agg.assign(cap, 0);
        const uint32_t r0 = uint32_t(fs[0]->row_ids.size()), r1 = fs.size() > 1 ? uint32_t(fs[1]->row_ids.size()) : 1;
        if (af)
          return fbk_count_matrix_sum_select(idx_.ctx_, fs[0]->batch, rows[0].data(), r0, fs.size() > 1 ? fs[1]->batch : nullptr,
                                             fs.size() > 1 ? rows[1].data() : nullptr, r1, fb_, fr_, af->batch, base.data(), af->bit_depth, uint32_t(n), &sel,
                                             cell.data(), cnt.data(), agg.data(), cap, out_n, matched);
        if (fs.size() == 3)
          return fbk_count_cube_select(idx_.ctx_, fs[0]->batch, rows[0].data(), r0, fs[1]->batch, rows[1].data(), r1, fs[2]->batch, rows[2].data(),
                                       uint32_t(fs[2]->row_ids.size()), fb_, fr_, uint32_t(n), &sel, cell.data(), cnt.data(), cap, out_n, matched);
        if (fs.size() == 2)
          return fbk_count_matrix_select(idx_.ctx_, fs[0]->batch, rows[0].data(), r0, fs[1]->batch, rows[1].data(), r1, fb_, fr_, uint32_t(n), &sel, cell.data(),
                                         cnt.data(), cap, out_n, matched);
        return fbk_count_matrix_select(idx_.ctx_, fs[0]->batch, rows[0].data(), r0, fb_, fr_, 1, nullptr, nullptr, uint32_t(n), &sel, cell.data(), cnt.data(), cap,
                                       out_n, matched);
      };
      uint64_t got = 0, matched = 0, cap = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(limit, 1 << 16), cells));
      int32_t rc = call(cap, &got, &matched);
      if (rc == FBK_OK && got == 0 && matched > 0 && sel.offset >= matched) {  // applyLimitAndOffsetToGroupByResult ignores such an offset
        sel.offset = 0;
        if (plain && opt.limit) sel.limit = *opt.limit;
        rc = call(cap, &got, &matched);
      }
      if (rc == FBK_E_CAPACITY) rc = call(got, &got, &matched);
      check(rc);
      cell.resize(got);
    } else {
      GroupAgg ga;
      ga.sum_field = agg_field;
      std::vector<FieldRow> group;
      std::vector<GroupCount> all;
      group_by_rec(fields, 0, prefix.get(), ga, 0, group, all);
      std::vector<uint64_t> c(all.size());
      std::vector<int64_t> a(all.size());
      for (size_t k = 0; k < all.size(); ++k) c[k] = all[k].Count, a[k] = all[k].Agg;
      uint64_t matched = fbk_group_select::select(c.data(), af ? a.data() : nullptr, c.size(), sel, cell);
      if (cell.empty() && matched > 0 && sel.offset >= matched) {
        sel.offset = 0;
        if (plain && opt.limit) sel.limit = *opt.limit;
        fbk_group_select::select(c.data(), af ? a.data() : nullptr, c.size(), sel, cell);
      }
      for (uint32_t k : cell) out.push_back(std::move(all[k]));
      return out;
    }
    for (size_t k = 0; k < cell.size(); ++k) {
      GroupCount g;
      uint64_t rest = cell[k];
      g.Group.resize(fs.size());
      for (size_t f = fs.size(); f-- > 0;) {  // odometer order, the last field fastest
        const uint64_t nr = fs[f]->row_ids.size();
        g.Group[f] = {fields[f], fs[f]->row_ids[rest % nr]};
        rest /= nr;
      }
      g.Count = cnt[k];
      g.Agg = af ? agg[k] : 0;  // (Base is 0 on this path)
      out.push_back(std::move(g));
    }
    return out;
  }

  // GroupBy(Rows(f0), Rows(f1), ..., filter, aggregate=Count(Distinct(distinct_filter, field=distinct_field))): the groups of
  // GroupBy (Count = |group ∩ filter|, Count == 0 skipped, odometer order, limit), Agg = the number of distinct values of the
  // int field over group ∩ filter ∩ distinct_filter (0 when the group has none) — executor.go:3338-3386.  The last one or two
  // levels take one fbk_count_matrix_distinct call per block of rows.  Int fields only.
  std::vector<GroupCount> GroupByCountDistinct(const std::vector<std::string>& fields, const Call* filter, const std::string& distinct_field,
                                               const Call* distinct_filter = nullptr, uint64_t limit = 0) {
    if (fields.empty()) throw Error(FBK_E_INVALID, "need at least one child call");  // executor.go:3927
    if (!idx_.ints_.count(distinct_field))
      throw Error(FBK_E_INVALID, "GroupBy aggregate=Count(Distinct(field=" + distinct_field + ")): " +
                                     (idx_.sets_.count(distinct_field) ? "set fields are not supported, only int fields" : "no such int field"));
    Scope sc(*this, {filter, distinct_filter});
    std::vector<GroupCount> out;
    if (shards().empty()) return out;
    std::unique_ptr<RowSet> prefix, dfilt;
    if (filter) prefix.reset(new RowSet(eval(*filter)));
    if (distinct_filter) dfilt.reset(new RowSet(eval(*distinct_filter)));
    std::vector<FieldRow> group;
    GroupAgg agg;
    agg.distinct_field = distinct_field;
    agg.distinct_filter = dfilt.get();
    group_by_rec(fields, 0, prefix.get(), agg, limit, group, out);
    return out;
  }

  // GroupBy(Rows(f0), Rows(f1), ..., filter) with the Min and the Max of an int field per group — what SQL's
  // SELECT f0, f1, MIN(x), MAX(x) ... GROUP BY f0, f1 asks for (the reference's planner refuses it: sql3/planner/oppqlgroupby.go:188-195).
  // The groups are GroupBy's (Count = |group ∩ filter|, Count == 0 skipped, odometer order, limit); Min / Max = the smallest /
  // largest value of the field over group ∩ filter, Base added, with the number of columns holding each (fragment.min / .max per
  // shard folded by ValCount.Smaller / Larger, executor.go:8446-8548).  The last one or two levels take one
  // fbk_count_matrix_minmax call per block of kSumBlock x kSumBlock rows; earlier levels fix their row (prefix ∩ row) as
  // GroupByCountDistinct does.
  std::vector<GroupMinMax> GroupByMinMax(const std::vector<std::string>& fields, const Call* filter, const std::string& agg_field, uint64_t limit = 0) {
    if (fields.empty()) throw Error(FBK_E_INVALID, "need at least one child call");  // executor.go:3927
    if (!idx_.ints_.count(agg_field))
      throw Error(FBK_E_INVALID, "GroupBy Min / Max(field=" + agg_field + "): " +
                                     (idx_.sets_.count(agg_field) ? "set fields are not supported, only int fields" : "no such int field"));
    Scope sc(*this, {filter});
    std::vector<GroupMinMax> out;
    if (shards().empty()) return out;
    std::unique_ptr<RowSet> prefix;
    if (filter) prefix.reset(new RowSet(eval(*filter)));
    std::vector<FieldRow> group;
    last_levels_rec(fields, 0, prefix.get(), group, [&](size_t level, const Index::SetField& fa, const std::vector<uint32_t>& rows_a, const Index::SetField* fb,
                                                       const std::vector<uint32_t>* rows_b, const RowSet* pre, const std::vector<uint64_t>& tot) {
      const size_t na = fa.row_ids.size(), nb = fb ? fb->row_ids.size() : 1;
      std::vector<int64_t> mins, maxs;
      std::vector<uint64_t> cmin, cmax;
      minmax_matrix(agg_field, fa, rows_a, fb, rows_b, pre, mins, maxs, cmin, cmax);
      for (size_t i = 0; i < na; ++i)
        for (size_t j = 0; j < nb; ++j) {
          const size_t k = i * nb + j;
          if (!tot[k]) continue;  // groupByIterator.Next skips Count == 0 (executor.go:8905-8913)
          GroupMinMax g;
          g.Group = group;
          g.Group.push_back({fields[level], fa.row_ids[i]});
          if (fb) g.Group.push_back({fields[level + 1], fb->row_ids[j]});
          g.Count = tot[k], g.Min = mins[k], g.Max = maxs[k], g.MinCount = cmin[k], g.MaxCount = cmax[k];
          out.push_back(std::move(g));
          if (limit && out.size() >= limit) return false;
        }
      return true;
    });
    return out;
  }

  // GroupBy(Rows(f0), Rows(f1), ..., filter) with percentiles of an int field per group — SQL's SELECT f0, f1, PERCENTILE_DISC(x, p)
  // ... GROUP BY f0, f1 (the reference evaluates it row by row on the host).  The groups are GroupBy's (Count = |group ∩ filter|,
  // Count == 0 skipped, odometer order, limit).  Per fraction (num, den): with s the ascending values of the field over group ∩
  // filter and N their number, s[max(1, ceil(N * num / den)) - 1] with Base added, and the number of columns holding it; a group
  // without a value has N == 0 and zeros.  At most 16 fractions, den <= 2^20.  The last one or two levels take one
  // fbk_count_matrix_quantiles call per block of kSumBlock x kSumBlock rows (rows of the leading field fewer where the call's
  // histogram scratch asks for it); earlier levels fix their row as GroupByMinMax does.
  std::vector<GroupQuantiles> GroupByQuantiles(const std::vector<std::string>& fields, const Call* filter, const std::string& agg_field,
                                               const std::vector<std::pair<uint32_t, uint32_t>>& fractions, uint64_t limit = 0) {
    if (fields.empty()) throw Error(FBK_E_INVALID, "need at least one child call");  // executor.go:3927
    if (!idx_.ints_.count(agg_field))
      throw Error(FBK_E_INVALID, "GroupBy Percentile(field=" + agg_field + "): " +
                                     (idx_.sets_.count(agg_field) ? "set fields are not supported, only int fields" : "no such int field"));
    Scope sc(*this, {filter});
    std::vector<GroupQuantiles> out;
    if (shards().empty()) return out;
    std::unique_ptr<RowSet> prefix;
    if (filter) prefix.reset(new RowSet(eval(*filter)));
    std::vector<FieldRow> group;
    const size_t nq = fractions.size();
    last_levels_rec(fields, 0, prefix.get(), group, [&](size_t level, const Index::SetField& fa, const std::vector<uint32_t>& rows_a, const Index::SetField* fb,
                                                       const std::vector<uint32_t>* rows_b, const RowSet* pre, const std::vector<uint64_t>& tot) {
      const size_t na = fa.row_ids.size(), nb = fb ? fb->row_ids.size() : 1;
      std::vector<int64_t> vals;
      std::vector<uint64_t> cnts, ns;
      quantile_matrix(agg_field, fractions, fa, rows_a, fb, rows_b, pre, vals, cnts, ns);
      for (size_t i = 0; i < na; ++i)
        for (size_t j = 0; j < nb; ++j) {
          const size_t k = i * nb + j;
          if (!tot[k]) continue;  // groupByIterator.Next skips Count == 0 (executor.go:8905-8913)
          GroupQuantiles g;
          g.Group = group;
          g.Group.push_back({fields[level], fa.row_ids[i]});
          if (fb) g.Group.push_back({fields[level + 1], fb->row_ids[j]});
          g.Count = tot[k], g.N = ns[k];
          g.Values.assign(vals.begin() + k * nq, vals.begin() + (k + 1) * nq), g.Counts.assign(cnts.begin() + k * nq, cnts.begin() + (k + 1) * nq);
          out.push_back(std::move(g));
          if (limit && out.size() >= limit) return false;
        }
      return true;
    });
    return out;
  }

  // ---- Extract --------------------------------------------------------------------------------
  // Extract(Limit(filter, limit=, offset=), Rows(f0), Rows(f1), ...) (executeExtract, executor.go:4711-5046; executeLimitCall,
  // :1027-1100): the filter's columns in ascending order, offset then limit, and per column one entry per field:
  //   int field   [value + Base] as uint64(int64) (:5023), or null when the column has no value;
  //   set field   the row ids ascending; a column with no bit gets an EMPTY, non-null list (the reference's branch for set fields
  //               without existence tracking, :4836-4842 — this mirror has no per-field existence view).
  // One fbk_extract_open for the filter, then one fbk_extract_bsi per int field and one fbk_extract_rows per block of kSumBlock
  // rows of a set field (the per-column lists concatenated in block order, as GroupByCountDistinct blocks wide fields).
  ExtractedIDMatrix Extract(const Call& filter, const std::vector<std::string>& fields, uint64_t limit = UINT64_MAX, uint64_t offset = 0) {
    for (const std::string& name : fields)
      if (!idx_.sets_.count(name) && !idx_.ints_.count(name)) throw Error(FBK_E_INVALID, "field not found: " + name);  // ErrFieldNotFound
    Scope sc(*this, {&filter});
    ExtractedIDMatrix out;
    out.Fields = fields;
    const size_t n = shards().size();
    if (n == 0) return out;
    RowSet fr = eval(filter);
    ExtractHandle hd{idx_.ctx_};
    uint64_t cnt = 0;
    check(fbk_extract_open(idx_.ctx_, fr.batch(), fr.rows().data(), shards().data(), uint32_t(n), offset, limit, &hd.h, &cnt));
    std::vector<uint64_t> cols(cnt);
    check(fbk_extract_columns(idx_.ctx_, hd.h, cols.data()));
    fill_fields(hd.h, cols, nullptr, fields, out);
    return out;
  }

  // ---- Sort -----------------------------------------------------------------------------------
  // Sort(filter, field=, sort-desc=, limit=, offset=) (executeSort, executor.go:9321-9385): the columns of exists ∩ filter in the
  // order of the field's value, offset then limit; Values carry Base.  Int, decimal and timestamp fields are all BSI fields and
  // share this path (the mirror stores their integer form).  One fbk_bsi_sort over every shard: the device selects the
  // offset + limit smallest, only the records of the result come back.  Columns of equal value come in ascending id (the
  // reference: unspecified); a stored value equal to Base does not take part unless keep_zero (the reference's behaviour, fbk.h).
  SortedRow Sort(const std::string& field, const Call* filter = nullptr, bool desc = false, uint64_t limit = UINT64_MAX, uint64_t offset = 0,
                 bool keep_zero = false) {
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    SortedRow out;
    const size_t n = shards().size();
    if (n == 0) return out;
    const std::vector<uint32_t> base = base_rows(f);
    std::optional<RowSet> fr;
    if (filter) fr.emplace(eval(*filter));
    const uint32_t flags = (desc ? FBK_SORT_DESC : 0u) | (keep_zero ? FBK_SORT_KEEP_ZERO : 0u);
    uint64_t cnt = 0, cap = limit < 4096 ? limit : 4096;
    for (;;) {
      out.Columns.assign(cap, 0);
      out.Values.assign(cap, 0);
      const int32_t rc = fbk_bsi_sort(idx_.ctx_, f.batch, base.data(), f.bit_depth, fr ? fr->batch() : nullptr, fr ? fr->rows().data() : nullptr,
                                      shards().data(), uint32_t(n), flags, offset, limit, out.Columns.data(), out.Values.data(), cap, &cnt, nullptr);
      if (rc == FBK_E_CAPACITY) {
        cap = cnt;
        continue;
      }
      check(rc);
      break;
    }
    out.Columns.resize(cnt);
    out.Values.resize(cnt);
    for (int64_t& v : out.Values) v += f.base;
    return out;
  }

  // Extract(Sort(filter, field=, sort-desc=, limit=, offset=), Rows(f0), ...) (executor.go:4686-4700, :4762-4769): the records in
  // SORT order.  The reference extracts every field for every sorted column of every shard and cuts afterwards; here offset and
  // limit are applied by the sort BEFORE any field is extracted: one fbk_bsi_sort, one fbk_extract_open_columns on the winners,
  // then one pass per field over the winners' shards only.
  ExtractedIDMatrix ExtractSorted(const std::string& sort_field, const Call* filter, bool desc, const std::vector<std::string>& fields,
                                  uint64_t limit = UINT64_MAX, uint64_t offset = 0, bool keep_zero = false) {
    for (const std::string& name : fields)
      if (!idx_.sets_.count(name) && !idx_.ints_.count(name)) throw Error(FBK_E_INVALID, "field not found: " + name);  // ErrFieldNotFound
    Scope sc(*this, {filter});
    ExtractedIDMatrix out;
    out.Fields = fields;
    if (shards().empty()) return out;
    const SortedRow sorted = Sort(sort_field, filter, desc, limit, offset, keep_zero);
    ExtractHandle hd{idx_.ctx_};
    std::vector<uint32_t> rank(sorted.Columns.size());
    check(fbk_extract_open_columns(idx_.ctx_, sorted.Columns.data(), sorted.Columns.size(), shards().data(), uint32_t(shards().size()), &hd.h, rank.data()));
    fill_fields(hd.h, sorted.Columns, &rank, fields, out);
    return out;
  }

 private:
  struct ExtractHandle {
    fbk_ctx* ctx;
    fbk_extract* h = nullptr;
    ~ExtractHandle() { fbk_extract_free(ctx, h); }
  };
  // the per-field calls of a handle: record k of `cols` is slot (rank ? rank[k] : k) of their outputs
  void fill_fields(fbk_extract* h, const std::vector<uint64_t>& cols, const std::vector<uint32_t>* rank, const std::vector<std::string>& fields,
                   ExtractedIDMatrix& out) {
    const size_t n = shards().size();
    const uint64_t cnt = cols.size();
    auto slot = [&](uint64_t k) { return rank ? uint64_t((*rank)[k]) : k; };
    out.Columns.resize(cnt);
    for (uint64_t k = 0; k < cnt; ++k) {
      out.Columns[k].ColumnID = cols[k];
      out.Columns[k].Rows.resize(fields.size());
    }
    for (size_t fi = 0; fi < fields.size(); ++fi) {
      auto it = idx_.ints_.find(fields[fi]);
      if (it != idx_.ints_.end()) {
        const Index::IntField& f = it->second;
        const std::vector<uint32_t> base = base_rows(f);
        std::vector<int64_t> vals(cnt);
        std::vector<uint8_t> pres(cnt);
        check(fbk_extract_bsi(idx_.ctx_, h, f.batch, base.data(), f.bit_depth, vals.data(), pres.data()));
        for (uint64_t k = 0; k < cnt; ++k)
          if (pres[slot(k)]) out.Columns[k].Rows[fi] = std::vector<uint64_t>{uint64_t(vals[slot(k)] + f.base)};
        continue;
      }
      const Index::SetField& f = idx_.sets_.at(fields[fi]);
      for (uint64_t k = 0; k < cnt; ++k) out.Columns[k].Rows[fi] = std::vector<uint64_t>();
      const size_t nr = f.row_ids.size();
      const std::vector<uint32_t> rows_a = nr ? field_rows(f) : std::vector<uint32_t>();
      std::vector<uint64_t> offs(cnt + 1);
      std::vector<uint32_t> items;
      for (size_t i0 = 0; i0 < nr; i0 += kSumBlock) {
        const size_t bi = std::min(kSumBlock, nr - i0);
        const std::vector<uint32_t> ra = row_block(rows_a, n, nr, i0, bi);
        uint64_t m = 0;
        int32_t rc = fbk_extract_rows(idx_.ctx_, h, f.batch, ra.data(), uint32_t(bi), offs.data(), items.data(), items.size(), &m);
        if (rc == FBK_E_CAPACITY) {
          items.resize(m);
          rc = fbk_extract_rows(idx_.ctx_, h, f.batch, ra.data(), uint32_t(bi), offs.data(), items.data(), items.size(), &m);
        }
        check(rc);
        for (uint64_t k = 0; k < cnt; ++k)
          for (uint64_t p = offs[slot(k)]; p < offs[slot(k) + 1]; ++p) out.Columns[k].Rows[fi]->push_back(f.row_ids[i0 + items[p]]);
      }
    }
  }
  struct GroupAgg {
    std::string sum_field;                  // aggregate=Sum(field)
    std::string distinct_field;             // aggregate=Count(Distinct(X, field))
    const RowSet* distinct_filter = nullptr;  // X (nullptr: none)
  };
  // ---- evaluation of bitmap calls ----
  RowSet leaf_row(const std::string& field, uint64_t row) {
    const Index::SetField& f = idx_.sets_.at(field);
    std::vector<uint32_t> rows;
    for (uint64_t s : shards()) {
      auto it = f.ordinal.find({s, row});
      rows.push_back(it == f.ordinal.end() ? f.empty_row : it->second);
    }
    return RowSet(idx_.ctx_, f.batch, std::move(rows), false);
  }
  RowSet fresh(fbk_batch* b) {
    std::vector<uint32_t> rows(shards().size());
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = uint32_t(i);
    return RowSet(idx_.ctx_, b, std::move(rows), true);
  }
  RowSet setop(int32_t op, const RowSet& a, const RowSet& b) {
    fbk_batch* o = nullptr;
    ++library_calls;
    check(fbk_setop(idx_.ctx_, op, a.batch(), a.rows().data(), b.batch(), b.rows().data(), a.rows().size(), FBK_SETOP_OPTIMIZE, &o, nullptr));
    return fresh(o);
  }
  std::vector<uint32_t> base_rows(const Index::IntField& f) const {
    std::vector<uint32_t> base;
    for (uint64_t s : shards()) {
      auto it = f.base_row.find(s);
      base.push_back(it == f.base_row.end() ? f.empty_base : it->second);
    }
    return base;
  }
  RowSet not_null(const Index::IntField& f) {  // fragment.notNull: the exists plane
    return RowSet(idx_.ctx_, f.batch, base_rows(f), false);
  }
  RowSet empty_set(const Index::IntField& f) {
    return RowSet(idx_.ctx_, f.batch, std::vector<uint32_t>(shards().size(), f.empty_base), false);
  }
  // executeRowBSIGroupShard, executor.go:5249-5355, with bsiGroup.baseValue / baseValueBetween: what a BSI condition becomes
  // once the predicate is clamped to the field — the empty row, the not-null row, or a scan with base-relative predicates
  struct RangeSpec {
    enum What { kEmpty, kNotNull, kScan, kScanBetween } what = kEmpty;
    int32_t op = 0;
    int64_t lo = 0, hi = 0;  // kScan: lo is the predicate
  };
  RangeSpec range_spec(const Call& c, const Index::IntField& f) const {
    const int64_t dmin = f.base - (f.bit_depth >= 63 ? INT64_MAX : ((int64_t(1) << f.bit_depth) - 1));  // bitDepthMin
    const int64_t dmax = f.base + (f.bit_depth >= 63 ? INT64_MAX : ((int64_t(1) << f.bit_depth) - 1));  // bitDepthMax
    RangeSpec r;
    if (c.kind == Call::kBetween) {
      int64_t lo = c.value, hi = c.value2;
      if (hi < dmin || lo > dmax || hi < lo) return r;  // baseValueBetween outOfRange
      if (lo <= f.min && hi >= f.max) return r.what = RangeSpec::kNotNull, r;
      lo = std::max(lo, dmin);
      hi = std::min(hi, dmax);
      r.what = RangeSpec::kScanBetween;
      r.lo = lo - f.base;
      r.hi = hi - f.base;
      return r;
    }
    const int32_t op = c.op;
    const int64_t value = c.value;
    int64_t bv = 0;
    bool out_of_range = false;
    if (op == FBK_BSI_GT || op == FBK_BSI_GTE) {
      if (value > dmax) out_of_range = true;
      else if (value < dmin) bv = dmin - f.base - (op == FBK_BSI_GT ? 1 : 0);
      else bv = value - f.base;
    } else if (op == FBK_BSI_LT || op == FBK_BSI_LTE) {
      if (value < dmin) out_of_range = true;
      else if (value > dmax) bv = dmax - f.base + (op == FBK_BSI_LT ? 1 : 0);
      else bv = value - f.base;
    } else {
      if (value < dmin || value > dmax) out_of_range = true;
      else bv = value - f.base;
    }
    if (out_of_range && op != FBK_BSI_NEQ) return r;
    if ((op == FBK_BSI_LT && value > f.max) || (op == FBK_BSI_LTE && value >= f.max) || (op == FBK_BSI_GT && value < f.min) ||
        (op == FBK_BSI_GTE && value <= f.min))
      return r.what = RangeSpec::kNotNull, r;
    if (out_of_range && op == FBK_BSI_NEQ) return r.what = RangeSpec::kNotNull, r;
    r.what = RangeSpec::kScan;
    r.op = op;
    r.lo = bv;
    return r;
  }
  RowSet range(const Call& c) {
    const Index::IntField& f = idx_.ints_.at(c.field);
    const RangeSpec r = range_spec(c, f);
    if (r.what == RangeSpec::kEmpty) return empty_set(f);
    if (r.what == RangeSpec::kNotNull) return not_null(f);
    std::vector<uint32_t> base = base_rows(f);
    fbk_batch* o = nullptr;
    ++library_calls;
    if (r.what == RangeSpec::kScanBetween)
      check(fbk_bsi_range_between(idx_.ctx_, f.batch, base.data(), uint32_t(base.size()), f.bit_depth, r.lo, r.hi, FBK_SETOP_OPTIMIZE, &o, nullptr));
    else
      check(fbk_bsi_range(idx_.ctx_, f.batch, base.data(), uint32_t(base.size()), r.op, f.bit_depth, r.lo, FBK_SETOP_OPTIMIZE, &o, nullptr));
    return fresh(o);
  }

  // Row(field_x <op> field_y): one fbk_bsi_compare with the two fields' Bases.  count: the count-only form, nothing is materialised.
  RowSet compare(const Call& c, uint64_t* count = nullptr) {
    const Index::IntField &fx = idx_.ints_.at(c.field), &fy = idx_.ints_.at(c.field2);
    const std::vector<uint32_t> bx = base_rows(fx), by = base_rows(fy);
    std::vector<uint64_t> counts(count ? bx.size() : 0);
    fbk_batch* o = nullptr;
    ++library_calls;
    check(fbk_bsi_compare(idx_.ctx_, fx.batch, bx.data(), fx.bit_depth, fx.base, fy.batch, by.data(), fy.bit_depth, fy.base, c.op, nullptr, nullptr, uint32_t(bx.size()),
                          FBK_SETOP_OPTIMIZE, count ? nullptr : &o, count ? counts.data() : nullptr));
    if (!count) return fresh(o);
    *count = 0;
    for (uint64_t x : counts) *count += x;
    return RowSet();
  }

  // ---- a call tree as ONE fbk_expr_* call -----------------------------------------------------------------------------------
  static bool is_operator(Call::Kind k) { return k == Call::kIntersect || k == Call::kUnion || k == Call::kDifference || k == Call::kXor || k == Call::kNot; }
  struct ExprBuild {
    std::vector<fbk_expr_leaf> leaves;
    std::vector<std::unique_ptr<std::vector<uint32_t>>> rows;  // the leaves' row lists (stable addresses)
    std::vector<uint32_t> prog;
    std::vector<RowSet> temps;  // rows evaluated beforehand (Shift results, subtrees beyond the limits): they enter as ROW leaves
    struct Mark {
      size_t l, r, p, t;
    };
    Mark mark() const { return {leaves.size(), rows.size(), prog.size(), temps.size()}; }
    void rollback(const Mark& m) {
      leaves.resize(m.l);
      rows.resize(m.r);
      prog.resize(m.p);
      temps.erase(temps.begin() + std::ptrdiff_t(m.t), temps.end());
    }
    void push(const fbk_batch* b, std::vector<uint32_t> r, uint32_t kind = FBK_EXPR_ROW, int32_t op = 0, uint32_t bit_depth = 0, int64_t lo = 0, int64_t hi = 0) {
      rows.emplace_back(new std::vector<uint32_t>(std::move(r)));
      fbk_expr_leaf lf{};
      lf.batch = b;
      lf.rows = rows.back()->data();
      lf.kind = kind;
      lf.op = op;
      lf.bit_depth = bit_depth;
      lf.lo = lo;
      lf.hi = hi;
      prog.push_back((FBK_EXPR_PUSH << 24) | uint32_t(leaves.size()));
      leaves.push_back(lf);
    }
    void push(RowSet&& r) {
      temps.push_back(std::move(r));
      push(temps.back().batch(), temps.back().rows());
    }
    bool too_big() const { return prog.size() > FBK_EXPR_MAX_PROG || leaves.size() > FBK_EXPR_MAX_LEAVES; }
  };
  RowSet run(ExprBuild& b) {
    fbk_batch* o = nullptr;
    ++library_calls;
    check(fbk_expr_eval(idx_.ctx_, b.leaves.data(), uint32_t(b.leaves.size()), b.prog.data(), uint32_t(b.prog.size()), uint32_t(shards().size()),
                        FBK_SETOP_OPTIMIZE, &o, nullptr));
    return fresh(o);
  }
  // Appends the postfix form of `c`, to be evaluated with `base` values already on the stack (base < FBK_EXPR_MAX_DEPTH); returns
  // the stack depth it adds, or -1 when it does not fit there (the caller evaluates it on its own and pushes the row).  `root`: c
  // is the whole program so far — when it outgrows the limits, what is there is evaluated and enters the rest as one row.
  int compile(const Call& c, ExprBuild& b, uint32_t base, bool root) {
    switch (c.kind) {
      case Call::kRow:
      case Call::kAll:
      case Call::kPrecomputed: {
        RowSet r = eval_nodes(c);  // (a row of a resident batch: no device call)
        b.push(r.batch(), r.rows());
        return 1;
      }
      case Call::kRange:
      case Call::kBetween: {  // the clamping stays on the host; what is left is a leaf of the tree
        const Index::IntField& f = idx_.ints_.at(c.field);
        const RangeSpec r = range_spec(c, f);
        if (r.what == RangeSpec::kEmpty) b.push(f.batch, std::vector<uint32_t>(shards().size(), f.empty_base));
        else if (r.what == RangeSpec::kNotNull) b.push(f.batch, base_rows(f));
        else b.push(f.batch, base_rows(f), r.what == RangeSpec::kScan ? FBK_EXPR_BSI : FBK_EXPR_BETWEEN, r.op, f.bit_depth, r.lo, r.hi);
        return 1;
      }
      case Call::kShift:    // crosses containers: a call of its own, its result a ROW leaf
      case Call::kCompare:  // two fields' planes: a call of its own (fbk_bsi_compare), its result a ROW leaf
        b.push(eval_nodes(c));
        return 1;
      default: break;
    }
    const bool is_not = c.kind == Call::kNot;
    if (is_not && c.children.size() != 1) throw Error(FBK_E_INVALID, "Not() requires exactly one child");
    if (c.children.empty()) throw Error(FBK_E_INVALID, "empty call");  // e.g. "Intersect() requires at least 1 child"
    const uint32_t op = c.kind == Call::kIntersect ? FBK_EXPR_AND : c.kind == Call::kUnion ? FBK_EXPR_OR : c.kind == Call::kXor ? FBK_EXPR_XOR : FBK_EXPR_ANDNOT;
    int d;
    if (is_not) {  // existence row \ x (executeNotShard)
      RowSet ex = leaf_row(Index::kExistence, 0);
      b.push(ex.batch(), ex.rows());
      d = 1;
    } else {
      d = compile_child(c.children[0], b, base);
    }
    for (size_t i = is_not ? 0 : 1; i < c.children.size(); ++i) {  // left fold, child by child
      if (base + 2 > FBK_EXPR_MAX_DEPTH) return -1;
      const ExprBuild::Mark m = b.mark();
      int di = compile_child(c.children[i], b, base + 1);
      b.prog.push_back(op << 24);
      if (b.too_big()) {
        if (!root) return -1;
        b.rollback(m);
        RowSet acc = run(b);
        b = ExprBuild();
        b.push(std::move(acc));
        d = 1;
        di = compile_child(c.children[i], b, 1);
        b.prog.push_back(op << 24);
      }
      d = std::max(d, 1 + di);
    }
    return d;
  }
  int compile_child(const Call& c, ExprBuild& b, uint32_t base) {
    const ExprBuild::Mark m = b.mark();
    const int d = compile(c, b, base, false);
    if (d >= 0 && base + uint32_t(d) <= FBK_EXPR_MAX_DEPTH && !b.too_big()) return d;
    b.rollback(m);
    b.push(eval(c));  // on its own, from an empty stack
    return 1;
  }
  void compile_root(const Call& c, ExprBuild& b) { (void)compile(c, b, 0, true); }
  RowSet eval_fused(const Call& c) {
    ExprBuild b;
    compile_root(c, b);
    return run(b);
  }
  // A call whose children are all plain rows of ONE set field keeps the one-level kernels tuned for exactly that shape
  // (fbk_fold_n) whatever its fan-out: measured, the union of 64 rows is 2.7 x faster there than through the
  // interpreter and at three rows the two are level, so nothing says the interpreter is ahead anywhere in between.
  static constexpr size_t kFoldFrom = 2;
  bool plain_rows_of_one_field(const Call& c) const {
    if (c.kind == Call::kNot || !is_operator(c.kind) || c.children.size() < kFoldFrom) return false;
    for (const Call& ch : c.children)
      if (ch.kind != Call::kRow || ch.field != c.children[0].field) return false;
    return true;
  }
  static int32_t fold_op(Call::Kind k) { return k == Call::kIntersect ? FBK_OP_AND : k == Call::kUnion ? FBK_OP_OR : k == Call::kXor ? FBK_OP_XOR : FBK_OP_ANDNOT; }
  std::vector<uint32_t> fold_groups(const Call& c) {  // [shard][child]
    const size_t n = shards().size(), k = c.children.size();
    std::vector<uint32_t> g(n * k);
    for (size_t j = 0; j < k; ++j) {
      RowSet r = leaf_row(c.children[j].field, c.children[j].row);
      for (size_t s = 0; s < n; ++s) g[s * k + j] = r.rows()[s];
    }
    return g;
  }
  RowSet eval_fold(const Call& c) {
    const std::vector<uint32_t> g = fold_groups(c);
    fbk_batch* o = nullptr;
    ++library_calls;
    check(fbk_fold_n(idx_.ctx_, fold_op(c.kind), idx_.sets_.at(c.children[0].field).batch, g.data(), shards().size(), uint32_t(c.children.size()), FBK_SETOP_OPTIMIZE, &o, nullptr));
    return fresh(o);
  }
  // Sum / Min / Max over an operator tree: the aggregate runs in the tree's own launch (fbk_expr_bsi_agg), the rule of Count(tree)
  // above.  A call over plain rows of one field keeps fbk_fold_n and the aggregate's own call (see kFoldFrom: nothing measured
  // says the interpreter is ahead on that shape); a plain row or no filter keeps today's single call.
  bool fuses_aggregate(const Call& c) const { return fuse_calls && is_operator(c.kind) && !plain_rows_of_one_field(c); }
  // TopK / TopN over an operator tree: fbk_expr_topk where its launch evaluates the tree ONCE per (shard, slot) — a field of at most
  // 64 rows, or 128 shards and more (k_expr_rows_vs_filter splits a longer field over several blocks while the grid is short of
  // 2048, and every block evaluates the tree again: measured 2-4 % behind fbk_expr_eval + fbk_topk at 96 shards x 256 / 1024 rows,
  // 10-19 % ahead at 64 rows and 2 % ahead at 1024 shards x 1024 rows).  Everything else keeps the pair.
  bool fuses_topk(const Call& c, size_t n_shards, size_t n_rows) const { return fuses_aggregate(c) && (n_rows <= 64 || n_shards >= 128); }
  void expr_aggregate(uint32_t agg, const Call& filter, const Index::IntField& f, const std::vector<uint32_t>& base, std::vector<int64_t>& vals,
                      std::vector<uint64_t>& counts) {
    ExprBuild b;
    compile_root(filter, b);  // (Shift results and subtrees beyond a limit enter as row leaves)
    ++library_calls;
    check(fbk_expr_bsi_agg(idx_.ctx_, b.leaves.data(), uint32_t(b.leaves.size()), b.prog.data(), uint32_t(b.prog.size()), uint32_t(base.size()), agg, f.batch,
                           base.data(), f.bit_depth, vals.data(), counts.data()));
  }
  RowSet eval(const Call& c) {
    if (!fuse_calls || !is_operator(c.kind)) return eval_nodes(c);
    return plain_rows_of_one_field(c) ? eval_fold(c) : eval_fused(c);
  }
  // node by node (children through eval: under fuse_calls an operator below a Shift is one call again)
  RowSet eval_nodes(const Call& c) {
    switch (c.kind) {
      case Call::kRow: return leaf_row(c.field, c.row);
      case Call::kRange:
      case Call::kBetween: return range(c);
      case Call::kCompare: return compare(c);
      case Call::kAll: return leaf_row(Index::kExistence, 0);
      case Call::kPrecomputed: {
        if (!c.pre || !c.pre->batch) throw Error(FBK_E_INVALID, "Precomputed() without a result");
        std::vector<uint32_t> rows;
        for (uint64_t s : shards()) rows.push_back(c.pre->PosRow(s));
        return RowSet(idx_.ctx_, c.pre->batch.get(), std::move(rows), false);
      }
      case Call::kShift: {
        if (c.children.size() != 1) throw Error(FBK_E_INVALID, c.children.empty() ? "Shift() requires an input row" : "Shift() only accepts a single row input");
        if (c.value < 0) throw Error(FBK_E_INVALID, "cannot shift by negative values");  // row.go:375-377
        RowSet acc = eval(c.children[0]);
        const std::vector<uint64_t>& sh = shards();
        for (int64_t i = 0; i < c.value; ++i) {  // Row.Shift: n single-column shifts (row.go:383-393)
          std::vector<uint32_t> carry(sh.size(), FBK_NO_ROW);
          for (size_t k = 1; k < sh.size(); ++k)
            if (sh[k - 1] + 1 == sh[k]) carry[k] = acc.rows()[k - 1];  // last column of the previous shard
          fbk_batch* o = nullptr;
          ++library_calls;
          check(fbk_shift(idx_.ctx_, acc.batch(), acc.rows().data(), carry.data(), sh.size(), FBK_SETOP_OPTIMIZE, &o, nullptr));
          acc = fresh(o);
        }
        return acc;
      }
      case Call::kNot: {
        if (c.children.size() != 1) throw Error(FBK_E_INVALID, "Not() requires exactly one child");
        RowSet ex = leaf_row(Index::kExistence, 0), child = eval(c.children[0]);
        return setop(FBK_OP_ANDNOT, ex, child);
      }
      default: break;
    }
    if (c.children.empty()) throw Error(FBK_E_INVALID, "empty call");  // e.g. "Intersect() requires at least 1 child"
    const int32_t op = c.kind == Call::kIntersect ? FBK_OP_AND : c.kind == Call::kUnion ? FBK_OP_OR : c.kind == Call::kXor ? FBK_OP_XOR : FBK_OP_ANDNOT;
    RowSet acc = eval(c.children[0]);
    for (size_t i = 1; i < c.children.size(); ++i) {  // left fold, child by child
      RowSet next = eval(c.children[i]);
      acc = setop(op, acc, next);
    }
    return acc;
  }
  uint64_t count_rows(const RowSet& r) {
    std::vector<uint64_t> counts(r.rows().size());
    if (!counts.empty()) {
      ++library_calls;
      check(fbk_count(idx_.ctx_, r.batch(), r.rows().data(), counts.size(), counts.data()));
    }
    uint64_t n = 0;
    for (uint64_t c : counts) n += c;
    return n;
  }
  // fn(i, p) for every set bit of rows[i]: p = its position within the shard row
  template <class Fn>
  void for_each_bit(const fbk_batch* b, const std::vector<uint32_t>& rows, Fn&& fn) {
    // gather the rows into one batch, download, expand
    fbk_batch* o = nullptr;
    check(fbk_setop(idx_.ctx_, FBK_OP_OR, b, rows.data(), b, rows.data(), rows.size(), 0, &o, nullptr));
    uint32_t n_rows = 0;
    uint64_t nc = 0, pb = 0;
    check(fbk_batch_info(idx_.ctx_, o, &n_rows, &nc, &pb));
    std::vector<fbk_container_desc> descs(nc ? nc : 1);
    std::vector<uint8_t> payload(pb ? pb : 1);
    int32_t rc = fbk_batch_download(idx_.ctx_, o, descs.data(), nc, payload.data(), pb);
    fbk_batch_free(idx_.ctx_, o);
    check(rc);
    for (uint64_t i = 0; i < nc; ++i) {
      const fbk_container_desc& d = descs[i];
      const uint64_t hb = (d.key & 15) << 16;
      const uint64_t* w = reinterpret_cast<const uint64_t*>(payload.data() + d.off);  // keep-bitmap output: 1024 words
      for (uint32_t k = 0; k < FBK_BITMAP_WORDS; ++k)
        for (uint64_t x = w[k]; x; x &= x - 1) fn(d.row, hb | (uint64_t(k) * 64 + uint64_t(__builtin_ctzll(x))));
    }
  }
  std::vector<uint64_t> columns(const RowSet& r) {
    std::vector<uint64_t> out;
    for_each_bit(r.batch(), r.rows(), [&](uint32_t i, uint64_t p) { out.push_back(shards()[i] * ShardWidth + p); });
    std::sort(out.begin(), out.end());
    return out;
  }
  ValCount minmax(const std::string& field, const Call* filter, bool is_min) {
    Scope sc(*this, {filter});
    const Index::IntField& f = idx_.ints_.at(field);
    const size_t n = shards().size();
    ValCount out;
    if (n == 0) return out;
    std::vector<uint32_t> base = base_rows(f);
    std::vector<int64_t> vals(n);
    std::vector<uint64_t> counts(n);
    auto fn = is_min ? fbk_bsi_min : fbk_bsi_max;
    if (filter && fuses_aggregate(*filter)) {
      expr_aggregate(is_min ? FBK_AGG_MIN : FBK_AGG_MAX, *filter, f, base, vals, counts);
    } else if (filter) {
      RowSet fr = eval(*filter);
      check(fn(idx_.ctx_, f.batch, base.data(), uint32_t(n), f.bit_depth, fr.batch(), fr.rows().data(), vals.data(), counts.data()));
    } else {
      check(fn(idx_.ctx_, f.batch, base.data(), uint32_t(n), f.bit_depth, nullptr, nullptr, vals.data(), counts.data()));
    }
    for (size_t s = 0; s < n; ++s) {
      // Field.MinForShard / MaxForShard: (0, 0) when the shard has no value, else value + Base (field.go:1590, 1620)
      const ValCount v = counts[s] ? ValCount{vals[s] + f.base, int64_t(counts[s])} : ValCount{};
      out = is_min ? out.Smaller(v) : out.Larger(v);
    }
    return out;
  }
  std::vector<uint32_t> field_rows(const Index::SetField& f) {
    const size_t n = shards().size(), nr = f.row_ids.size();
    std::vector<uint32_t> rows(n * nr);
    for (size_t s = 0; s < n; ++s)
      for (size_t i = 0; i < nr; ++i) {
        auto it = f.ordinal.find({shards()[s], f.row_ids[i]});
        rows[s * nr + i] = it == f.ordinal.end() ? f.empty_row : it->second;
      }
    return rows;
  }
  bool emit(const std::vector<FieldRow>& group, uint64_t count, int64_t agg, uint64_t limit, std::vector<GroupCount>& out) {
    if (count == 0) return true;  // groupByIterator.Next skips Count == 0 (executor.go:8905-8913)
    GroupCount g;
    g.Group = group;
    g.Count = count;
    g.Agg = agg;
    out.push_back(std::move(g));
    return !(limit && out.size() >= limit);
  }
  // aggregate=Sum(field) of the last level (b == nullptr) or the last two levels: fbk_count_matrix_sum, the prefix row (if any)
  // as the filter — ONE call when both fields have at most kSumBlock rows, otherwise one call per block of kSumBlock x kSumBlock
  // rows (the call's limit per side; fbk_count / fbk_count_matrix take up to 2^22 rows against one).  counts[i * nb + j] =
  // columns WITH a value (the group's Count), sums + count * Base = its Agg (executeSumCountShard per group, executor.go:2155-2216).
  static constexpr size_t kSumBlock = 4096;
  static constexpr size_t kCubeCells = size_t(1) << 24;  // groups per fbk_count_cube call
  // the rows [k0, k0 + bk) of every shard of a [n][nk] row list
  static std::vector<uint32_t> row_block(const std::vector<uint32_t>& rows, size_t n, size_t nk, size_t k0, size_t bk) {
    if (k0 == 0 && bk == nk) return rows;
    std::vector<uint32_t> out(n * bk);
    for (size_t s = 0; s < n; ++s) std::copy(rows.begin() + s * nk + k0, rows.begin() + s * nk + k0 + bk, out.begin() + s * bk);
    return out;
  }
  void sum_matrix(const std::string& agg_field, const Index::SetField& fa, const std::vector<uint32_t>& rows_a, const Index::SetField* fb,
                  const std::vector<uint32_t>* rows_b, const RowSet* prefix, std::vector<int64_t>& agg, std::vector<uint64_t>& counts) {
    const Index::IntField& f = idx_.ints_.at(agg_field);
    std::vector<uint32_t> base = base_rows(f);
    const size_t n = base.size(), na = fa.row_ids.size(), nb = fb ? fb->row_ids.size() : 1;
    agg.assign(na * nb, 0);
    counts.assign(na * nb, 0);
    for (size_t i0 = 0; i0 < na; i0 += kSumBlock)
      for (size_t j0 = 0; j0 < nb; j0 += kSumBlock) {
        const size_t bi = std::min(kSumBlock, na - i0), bj = std::min(kSumBlock, nb - j0);
        const std::vector<uint32_t> ra = row_block(rows_a, n, na, i0, bi);
        const std::vector<uint32_t> rb = fb ? row_block(*rows_b, n, nb, j0, bj) : std::vector<uint32_t>();
        std::vector<int64_t> sums(bi * bj);
        std::vector<uint64_t> cnt(bi * bj);
        check(fbk_count_matrix_sum(idx_.ctx_, fa.batch, ra.data(), uint32_t(bi), fb ? fb->batch : nullptr, fb ? rb.data() : nullptr, uint32_t(bj),
                                   prefix ? prefix->batch() : nullptr, prefix ? prefix->rows().data() : nullptr, f.batch, base.data(), f.bit_depth,
                                   uint32_t(n), sums.data(), cnt.data()));
        for (size_t i = 0; i < bi; ++i)
          for (size_t j = 0; j < bj; ++j) {
            const size_t k = (i0 + i) * nb + j0 + j;
            counts[k] = cnt[i * bj + j];
            agg[k] = int64_t(uint64_t(sums[i * bj + j]) + counts[k] * uint64_t(f.base));
          }
      }
  }
  // aggregate=Count(Distinct(X, field)) of the last level (fb == nullptr) or the last two levels: fbk_count_matrix_distinct with
  // prefix ∩ X as the filter, in blocks of kSumBlock x kSumBlock rows as sum_matrix.  distinct[i * nb + j] = the group's Agg.
  void distinct_matrix(const GroupAgg& agg, const Index::SetField& fa, const std::vector<uint32_t>& rows_a, const Index::SetField* fb,
                       const std::vector<uint32_t>* rows_b, const RowSet* prefix, std::vector<int64_t>& distinct) {
    const Index::IntField& f = idx_.ints_.at(agg.distinct_field);
    std::vector<uint32_t> base = base_rows(f);
    const size_t n = base.size(), na = fa.row_ids.size(), nb = fb ? fb->row_ids.size() : 1;
    std::unique_ptr<RowSet> both;
    const RowSet* filt = prefix ? prefix : agg.distinct_filter;
    if (prefix && agg.distinct_filter) {
      both.reset(new RowSet(setop(FBK_OP_AND, *prefix, *agg.distinct_filter)));
      filt = both.get();
    }
    distinct.assign(na * nb, 0);
    for (size_t i0 = 0; i0 < na; i0 += kSumBlock)
      for (size_t j0 = 0; j0 < nb; j0 += kSumBlock) {
        const size_t bi = std::min(kSumBlock, na - i0), bj = std::min(kSumBlock, nb - j0);
        const std::vector<uint32_t> ra = row_block(rows_a, n, na, i0, bi);
        const std::vector<uint32_t> rb = fb ? row_block(*rows_b, n, nb, j0, bj) : std::vector<uint32_t>();
        std::vector<uint64_t> d(bi * bj);
        check(fbk_count_matrix_distinct(idx_.ctx_, fa.batch, ra.data(), uint32_t(bi), fb ? fb->batch : nullptr, fb ? rb.data() : nullptr, uint32_t(bj),
                                        filt ? filt->batch() : nullptr, filt ? filt->rows().data() : nullptr, f.batch, base.data(), f.bit_depth,
                                        uint32_t(n), d.data(), nullptr));
        for (size_t i = 0; i < bi; ++i)
          for (size_t j = 0; j < bj; ++j) distinct[(i0 + i) * nb + j0 + j] = int64_t(d[i * bj + j]);
      }
  }
  // Min / Max of an int field for the last level (fb == nullptr) or the last two levels: fbk_count_matrix_minmax with the prefix
  // row (if any) as the filter, in blocks of kSumBlock x kSumBlock rows as sum_matrix.  Base is added where the group has a value.
  void minmax_matrix(const std::string& agg_field, const Index::SetField& fa, const std::vector<uint32_t>& rows_a, const Index::SetField* fb,
                     const std::vector<uint32_t>* rows_b, const RowSet* prefix, std::vector<int64_t>& mins, std::vector<int64_t>& maxs,
                     std::vector<uint64_t>& cmin, std::vector<uint64_t>& cmax) {
    const Index::IntField& f = idx_.ints_.at(agg_field);
    std::vector<uint32_t> base = base_rows(f);
    const size_t n = base.size(), na = fa.row_ids.size(), nb = fb ? fb->row_ids.size() : 1;
    mins.assign(na * nb, 0), maxs.assign(na * nb, 0), cmin.assign(na * nb, 0), cmax.assign(na * nb, 0);
    for (size_t i0 = 0; i0 < na; i0 += kSumBlock)
      for (size_t j0 = 0; j0 < nb; j0 += kSumBlock) {
        const size_t bi = std::min(kSumBlock, na - i0), bj = std::min(kSumBlock, nb - j0);
        const std::vector<uint32_t> ra = row_block(rows_a, n, na, i0, bi);
        const std::vector<uint32_t> rb = fb ? row_block(*rows_b, n, nb, j0, bj) : std::vector<uint32_t>();
        std::vector<int64_t> mn(bi * bj), mx(bi * bj);
        std::vector<uint64_t> c0(bi * bj), c1(bi * bj);
        check(fbk_count_matrix_minmax(idx_.ctx_, fa.batch, ra.data(), uint32_t(bi), fb ? fb->batch : nullptr, fb ? rb.data() : nullptr, uint32_t(bj),
                                      prefix ? prefix->batch() : nullptr, prefix ? prefix->rows().data() : nullptr, f.batch, base.data(), f.bit_depth,
                                      uint32_t(n), FBK_MINMAX_AUTO, mn.data(), mx.data(), c0.data(), c1.data()));
        for (size_t i = 0; i < bi; ++i)
          for (size_t j = 0; j < bj; ++j) {
            const size_t k = (i0 + i) * nb + j0 + j, q = i * bj + j;
            if (!c0[q]) continue;  // an empty group: (0, 0) with counts 0
            mins[k] = int64_t(uint64_t(mn[q]) + uint64_t(f.base)), maxs[k] = int64_t(uint64_t(mx[q]) + uint64_t(f.base));
            cmin[k] = c0[q], cmax[k] = c1[q];
          }
      }
  }
  // Percentiles of an int field for the last level (fb == nullptr) or the last two levels: fbk_count_matrix_quantiles with the prefix
  // row (if any) as the filter, in blocks of rows as minmax_matrix; the leading field's block shrinks until the call's histograms
  // (2 KiB per group and fraction) fit its 2^30-byte scratch.  vals / cnts: [na * nb][fractions], Base added where the group has a
  // value; ns: [na * nb].
  void quantile_matrix(const std::string& agg_field, const std::vector<std::pair<uint32_t, uint32_t>>& fractions, const Index::SetField& fa,
                       const std::vector<uint32_t>& rows_a, const Index::SetField* fb, const std::vector<uint32_t>* rows_b, const RowSet* prefix,
                       std::vector<int64_t>& vals, std::vector<uint64_t>& cnts, std::vector<uint64_t>& ns) {
    const Index::IntField& f = idx_.ints_.at(agg_field);
    std::vector<uint32_t> base = base_rows(f), num, den;
    for (const auto& fr : fractions) num.push_back(fr.first), den.push_back(fr.second);
    const size_t n = base.size(), na = fa.row_ids.size(), nb = fb ? fb->row_ids.size() : 1, nq = fractions.size();
    vals.assign(na * nb * nq, 0), cnts.assign(na * nb * nq, 0), ns.assign(na * nb, 0);
    const size_t bj_most = std::min(kSumBlock, nb), pairs_most = (size_t(1) << 30) / (8u << 8);  // (FBK_GQUANT_GLOBAL's digit: 8 bits)
    const size_t bi_most = std::max<size_t>(1, std::min(kSumBlock, pairs_most / (bj_most * std::max<size_t>(1, nq))));
    for (size_t i0 = 0; i0 < na; i0 += bi_most)
      for (size_t j0 = 0; j0 < nb; j0 += kSumBlock) {
        const size_t bi = std::min(bi_most, na - i0), bj = std::min(kSumBlock, nb - j0);
        const std::vector<uint32_t> ra = row_block(rows_a, n, na, i0, bi);
        const std::vector<uint32_t> rb = fb ? row_block(*rows_b, n, nb, j0, bj) : std::vector<uint32_t>();
        std::vector<int64_t> v(bi * bj * nq);
        std::vector<uint64_t> c(bi * bj * nq), t(bi * bj);
        check(fbk_count_matrix_quantiles(idx_.ctx_, fa.batch, ra.data(), uint32_t(bi), fb ? fb->batch : nullptr, fb ? rb.data() : nullptr, uint32_t(bj),
                                         prefix ? prefix->batch() : nullptr, prefix ? prefix->rows().data() : nullptr, f.batch, base.data(), f.bit_depth,
                                         uint32_t(n), num.data(), den.data(), uint32_t(nq), FBK_GQUANT_AUTO, v.data(), c.data(), t.data()));
        for (size_t i = 0; i < bi; ++i)
          for (size_t j = 0; j < bj; ++j) {
            const size_t k = (i0 + i) * nb + j0 + j, g = i * bj + j;
            ns[k] = t[g];
            for (size_t q = 0; q < nq && t[g]; ++q) vals[k * nq + q] = int64_t(uint64_t(v[g * nq + q]) + uint64_t(f.base)), cnts[k * nq + q] = c[g * nq + q];
          }
      }
  }
  // GroupByMinMax / GroupByQuantiles over fields[level..]: the last one or two levels are one count call (tot = Count per group)
  // and leaf(level, fa, rows_a, fb, rows_b, prefix, tot), which emits the records and returns false once the limit is reached;
  // earlier levels materialise prefix ∩ row as group_by_rec does
  template <class Leaf>
  bool last_levels_rec(const std::vector<std::string>& fields, size_t level, const RowSet* prefix, std::vector<FieldRow>& group, const Leaf& leaf) {
    const size_t n = shards().size();
    const Index::SetField& fa = idx_.sets_.at(fields[level]);
    const size_t na = fa.row_ids.size();
    if (na == 0) return true;
    const size_t remaining = fields.size() - level;
    if (remaining > 2) {
      for (size_t i = 0; i < na; ++i) {
        RowSet r = leaf_row(fields[level], fa.row_ids[i]);
        group.push_back({fields[level], fa.row_ids[i]});
        bool go;
        if (prefix) {
          RowSet p = setop(FBK_OP_AND, r, *prefix);
          go = count_rows(p) == 0 ? true : last_levels_rec(fields, level + 1, &p, group, leaf);
        } else {
          go = last_levels_rec(fields, level + 1, &r, group, leaf);
        }
        group.pop_back();
        if (!go) return false;
      }
      return true;
    }
    const Index::SetField* fb = remaining == 2 ? &idx_.sets_.at(fields[level + 1]) : nullptr;
    const size_t nb = fb ? fb->row_ids.size() : 1;
    if (nb == 0) return true;
    const std::vector<uint32_t> rows_a = field_rows(fa), rows_b = fb ? field_rows(*fb) : std::vector<uint32_t>();
    std::vector<uint64_t> tot(na * nb, 0);  // Count: |group ∩ prefix|
    if (fb) {
      for (size_t i0 = 0; i0 < na; i0 += kSumBlock)
        for (size_t j0 = 0; j0 < nb; j0 += kSumBlock) {
          const size_t bi = std::min(kSumBlock, na - i0), bj = std::min(kSumBlock, nb - j0);
          const std::vector<uint32_t> ra = row_block(rows_a, n, na, i0, bi), rb = row_block(rows_b, n, nb, j0, bj);
          std::vector<uint64_t> c(bi * bj);
          check(fbk_count_matrix(idx_.ctx_, fa.batch, ra.data(), uint32_t(bi), fb->batch, rb.data(), uint32_t(bj), prefix ? prefix->batch() : nullptr,
                                 prefix ? prefix->rows().data() : nullptr, uint32_t(n), c.data(), nullptr));
          for (size_t i = 0; i < bi; ++i) std::copy(c.begin() + i * bj, c.begin() + (i + 1) * bj, tot.begin() + (i0 + i) * nb + j0);
        }
    } else if (prefix) {
      check(fbk_count_matrix(idx_.ctx_, fa.batch, rows_a.data(), uint32_t(na), prefix->batch(), prefix->rows().data(), 1, nullptr, nullptr, uint32_t(n),
                             tot.data(), nullptr));
    } else {
      std::vector<uint64_t> c(n * na);
      check(fbk_count(idx_.ctx_, fa.batch, rows_a.data(), c.size(), c.data()));
      for (size_t s = 0; s < n; ++s)
        for (size_t i = 0; i < na; ++i) tot[i] += c[s * na + i];
    }
    return leaf(level, fa, rows_a, fb, fb ? &rows_b : nullptr, prefix, tot);
  }
  // fields[level..]: the last three levels are one count-cube call; with an aggregate the last two are one count-matrix-sum /
  // -distinct call; earlier levels materialise prefix ∩ row (gbi.rows[i].row.Intersect(gbi.rows[i-1].row), executor.go:8829-8834)
  bool group_by_rec(const std::vector<std::string>& fields, size_t level, const RowSet* prefix, const GroupAgg& ag, uint64_t limit,
                    std::vector<FieldRow>& group, std::vector<GroupCount>& out) {
    const std::string& agg_field = ag.sum_field;
    const size_t n = shards().size();
    const Index::SetField& fa = idx_.sets_.at(fields[level]);
    const size_t na = fa.row_ids.size();
    if (na == 0) return true;
    std::vector<uint32_t> rows_a = field_rows(fa);
    const size_t remaining = fields.size() - level;
    if (remaining == 1) {
      std::vector<uint64_t> tot(na, 0);
      std::vector<int64_t> agg(na, 0);
      if (!agg_field.empty()) {
        sum_matrix(agg_field, fa, rows_a, nullptr, nullptr, prefix, agg, tot);
      } else if (prefix) {
        check(fbk_count_matrix(idx_.ctx_, fa.batch, rows_a.data(), uint32_t(na), prefix->batch(), prefix->rows().data(), 1, nullptr, nullptr,
                               uint32_t(n), tot.data(), nullptr));
      } else {
        std::vector<uint64_t> c(n * na);
        check(fbk_count(idx_.ctx_, fa.batch, rows_a.data(), c.size(), c.data()));
        for (size_t s = 0; s < n; ++s)
          for (size_t i = 0; i < na; ++i) tot[i] += c[s * na + i];
      }
      if (!ag.distinct_field.empty()) distinct_matrix(ag, fa, rows_a, nullptr, nullptr, prefix, agg);
      for (size_t i = 0; i < na; ++i) {
        if (!tot[i]) continue;
        group.push_back({fields[level], fa.row_ids[i]});
        const bool go = emit(group, tot[i], agg[i], limit, out);
        group.pop_back();
        if (!go) return false;
      }
      return true;
    }
    if (remaining == 2) {
      const Index::SetField& fb = idx_.sets_.at(fields[level + 1]);
      const size_t nb = fb.row_ids.size();
      if (nb == 0) return true;
      std::vector<uint32_t> rows_b = field_rows(fb);
      std::vector<uint64_t> tot(na * nb, 0);
      std::vector<int64_t> agg(na * nb, 0);
      if (!agg_field.empty()) {
        sum_matrix(agg_field, fa, rows_a, &fb, &rows_b, prefix, agg, tot);
      } else if (!ag.distinct_field.empty()) {
        // Count: the count matrix in blocks of kSumBlock x kSumBlock rows (its limit per side); Agg: the distinct matrix
        for (size_t i0 = 0; i0 < na; i0 += kSumBlock)
          for (size_t j0 = 0; j0 < nb; j0 += kSumBlock) {
            const size_t bi = std::min(kSumBlock, na - i0), bj = std::min(kSumBlock, nb - j0);
            const std::vector<uint32_t> ra = row_block(rows_a, n, na, i0, bi), rb = row_block(rows_b, n, nb, j0, bj);
            std::vector<uint64_t> c(bi * bj);
            check(fbk_count_matrix(idx_.ctx_, fa.batch, ra.data(), uint32_t(bi), fb.batch, rb.data(), uint32_t(bj), prefix ? prefix->batch() : nullptr,
                                   prefix ? prefix->rows().data() : nullptr, uint32_t(n), c.data(), nullptr));
            for (size_t i = 0; i < bi; ++i) std::copy(c.begin() + i * bj, c.begin() + (i + 1) * bj, tot.begin() + (i0 + i) * nb + j0);
          }
        distinct_matrix(ag, fa, rows_a, &fb, &rows_b, prefix, agg);
      } else {
        check(fbk_count_matrix(idx_.ctx_, fa.batch, rows_a.data(), uint32_t(na), fb.batch, rows_b.data(), uint32_t(nb), prefix ? prefix->batch() : nullptr,
                               prefix ? prefix->rows().data() : nullptr, uint32_t(n), tot.data(), nullptr));
      }
      for (size_t i = 0; i < na; ++i)
        for (size_t j = 0; j < nb; ++j) {
          if (!tot[i * nb + j]) continue;
          group.push_back({fields[level], fa.row_ids[i]});
          group.push_back({fields[level + 1], fb.row_ids[j]});
          const bool go = emit(group, tot[i * nb + j], agg[i * nb + j], limit, out);
          group.pop_back();
          group.pop_back();
          if (!go) return false;
        }
      return true;
    }
    if (remaining == 3 && agg_field.empty() && ag.distinct_field.empty()) {
      // plain counts of the last three levels: fbk_count_cube, the prefix row (if any) as the filter — no prefix ∩ row is
      // materialised.  The leading field in blocks of bp rows (bp x kSumBlock x kSumBlock groups at most: the call's 2^24), the
      // other two in blocks of kSumBlock rows; the groups of a block of leading rows are emitted before the next block is
      // counted, so a small limit ends after the first one.
      const Index::SetField& fb = idx_.sets_.at(fields[level + 1]);
      const Index::SetField& fc = idx_.sets_.at(fields[level + 2]);
      const size_t nb = fb.row_ids.size(), nc = fc.row_ids.size();
      if (nb == 0 || nc == 0) return true;
      const std::vector<uint32_t> rows_b = field_rows(fb), rows_c = field_rows(fc);
      const size_t bp = std::max<size_t>(1, std::min(na, kCubeCells / (std::min(nb, kSumBlock) * std::min(nc, kSumBlock))));
      std::vector<uint64_t> tot, c;
      for (size_t p0 = 0; p0 < na; p0 += bp) {
        const size_t np = std::min(bp, na - p0);
        const std::vector<uint32_t> rp = row_block(rows_a, n, na, p0, np);
        tot.assign(np * nb * nc, 0);
        for (size_t i0 = 0; i0 < nb; i0 += kSumBlock)
          for (size_t j0 = 0; j0 < nc; j0 += kSumBlock) {
            const size_t bi = std::min(kSumBlock, nb - i0), bj = std::min(kSumBlock, nc - j0);
            const std::vector<uint32_t> rb = row_block(rows_b, n, nb, i0, bi), rc = row_block(rows_c, n, nc, j0, bj);
            c.assign(np * bi * bj, 0);
            check(fbk_count_cube(idx_.ctx_, fa.batch, rp.data(), uint32_t(np), fb.batch, rb.data(), uint32_t(bi), fc.batch, rc.data(), uint32_t(bj),
                                 prefix ? prefix->batch() : nullptr, prefix ? prefix->rows().data() : nullptr, uint32_t(n), c.data()));
            for (size_t p = 0; p < np; ++p)
              for (size_t i = 0; i < bi; ++i)
                std::copy(c.begin() + (p * bi + i) * bj, c.begin() + (p * bi + i + 1) * bj, tot.begin() + (p * nb + i0 + i) * nc + j0);
          }
        for (size_t p = 0; p < np; ++p)
          for (size_t i = 0; i < nb; ++i)
            for (size_t j = 0; j < nc; ++j) {
              const uint64_t cnt = tot[(p * nb + i) * nc + j];
              if (!cnt) continue;
              group.push_back({fields[level], fa.row_ids[p0 + p]});
              group.push_back({fields[level + 1], fb.row_ids[i]});
              group.push_back({fields[level + 2], fc.row_ids[j]});
              const bool go = emit(group, cnt, 0, limit, out);
              group.resize(group.size() - 3);
              if (!go) return false;
            }
      }
      return true;
    }
    for (size_t i = 0; i < na; ++i) {  // four or more fields left (three with an aggregate): fix this field's row
      RowSet r = leaf_row(fields[level], fa.row_ids[i]);
      group.push_back({fields[level], fa.row_ids[i]});
      bool go;
      if (prefix) {
        RowSet p = setop(FBK_OP_AND, r, *prefix);
        go = count_rows(p) == 0 ? true : group_by_rec(fields, level + 1, &p, ag, limit, group, out);
      } else {
        go = group_by_rec(fields, level + 1, &r, ag, limit, group, out);
      }
      group.pop_back();
      if (!go) return false;
    }
    return true;
  }

  Index& idx_;
};

}  // namespace fbk
