// fbk_expr_plan.h — host planner of fbk_expr_* (HIP-free: compiled into the library and into the stand-alone check of the
// tests).  A filter arrives as leaves plus a postfix program (include/fbk.h); this header validates it, computes the stack
// depth it needs and lowers it to the instruction list k_expr_slot interprets (fbk_expr.hip.h).
//
// The internal machine has an accumulator X, the BSI scans' matched register M, and a stack of saved fragments (LDS).
// Lowering decides the cost:
//   * an operator with a ROW leaf on either side becomes "X op= leaf" — nothing is saved;
//   * where both operands are subtrees, the one that needs more saved values is evaluated first (Sethi-Ullman), the
//     other after one PUSH, and a POP instruction combines them (both operand orders of ANDNOT exist, so every operator
//     may be reordered);
//   * a BSI leaf is expanded in place into the plane program of its predicate (fbk_bsi_prog.h: the programs fbk_bsi_range
//     and fbk_bsi_range_between run), S of that program being one more saved value.
// need(program) <= the postfix program's own depth, so FBK_EXPR_MAX_DEPTH bounds the kernel's LDS.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fbk_bsi_prog.h"

namespace fbk_expr {

// instruction word: op << 24 | leaf << 12 | row of the leaf's fragment (0 for a ROW leaf)
enum Ins : uint32_t {
  kLoad = 0,      // X = T
  kAnd = 1,       // X &= T
  kAndn = 2,      // X &= ~T
  kOr = 3,        // X |= T
  kXor = 4,       // X ^= T
  kAndnRev = 5,   // X = T & ~X
  kMorXA = 6,     // M |= X & T
  kMorXAn = 7,    // M |= X & ~T      (ops <= kMorXAn read a container T)
  kMZero = 8,     // M = 0
  kXFromM = 9,    // X = M
  kZeroX = 10,    // X = 0
  kPush = 11,     // stack[sp++] = X
  kPop = 16,      // kPop + {kAnd .. kAndnRev}: T = stack[--sp], then as above
};
constexpr uint32_t kLeafShift = 12, kRowMask = 0xFFFu;
inline uint32_t ins_word(uint32_t op, uint32_t leaf = 0, uint32_t row = 0) { return (op << 24) | (leaf << kLeafShift) | row; }

struct Error {
  const char* tag = nullptr;  // nullptr: no error
  std::string msg;
  explicit operator bool() const { return tag != nullptr; }
};
inline Error err(const char* tag, std::string msg) {
  Error e;
  e.tag = tag;
  e.msg = std::move(msg);
  return e;
}

struct Plan {
  uint32_t depth = 0;         // values on the stack of the postfix program at once
  uint32_t slots = 0;         // saved fragments the lowered program needs at once
  uint32_t first_leaf = 0;    // the leaf of the first PUSH (the output rows take its keys)
  std::vector<uint32_t> ins;  // the lowered program
};

// Every rule of include/fbk.h, in a fixed order (limits, leaves, program words, what is left); *depth = the stack depth.
inline Error validate(const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, uint32_t* depth) {
  if (n_prog == 0) return err("n_prog", "expr: empty program");
  if (n_prog > FBK_EXPR_MAX_PROG) return err("max_prog", "expr: more than FBK_EXPR_MAX_PROG (" + std::to_string(FBK_EXPR_MAX_PROG) + ") program words");
  if (n_leaves > FBK_EXPR_MAX_LEAVES) return err("max_leaves", "expr: more than FBK_EXPR_MAX_LEAVES (" + std::to_string(FBK_EXPR_MAX_LEAVES) + ") leaves");
  for (uint32_t l = 0; l < n_leaves; ++l) {
    const fbk_expr_leaf& f = leaves[l];
    if (!f.batch) return err("null_batch", "expr: leaf " + std::to_string(l) + " has no batch");
    if (f.kind > FBK_EXPR_BETWEEN) return err("leaf_kind", "expr: leaf " + std::to_string(l) + " has an unknown kind");
    if (f.kind == FBK_EXPR_ROW) continue;
    if (f.bit_depth > 64) return err("bit_depth", "expr: leaf " + std::to_string(l) + ": bit depth > 64");
    if (f.kind == FBK_EXPR_BSI && (f.op < FBK_BSI_EQ || f.op > FBK_BSI_GTE)) return err("range_op", "expr: leaf " + std::to_string(l) + ": invalid range operation");
  }
  uint32_t sp = 0, deepest = 0;
  for (uint32_t i = 0; i < n_prog; ++i) {
    const uint32_t opc = prog[i] >> 24, leaf = prog[i] & 0xFFFFFFu;
    if (opc > FBK_EXPR_ANDNOT) return err("opcode", "expr: word " + std::to_string(i) + ": unknown opcode");
    if (opc == FBK_EXPR_PUSH) {
      if (leaf >= n_leaves) return err("leaf_index", "expr: word " + std::to_string(i) + ": leaf index past n_leaves");
      if (++sp > deepest) deepest = sp;
      if (sp > FBK_EXPR_MAX_DEPTH) return err("max_depth", "expr: more than FBK_EXPR_MAX_DEPTH (" + std::to_string(FBK_EXPR_MAX_DEPTH) + ") values on the stack");
    } else {
      if (sp < 2) return err("underflow", "expr: word " + std::to_string(i) + ": stack underflow");
      --sp;
    }
  }
  if (sp != 1) return err("leftover", "expr: the program leaves " + std::to_string(sp) + " values, not one");
  if (depth) *depth = deepest;
  return Error();
}

namespace detail {

struct Node {
  int32_t leaf = -1;  // >= 0: a leaf
  uint32_t op = 0;    // FBK_EXPR_AND .. _ANDNOT
  int32_t a = -1, b = -1;
  uint32_t need = 0;  // saved fragments needed to leave this node's value in X
  bool a_first = true;
};

struct Lowering {
  const fbk_expr_leaf* leaves;
  std::vector<Node> nodes;
  std::vector<std::vector<uint32_t>> bsi;  // per leaf: its plane program (fbk_bsi_prog.h words), empty for ROW leaves
  std::vector<uint32_t>* out;

  bool is_row(int32_t n) const { return nodes[n].leaf >= 0 && leaves[nodes[n].leaf].kind == FBK_EXPR_ROW; }

  void emit_bsi(uint32_t leaf) {
    for (uint32_t w : bsi[leaf]) {
      const uint32_t op = w >> 24, row = w & 0xFFFFFFu;
      switch (op) {
        case fbk::kLoadX: out->push_back(ins_word(kLoad, leaf, row)); break;
        case fbk::kAndX: out->push_back(ins_word(kAnd, leaf, row)); break;
        case fbk::kAndnX: out->push_back(ins_word(kAndn, leaf, row)); break;
        case fbk::kMorXA: out->push_back(ins_word(kMorXA, leaf, row)); break;
        case fbk::kMorXAn: out->push_back(ins_word(kMorXAn, leaf, row)); break;
        case fbk::kMZero: out->push_back(ins_word(kMZero)); break;
        case fbk::kXFromM: out->push_back(ins_word(kXFromM)); break;
        case fbk::kZeroX: out->push_back(ins_word(kZeroX)); break;
        case fbk::kSaveX: out->push_back(ins_word(kPush)); break;            // S is the top of the stack
        case fbk::kOrXS: out->push_back(ins_word(kPop + kOr)); break;        // X |= S
        case fbk::kAndnXS: out->push_back(ins_word(kPop + kAndn)); break;    // X &= ~S
        default: break;
      }
    }
  }

  // the instruction for X = X op T (rev: X = T op X)
  static uint32_t apply_op(uint32_t op, bool rev) {
    switch (op) {
      case FBK_EXPR_AND: return kAnd;
      case FBK_EXPR_OR: return kOr;
      case FBK_EXPR_XOR: return kXor;
      default: return rev ? kAndnRev : kAndn;
    }
  }

  void emit(int32_t n) {
    const Node& nd = nodes[n];
    if (nd.leaf >= 0) {
      if (is_row(n)) out->push_back(ins_word(kLoad, uint32_t(nd.leaf)));
      else emit_bsi(uint32_t(nd.leaf));
      return;
    }
    if (is_row(nd.b)) {
      emit(nd.a);
      out->push_back(ins_word(apply_op(nd.op, false), uint32_t(nodes[nd.b].leaf)));
    } else if (is_row(nd.a)) {
      emit(nd.b);
      out->push_back(ins_word(apply_op(nd.op, true), uint32_t(nodes[nd.a].leaf)));
    } else if (nd.a_first) {
      emit(nd.a);
      out->push_back(ins_word(kPush));
      emit(nd.b);
      out->push_back(ins_word(kPop + apply_op(nd.op, true)));  // X = saved(a) op X(b)
    } else {
      emit(nd.b);
      out->push_back(ins_word(kPush));
      emit(nd.a);
      out->push_back(ins_word(kPop + apply_op(nd.op, false)));  // X(a) op= saved(b)
    }
  }
};

}  // namespace detail

// validate + lower.  `leaves` need their kind / op / bit_depth / lo / hi (and a non-NULL batch) only.
inline Error plan(const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog, Plan& out) {
  if (Error e = validate(leaves, n_leaves, prog, n_prog, &out.depth)) return e;
  detail::Lowering lo;
  lo.leaves = leaves;
  lo.bsi.resize(n_leaves);
  lo.out = &out.ins;
  std::vector<uint32_t> leaf_need(n_leaves, 0);
  std::vector<bool> have(n_leaves, false);
  std::vector<int32_t> st;
  bool first = true;
  for (uint32_t i = 0; i < n_prog; ++i) {
    const uint32_t opc = prog[i] >> 24, leaf = prog[i] & 0xFFFFFFu;
    detail::Node nd;
    if (opc == FBK_EXPR_PUSH) {
      if (first) out.first_leaf = leaf, first = false;
      const fbk_expr_leaf& f = leaves[leaf];
      if (f.kind != FBK_EXPR_ROW && !have[leaf]) {
        fbk_bsi::BsiProg p;
        if (f.kind == FBK_EXPR_BETWEEN) fbk_bsi::gen_between(p, f.bit_depth, f.lo, f.hi);
        else if (!fbk_bsi::gen_range_op(p, f.op, f.bit_depth, f.lo)) return err("range_op", "expr: invalid range operation");
        for (uint32_t w : p.v)
          if ((w >> 24) == fbk::kSaveX) leaf_need[leaf] = 1;
        lo.bsi[leaf] = std::move(p.v);
        have[leaf] = true;
      }
      nd.leaf = int32_t(leaf);
      nd.need = leaf_need[leaf];
    } else {
      nd.op = opc;
      nd.b = st.back();
      st.pop_back();
      nd.a = st.back();
      st.pop_back();
      const uint32_t na = lo.nodes[nd.a].need, nb = lo.nodes[nd.b].need;
      if (lo.is_row(nd.b)) nd.need = na;
      else if (lo.is_row(nd.a)) nd.need = nb;
      else {
        const uint32_t ab = std::max(na, 1 + nb), ba = std::max(nb, 1 + na);
        nd.a_first = ab <= ba;
        nd.need = std::min(ab, ba);
      }
    }
    st.push_back(int32_t(lo.nodes.size()));
    lo.nodes.push_back(nd);
  }
  out.slots = lo.nodes[st.back()].need;
  out.ins.clear();
  lo.emit(st.back());
  return Error();
}

// the containers a lowered program reads per (shard, slot): its instructions with an operand (ops <= kMorXAn)
inline uint32_t operand_reads(const std::vector<uint32_t>& ins) {
  uint32_t n = 0;
  for (uint32_t w : ins) n += (w >> 24) <= kMorXAn ? 1u : 0u;
  return n;
}

// Rows of the field per block of k_expr_rows_vs_filter (fbk_expr_topk.hip.h), which evaluates the tree once per block: a block
// reads L + rpb containers, L = operand_reads(program).  The rule of k_rows_vs_filter's launches — halve while the grid is short
// of 2048 blocks and more than 64 rows are left, then a multiple of 64, at least 64 — with one more condition: a split is taken
// only while (chunks - 1) * L <= n_a for the chunks it leads to, so that re-evaluating the tree at most doubles the containers
// read (chunks * L + n_a <= 2 * n_a + L).  L = 0 is the rule of k_rows_vs_filter itself.
inline uint32_t rows_per_block(uint32_t n_a, uint32_t n_shards_in_pass, uint32_t L) {
  auto rounded = [](uint32_t r) { return std::max<uint32_t>(64u, (r + 63u) & ~63u); };
  uint32_t rpb = n_a;
  while (rpb > 64 && uint64_t(n_shards_in_pass) * 16 * ((n_a + rpb - 1) / rpb) < 2048) {
    const uint32_t half = (rpb + 1) / 2, r = rounded(half);
    const uint64_t chunks = (uint64_t(n_a) + r - 1) / r;
    if ((chunks - 1) * L > n_a) break;
    rpb = half;
  }
  return rounded(rpb);
}

}  // namespace fbk_expr
