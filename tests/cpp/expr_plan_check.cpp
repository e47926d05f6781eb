// expr_plan_check.cpp — stand-alone driver of the host planner of fbk_expr_* (featurebase_amd/csrc/fbk_expr_plan.h), built
// WITHOUT HIP and with -fsanitize=address,undefined by tests/test_expr_cpu.py.
//
//   expr_plan_check <corpus>
//
// corpus (text): per case
//     case <n_leaves> <n_prog>
//     leaf <kind> <op> <bit_depth> <lo> <hi> <has_batch>        (n_leaves lines)
//     prog <word> ...                                           (n_prog words)
// One line per case on stdout:
//     OK <depth> <slots> <first_leaf> <n_ins> <ins> ...         the lowered program (fbk_expr::Ins words)
//     ERR <tag>                                                 the rule that refused it
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../featurebase_amd/csrc/fbk_expr_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: expr_plan_check <corpus>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  static const int dummy = 0;
  const fbk_batch* some_batch = reinterpret_cast<const fbk_batch*>(&dummy);  // the planner only asks whether a batch is there
  std::string word;
  while (in >> word) {
    if (word != "case") {
      std::fprintf(stderr, "corpus: expected 'case', got '%s'\n", word.c_str());
      return 2;
    }
    uint32_t n_leaves = 0, n_prog = 0;
    in >> n_leaves >> n_prog;
    std::vector<fbk_expr_leaf> leaves(n_leaves);
    for (uint32_t l = 0; l < n_leaves; ++l) {
      int has_batch = 0;
      fbk_expr_leaf& f = leaves[l];
      in >> word >> f.kind >> f.op >> f.bit_depth >> f.lo >> f.hi >> has_batch;
      f.batch = has_batch ? some_batch : nullptr;
      f.rows = nullptr;
      f.pad = 0;
    }
    in >> word;  // "prog"
    std::vector<uint32_t> prog(n_prog);
    for (uint32_t i = 0; i < n_prog; ++i) in >> prog[i];
    if (!in) {
      std::fprintf(stderr, "corpus: truncated case\n");
      return 2;
    }
    // exact-size copies on the heap: an index past either end is the sanitizer's to report
    fbk_expr::Plan plan;
    const fbk_expr::Error e = fbk_expr::plan(leaves.data(), n_leaves, prog.data(), n_prog, plan);
    if (e) {
      if (e.msg.empty()) {
        std::fprintf(stderr, "an error without a message (%s)\n", e.tag);
        return 3;
      }
      std::printf("ERR %s\n", e.tag);
      continue;
    }
    std::printf("OK %u %u %u %zu", plan.depth, plan.slots, plan.first_leaf, plan.ins.size());
    for (uint32_t w : plan.ins) std::printf(" %u", w);
    std::printf("\n");
  }
  return 0;
}
