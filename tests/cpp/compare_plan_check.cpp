// Stand-alone driver of featurebase_amd/csrc/fbk_compare_plan.h for tests/test_bsi_compare_cpu.py (built with
// -fsanitize=address,undefined).  One request per input line, one line per request:
//   P dx dy base_x base_y flags op   -> steps general take_lt take_gt invert ok bits
//                                       bits: bit i of k = base_x - base_y for i = 0 .. 139 as a string of 0 / 1 (sign-extended)
//   K                                -> kMaxDepth kMaxShards kPathOffset
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../featurebase_amd/csrc/fbk_compare_plan.h"

namespace cp = fbk_compare_plan;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char req = 0;
    in >> req;
    if (req == 'P') {
      uint32_t dx, dy, flags;
      int64_t bx, by;
      int32_t op;
      in >> dx >> dy >> bx >> by >> flags >> op;
      const cp::Offset k = cp::offset(bx, by);
      const cp::Combine c = cp::combine(op);
      std::string bits;
      for (uint32_t i = 0; i < 140; ++i) bits += cp::offset_bit(k, i) ? '1' : '0';
      // offset_low is what the kernel shifts: it must agree with offset_bit below 64
      for (uint32_t i = 0; i < 64; ++i)
        if (((cp::offset_low(k) >> i) & 1) != cp::offset_bit(k, i)) return 4;
      std::printf("%u %d %d %d %d %d %s\n", cp::steps(dx, dy, k, flags), int(cp::general(k, flags)), int(c.take_lt), int(c.take_gt), int(c.invert), int(c.ok),
                  bits.c_str());
    } else if (req == 'K') {
      std::printf("%u %u %u\n", cp::kMaxDepth, cp::kMaxShards, cp::kPathOffset);
    } else {
      return 2;
    }
    if (!in) return 3;
  }
  return 0;
}
