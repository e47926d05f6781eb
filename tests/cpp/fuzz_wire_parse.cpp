// fuzz_wire_parse.cpp — stand-alone host program: the parsers of featurebase_amd/csrc/fbk_wire_parse.h over a fuzz corpus
// (tests/wire_fuzz_gen.py writes it; tests/test_wire_fuzz_cpu.py builds this with the address and undefined-behaviour
// sanitizers, tests/test_gpu_fuzz_wire.py without).  Host code only:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined tests/cpp/fuzz_wire_parse.cpp -o build/fuzz_wire_parse && build/fuzz_wire_parse CORPUS
// Corpus: records {kind u32 (0 roaring image, 1 RBF file), name_len u32, name, len u64, bytes}, little endian, to the end of the file.
// Every record is copied into an allocation of exactly its size, so a read past the image is a sanitizer report.  A roaring
// image goes the way of fbk_batch_upload_roaring: wire_parse, ops_parse from ops_off, wire_parse on every nested image; an RBF
// file through rbf_find_root(name) and rbf_walk.  What an accepted case promises the device side is checked here (violation():
// exit status 1); one JSON line per case goes to stdout:
//   {"i":N,"ok":false,"msg":"..."}
//   {"i":N,"ok":true,"root":P,"base":[D...],"ops":[[type,n_values,[D...]]...]}   D = [key,type,n,len,src%16,bytes,mode,branch]
// branch: the path k_wire_copy (fbk_wire_kernels.hip.h) takes for the descriptor when the blob and the arena are 16-byte aligned:
// 0 16-byte vectors, 1 dwords + byte tail, 2 u16 + odd byte, 3 bytes, 4 run conversion by dwords, 5 run conversion by bytes.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../featurebase_amd/csrc/fbk_wire_parse.h"

namespace {
std::string g_msg;
int32_t fail(int32_t code, const std::string& msg) {
  g_msg = msg;
  return code;
}
}  // namespace

static int g_violations = 0;
static void violation(uint64_t idx, const char* where, const std::string& what) {
  std::fprintf(stderr, "CONTRACT VIOLATION case %llu (%s): %s\n", (unsigned long long)idx, where, what.c_str());
  ++g_violations;
}

// the same expression as k_wire_copy, with src_base = dst_base = 0 (mod 16) and d.dst a multiple of 16
static int copy_branch(const WireContainer& c) {
  const uint64_t al = c.src;
  if (c.mode == 1) return (al & 3) == 0 ? 4 : 5;
  if ((al & 15) == 0 && (c.bytes & 15) == 0) return 0;
  if ((al & 3) == 0) return 1;
  if ((al & 1) == 0) return 2;
  return 3;
}

static void check_contract(uint64_t idx, const char* where, const std::vector<WireContainer>& cs, uint64_t blob_len) {
  for (size_t i = 0; i < cs.size(); ++i) {
    const WireContainer& c = cs[i];
    const std::string at = "container " + std::to_string(i) + " key " + std::to_string(c.key);
    if (c.src > blob_len || c.bytes > blob_len - c.src)
      violation(idx, where, at + ": [src, src + bytes) = [" + std::to_string(c.src) + ", +" + std::to_string(c.bytes) + ") leaves the blob of " + std::to_string(blob_len));
    if (i && c.key <= cs[i - 1].key) violation(idx, where, at + ": keys not strictly ascending");
    if (c.n < 1 || c.n > 65536) violation(idx, where, at + ": n = " + std::to_string(c.n));
    if (c.type == FBK_TYPE_ARRAY) {
      if (c.len > 65536 || c.bytes != c.len * 2) violation(idx, where, at + ": array len / bytes");
    } else if (c.type == FBK_TYPE_RUN) {
      if (c.len > 32768 || c.bytes != c.len * 4) violation(idx, where, at + ": run len / bytes");
    } else if (c.type == FBK_TYPE_BITMAP) {
      if (c.len != FBK_BITMAP_WORDS || c.bytes != 8192) violation(idx, where, at + ": bitmap len / bytes");
    } else {
      violation(idx, where, at + ": type " + std::to_string(c.type));
    }
    if (c.mode > 1 || (c.mode == 1 && c.type != FBK_TYPE_RUN)) violation(idx, where, at + ": mode");
  }
}

static std::string json_str(const std::string& s) {
  std::string o = "\"";
  for (unsigned char ch : s) {
    if (ch == '"' || ch == '\\') {
      o += '\\';
      o += char(ch);
    } else if (ch < 0x20 || ch >= 0x7F) {
      char b[8];
      std::snprintf(b, sizeof b, "\\u%04x", ch);
      o += b;
    } else {
      o += char(ch);
    }
  }
  return o + "\"";
}

static std::string descs_json(const std::vector<WireContainer>& cs) {
  std::string o = "[";
  for (size_t i = 0; i < cs.size(); ++i) {
    const WireContainer& c = cs[i];
    if (i) o += ",";
    o += "[" + std::to_string(c.key) + "," + std::to_string(c.type) + "," + std::to_string(c.n) + "," + std::to_string(c.len) + "," +
         std::to_string(c.src & 15) + "," + std::to_string(c.bytes) + "," + std::to_string(c.mode) + "," + std::to_string(copy_branch(c)) + "]";
  }
  return o + "]";
}

static void reject(uint64_t idx) { std::printf("{\"i\":%llu,\"ok\":false,\"msg\":%s}\n", (unsigned long long)idx, json_str(g_msg).c_str()); }

static void run_roaring(uint64_t idx, const uint8_t* blob, uint64_t len) {
  std::vector<WireContainer> base;
  uint64_t ops_off = len;
  if (wire_parse(blob, len, base, &ops_off)) return reject(idx);
  check_contract(idx, "image", base, len);
  if (ops_off > len) violation(idx, "image", "ops_off " + std::to_string(ops_off) + " past the blob");
  std::vector<WireOp> ops;
  std::vector<std::vector<WireContainer>> nested;
  if (ops_off < len) {  // upload_roaring_with_ops
    if (ops_parse(blob, len, ops_off, ops)) return reject(idx);
    nested.resize(ops.size());
    for (size_t i = 0; i < ops.size(); ++i) {
      if (ops[i].typ >= 4) {
        if (ops[i].img_off > len || ops[i].img_len > len - ops[i].img_off) {
          violation(idx, "ops", "nested image of op " + std::to_string(i) + " leaves the blob");
          continue;
        }
        uint64_t inner_ops = 0;
        if (wire_parse(blob + ops[i].img_off, ops[i].img_len, nested[i], &inner_ops)) return reject(idx);
        check_contract(idx, "nested image (own offsets)", nested[i], ops[i].img_len);
        for (WireContainer& c : nested[i]) c.src += ops[i].img_off;
        check_contract(idx, "nested image (rebased)", nested[i], len);
      } else if (!ops[i].values.empty()) {  // the synthetic image the point / batch ops become
        std::vector<uint64_t> pos = ops[i].values;
        std::sort(pos.begin(), pos.end());
        pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
        std::vector<uint8_t> img;
        std::vector<WireContainer> cs;
        positions_image(pos, img, cs);
        check_contract(idx, "positions image", cs, img.size());
      }
    }
  }
  std::string o = "{\"i\":" + std::to_string(idx) + ",\"ok\":true,\"root\":0,\"base\":" + descs_json(base) + ",\"ops\":[";
  for (size_t i = 0; i < ops.size(); ++i)
    o += std::string(i ? "," : "") + "[" + std::to_string(ops[i].typ) + "," + std::to_string(ops[i].values.size()) + "," + descs_json(nested[i]) + "]";
  std::printf("%s]}\n", o.c_str());
}

static void run_rbf(uint64_t idx, const uint8_t* file, uint64_t len, const std::string& name) {
  uint32_t root = 0;
  if (rbf_find_root(file, len, name.c_str(), &root)) return reject(idx);
  std::vector<WireContainer> cs;
  std::vector<uint8_t> visited;
  if (rbf_walk(file, len, root, 0, cs, visited)) return reject(idx);
  check_contract(idx, "rbf", cs, len);
  std::printf("{\"i\":%llu,\"ok\":true,\"root\":%u,\"base\":%s,\"ops\":[]}\n", (unsigned long long)idx, root, descs_json(cs).c_str());
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s CORPUS\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  uint64_t idx = 0;
  for (;; ++idx) {
    uint8_t head[8];
    const size_t got = std::fread(head, 1, 8, f);
    if (got == 0) break;
    if (got != 8) {
      std::fprintf(stderr, "corpus: short record header at case %llu\n", (unsigned long long)idx);
      return 2;
    }
    const uint32_t kind = rd32(head), name_len = rd32(head + 4);
    std::string name(name_len, '\0');
    uint8_t lenb[8];
    if ((name_len && std::fread(&name[0], 1, name_len, f) != name_len) || std::fread(lenb, 1, 8, f) != 8) {
      std::fprintf(stderr, "corpus: short record at case %llu\n", (unsigned long long)idx);
      return 2;
    }
    const uint64_t len = rd64(lenb);
    uint8_t* blob = static_cast<uint8_t*>(std::malloc(len ? len : 1));  // exactly `len` bytes (one when empty): the sanitizer sees any read past them
    if (!blob || (len && std::fread(blob, 1, len, f) != len)) {
      std::fprintf(stderr, "corpus: short record body at case %llu\n", (unsigned long long)idx);
      return 2;
    }
    g_msg.clear();
    if (kind == 0) run_roaring(idx, blob, len);
    else if (kind == 1) run_rbf(idx, blob, len, name);
    else {
      std::fprintf(stderr, "corpus: unknown kind %u at case %llu\n", kind, (unsigned long long)idx);
      return 2;
    }
    std::free(blob);
  }
  std::fclose(f);
  std::fflush(stdout);
  if (g_violations) {
    std::fprintf(stderr, "%d contract violation(s)\n", g_violations);
    return 1;
  }
  std::fprintf(stderr, "fuzz_wire_parse: %llu cases, contract ok\n", (unsigned long long)idx);
  return 0;
}
