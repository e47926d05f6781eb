// fbk_wire_parse.h — the host parsers of the serialised uploads (Pilosa / official roaring images, the ops log, RBF pages):
// offset arithmetic on untrusted bytes, nothing else.  Plain C++, HIP not needed: fbk.hip includes it for the entry points of
// fbk_wire_api.inc, tests/cpp/fuzz_wire_parse.cpp compiles it on its own (with the sanitizers) and runs it over a fuzz corpus.
// Header parsing restates the reference's iterators (roaring.go:1945-2262, 6948-7006) bound check by bound check.  What an
// accepted image promises the device side (k_wire_copy, k_validate_recount): every container's [src, src + bytes) lies inside
// the blob, keys ascend strictly, n is in 1..65536, bytes follows from type and len.
#pragma once
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/fbk.h"

namespace {

// Records the message and returns `code`.  The library defines it (fbk.hip); a stand-alone program supplies its own.
int32_t fail(int32_t code, const std::string& msg);


constexpr uint32_t kMagicNumber = 12348;        // roaring.go:21
constexpr uint32_t kSerialCookieNoRun = 12346;  // official format without run containers
constexpr uint32_t kSerialCookie = 12347;       // official format with a run bitmap
constexpr uint64_t kHeaderBaseSize = 8;         // roaring.go:34

inline uint16_t rd16(const uint8_t* p) { return uint16_t(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t* p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }
inline uint64_t rd64(const uint8_t* p) { return uint64_t(rd32(p)) | (uint64_t(rd32(p + 4)) << 32); }
inline void wr16(uint8_t* p, uint16_t v) { p[0] = uint8_t(v); p[1] = uint8_t(v >> 8); }
inline void wr32(uint8_t* p, uint32_t v) { wr16(p, uint16_t(v)); wr16(p + 2, uint16_t(v >> 16)); }
inline void wr64(uint8_t* p, uint64_t v) { wr32(p, uint32_t(v)); wr32(p + 4, uint32_t(v >> 32)); }

struct WireContainer {
  uint64_t key;
  uint64_t src;  // payload offset in the blob (after the run-count prefix)
  uint32_t type, n, len, bytes, mode;
};

int32_t wire_push(std::vector<WireContainer>& out, uint64_t key, uint32_t type, uint32_t n, uint32_t run_count, uint64_t off,
                  uint64_t len_total, uint32_t mode) {
  WireContainer c;
  c.key = key;
  c.src = off;
  c.type = type;
  c.n = n;
  c.mode = mode;
  if (type == FBK_TYPE_ARRAY) {
    c.len = n;
    c.bytes = n * 2;
  } else if (type == FBK_TYPE_BITMAP) {
    c.len = FBK_BITMAP_WORDS;
    c.bytes = 8192;
  } else if (type == FBK_TYPE_RUN) {
    if (run_count > 32768) return fail(FBK_E_INVALID, "roaring: run container with more than 32768 intervals");
    c.len = run_count;
    c.bytes = run_count * 4;
  } else {
    return fail(FBK_E_INVALID, "roaring: unknown container type " + std::to_string(type));
  }
  if (off > len_total || off < kHeaderBaseSize || off + c.bytes > len_total)
    return fail(FBK_E_INVALID, "roaring: container payload out of bounds");  // roaring.go:2165, 2183
  if (!out.empty() && key <= out.back().key) return fail(FBK_E_INVALID, "roaring: container keys not ascending");
  out.push_back(c);
  return FBK_OK;
}

// NewRoaringIterator + pilosaRoaringIterator.Next / officialRoaringIterator.Next
int32_t wire_parse(const uint8_t* data, uint64_t len, std::vector<WireContainer>& out, uint64_t* ops_off) {
  *ops_off = len;
  if (len < kHeaderBaseSize) return fail(FBK_E_INVALID, "invalid data: not long enough to be a roaring header");
  const uint32_t magic = rd16(data);
  if (magic == kMagicNumber) {
    if (data[2] != 0) return fail(FBK_E_INVALID, "wrong roaring version, file is v" + std::to_string(data[2]) + ", server requires v0");
    const uint64_t keys = rd32(data + 4);
    if (keys == 0) {
      *ops_off = kHeaderBaseSize;  // zero containers but possibly an ops log (roaring.go:1994-2000)
      return FBK_OK;
    }
    if (len < kHeaderBaseSize + keys * 16) return fail(FBK_E_INVALID, "insufficient data for header + offsets");
    const uint8_t* headers = data + kHeaderBaseSize;
    const uint8_t* offsets = headers + keys * 12;
    uint32_t prev32 = uint32_t(kHeaderBaseSize + keys * 16);
    uint64_t chunk = (kHeaderBaseSize + keys * 16) & ~0xFFFFFFFFull;
    out.reserve(keys);
    for (uint64_t i = 0; i < keys; ++i) {
      const uint8_t* h = headers + i * 12;
      const uint32_t type = rd16(h + 8);
      const uint32_t off32 = rd32(offsets + i * 4);
      if (off32 < prev32) chunk += 1ull << 32;  // offsets are u32 and wrap every 4 GiB (roaring.go:2150)
      prev32 = off32;
      uint64_t off = chunk + off32;
      uint32_t run_count = 0;
      if (type == FBK_TYPE_RUN) {
        if (off + 2 > len) return fail(FBK_E_INVALID, "roaring: run count out of bounds");
        run_count = rd16(data + off);
        off += 2;
      }
      if (int32_t rc = wire_push(out, rd64(h), type, uint32_t(rd16(h + 10)) + 1, run_count, off, len, 0)) return rc;
    }
    // Whatever follows the last container is the ops log (Remaining(), roaring.go:2103), which
    // Bitmap.UnmarshalBinary replays (unmarshal_binary.go:66-95); the caller of wire_parse decides
    // what to do with it — silently dropping it would upload stale data.
    *ops_off = out.empty() ? kHeaderBaseSize : out.back().src + out.back().bytes;
    return FBK_OK;
  }
  if (magic == kSerialCookie || magic == kSerialCookieNoRun) {  // readOfficialHeader, roaring.go:6948
    const uint32_t cookie = rd32(data);
    uint64_t pos = 4;
    uint32_t size;
    const uint8_t* is_run = nullptr;
    if (cookie == kSerialCookieNoRun) {
      size = rd32(data + pos);
      pos += 4;
    } else if ((cookie & 0xFFFF) == kSerialCookie) {
      size = uint32_t(uint16_t(cookie >> 16)) + 1;
      const uint64_t rb = (uint64_t(size) + 7) / 8;
      if (pos + rb > len) return fail(FBK_E_INVALID, "malformed bitmap, is-run bitmap overruns buffer");
      is_run = data + pos;
      pos += rb;
    } else {
      return fail(FBK_E_INVALID, "did not find expected serialCookie in header");
    }
    const uint64_t header = pos;
    if (size > (1u << 16)) return fail(FBK_E_INVALID, "it is logically impossible to have more than (1<<16) containers");
    if (pos + 4ull * size >= len)
      return fail(FBK_E_INVALID, "malformed bitmap, key-cardinality slice overruns buffer at " + std::to_string(pos + 4ull * size));
    pos += 4ull * size;
    uint64_t data_off = pos;
    const uint8_t* offsets = nullptr;
    if (!is_run) {
      if (len < pos + 4ull * size) return fail(FBK_E_INVALID, "insufficient data for offsets");
      offsets = data + pos;
    }
    out.reserve(size);
    for (uint32_t i = 0; i < size; ++i) {
      const uint64_t key = rd16(data + header + 4ull * i);
      const uint32_t n = uint32_t(rd16(data + header + 4ull * i + 2)) + 1;
      uint32_t type = n < 4096 ? FBK_TYPE_ARRAY : FBK_TYPE_BITMAP;  // containerTyper, roaring.go:6954
      if (is_run && (is_run[i / 8] & (1u << (i % 8)))) type = FBK_TYPE_RUN;
      if (!is_run) data_off = rd32(offsets + 4ull * i);
      uint32_t run_count = 0;
      if (type == FBK_TYPE_RUN) {
        if (data_off + 2 > len) return fail(FBK_E_INVALID, "roaring: run count out of bounds");
        run_count = rd16(data + data_off);
        data_off += 2;
      }
      if (int32_t rc = wire_push(out, key, type, n, run_count, data_off, len, type == FBK_TYPE_RUN ? 1 : 0)) return rc;
      data_off += out.back().bytes;
    }
    return FBK_OK;
  }
  return fail(FBK_E_INVALID, "unknown roaring magic number " + std::to_string(magic));
}

// ---- RBF (the reference's storage engine file format, rbf/rbf.go) ---------------------------
// Pages are 8 KiB (rbf.go:29).  Page header: pgno u32, flags u32, cellN u16 — BIG endian
// (rbf.go:189-206) — then cellN big-endian u16 cell offsets; cells themselves are written with
// native (little-endian) stores (rbf.go:585-593): leaf cell = key u64, type u32, ElemN u16,
// BitN u32, data at +18; branch cell = leftKey u64, flags u32, childPgno u32 (:637-642).
constexpr uint64_t kRbfPage = 8192;
constexpr uint32_t kRbfLeaf = 2, kRbfBranch = 4;                       // PageTypeLeaf / PageTypeBranch, rbf.go:47-53
constexpr uint32_t kRbfArray = 1, kRbfRle = 2, kRbfBitmap = 3, kRbfBitmapPtr = 4;  // ContainerType, rbf.go:63-69
inline uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }
inline uint32_t be16(const uint8_t* p) { return (uint32_t(p[0]) << 8) | p[1]; }

int32_t rbf_walk(const uint8_t* file, uint64_t len, uint32_t pgno, int depth, std::vector<WireContainer>& out,
                 std::vector<uint8_t>& visited) {
  if (depth > 16) return fail(FBK_E_INVALID, "rbf: b-tree deeper than 16 levels");
  const uint64_t n_pages = len / kRbfPage;
  if (pgno == 0 || pgno >= n_pages)  // "page read out of bounds" (rbf/tx.go readPage)
    return fail(FBK_E_INVALID, "rbf: page read out of bounds: pgno=" + std::to_string(pgno) + " max=" + std::to_string(n_pages ? n_pages - 1 : 0));
  // a tree visits every page once: a branch cell that points back at an ancestor (or a page shared
  // by two parents) is corruption, and without this check a cycle recurses cell_n^16 times
  if (visited.size() < n_pages) visited.resize(n_pages, 0);
  if (visited[pgno]) return fail(FBK_E_INVALID, "rbf: page " + std::to_string(pgno) + " is reachable twice (cycle or shared page in the b-tree)");
  visited[pgno] = 1;
  const uint8_t* page = file + uint64_t(pgno) * kRbfPage;
  const uint32_t flags = be32(page + 4), cell_n = be16(page + 8);
  if (10 + 2ull * cell_n > kRbfPage) return fail(FBK_E_INVALID, "rbf: cell index overruns the page");
  if (flags == kRbfBranch) {
    if (cell_n == 0) return fail(FBK_E_INVALID, "rbf: branch page " + std::to_string(pgno) + " is empty");
    for (uint32_t i = 0; i < cell_n; ++i) {
      const uint32_t off = be16(page + 10 + 2 * i);
      if (off + 16ull > kRbfPage) return fail(FBK_E_INVALID, "rbf: branch cell out of bounds");
      if (int32_t rc = rbf_walk(file, len, rd32(page + off + 12), depth + 1, out, visited)) return rc;
    }
    return FBK_OK;
  }
  if (flags != kRbfLeaf) return fail(FBK_E_INVALID, "rbf: page " + std::to_string(pgno) + " is neither a leaf nor a branch (flags " + std::to_string(flags) + ")");
  for (uint32_t i = 0; i < cell_n; ++i) {
    const uint32_t off = be16(page + 10 + 2 * i);
    if (off + 18ull > kRbfPage) return fail(FBK_E_INVALID, "rbf: leaf cell out of bounds");
    const uint8_t* c = page + off;
    const uint64_t key = rd64(c);
    const uint32_t type = rd32(c + 8), elem_n = rd16(c + 12), bit_n = rd32(c + 14);
    WireContainer w;
    w.key = key;
    w.n = bit_n;
    w.mode = 0;
    const uint64_t data = uint64_t(pgno) * kRbfPage + off + 18;
    if (type == kRbfArray) {
      w.type = FBK_TYPE_ARRAY;
      w.len = elem_n;
      w.bytes = elem_n * 2;
      w.src = data;
    } else if (type == kRbfRle) {
      w.type = FBK_TYPE_RUN;
      w.len = elem_n;
      w.bytes = elem_n * 4;
      w.src = data;
    } else if (type == kRbfBitmapPtr) {
      if (off + 22ull > kRbfPage) return fail(FBK_E_INVALID, "rbf: bitmap pointer out of bounds");
      const uint32_t bp = rd32(c + 18);  // toPgno(cell.Data): the bitmap lives on its own page
      if (bp == 0 || bp >= n_pages)
        return fail(FBK_E_INVALID, "rbf: cannot read page: pgno=" + std::to_string(bp) + " parent=" + std::to_string(pgno));
      if (visited[bp]) return fail(FBK_E_INVALID, "rbf: bitmap page " + std::to_string(bp) + " is referenced twice");
      visited[bp] = 1;
      w.type = FBK_TYPE_BITMAP;
      w.len = FBK_BITMAP_WORDS;
      w.bytes = 8192;
      w.src = uint64_t(bp) * kRbfPage;
    } else if (type == kRbfBitmap) {  // inline bitmap: only exists transiently inside the reference (rbf.go:52)
      return fail(FBK_E_INVALID, "rbf: inline bitmap cell in a stored page");
    } else {
      return fail(FBK_E_INVALID, "rbf: invalid container type: " + std::to_string(type));
    }
    if (w.type != FBK_TYPE_BITMAP && uint64_t(off) + 18 + w.bytes > kRbfPage) return fail(FBK_E_INVALID, "rbf: leaf cell data overruns the page");
    if (w.n == 0 || w.bytes == 0) continue;  // toContainer: empty data -> nil (rbf/cursorx.go:231)
    if (w.n > 65536) return fail(FBK_E_INVALID, "rbf: BitN out of range");
    if (!out.empty() && key <= out.back().key) return fail(FBK_E_INVALID, "rbf: leaf cell keys not ascending");
    out.push_back(w);
  }
  return FBK_OK;
}

// The page walk of fbk_rbf_find_root: the root page of the bitmap `name`, from the root records of the file image.
int32_t rbf_find_root(const uint8_t* f, uint64_t len, const char* name, uint32_t* out_pgno) {
  if (len < 2 * kRbfPage || std::memcmp(f, "\xFFRBF", 4) != 0) return fail(FBK_E_INVALID, "rbf: missing meta page magic");
  const uint64_t n_pages = len / kRbfPage;
  const size_t name_len = std::strlen(name);
  // meta page: root record page number at +20 (rbf.go:138); root record pages chain through an
  // overflow pgno at +8 (rbf.go:158), records = {pgno u32 BE, len u16 BE, name} from +12 (:163)
  for (uint32_t pg = be32(f + 20), hops = 0; pg != 0; ++hops) {
    if (pg >= n_pages || hops > n_pages) return fail(FBK_E_INVALID, "rbf: root record page out of bounds");
    const uint8_t* page = f + uint64_t(pg) * kRbfPage;
    uint64_t pos = 12;
    while (pos + 6 <= kRbfPage) {
      const uint32_t root = be32(page + pos);
      if (root == 0) break;
      const uint32_t sz = be16(page + pos + 4);
      pos += 6;
      if (pos + sz > kRbfPage) return fail(FBK_E_INVALID, "rbf: short root record buffer");
      if (sz == name_len && std::memcmp(page + pos, name, sz) == 0) {
        *out_pgno = root;
        return FBK_OK;
      }
      pos += sz;
    }
    pg = be32(page + 8);
  }
  return fail(FBK_E_INVALID, std::string("rbf: bitmap not found: ") + name);  // ErrBitmapNotFound
}

// ---- the ops log of a Pilosa-format file image (roaring.go:6254-6431, unmarshal_binary.go:66-95) ----
// What follows the last container: a sequence of ops {type u8, value u64, checksum u32 (FNV-1a over everything
// but itself), ...}: add / remove one position (13 bytes), add / remove a batch (value = count, then count u64),
// add / remove a whole serialised bitmap (value = its length, then opN u32, then the image).  The reference
// replays them one by one onto the bitmap it has just unmarshalled; here the containers are unpacked on the
// device as usual, and the log is folded into it with set operations on the device: runs of point / batch ops
// become one "added" and one "removed" image (per position the LAST op wins), a nested image is united /
// subtracted at its place in the sequence.
struct WireOp {
  uint32_t typ = 0;
  std::vector<uint64_t> values;  // add / remove (one value), addN / removeN
  uint64_t img_off = 0, img_len = 0;  // addRoaring / removeRoaring: the nested image inside the blob
};

inline uint32_t fnv1a32(uint32_t h, const uint8_t* p, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
  return h;
}

int32_t ops_parse(const uint8_t* data, uint64_t len, uint64_t off, std::vector<WireOp>& ops) {
  while (off < len) {  // op.UnmarshalBinary, roaring.go:6364-6431
    const uint8_t* d = data + off;
    const uint64_t left = len - off;
    if (left < 13) return fail(FBK_E_INVALID, "roaring ops log: op data out of bounds: len=" + std::to_string(left) + " at offset " + std::to_string(off));
    WireOp op;
    op.typ = d[0];
    const uint64_t value = rd64(d + 1);
    uint32_t h = fnv1a32(2166136261u, d, 9);
    uint64_t size = 13;
    if (op.typ == 0 || op.typ == 1) {
      op.values.push_back(value);
    } else if (op.typ == 2 || op.typ == 3) {
      if (value > (1ull << 59)) return fail(FBK_E_INVALID, "roaring ops log: maximum operation size exceeded");
      size = 13 + value * 8;
      if (left < size) return fail(FBK_E_INVALID, "roaring ops log: op data truncated - expected " + std::to_string(size) + ", got " + std::to_string(left));
      h = fnv1a32(h, d + 13, value * 8);
      op.values.resize(value);
      for (uint64_t i = 0; i < value; ++i) op.values[i] = rd64(d + 13 + 8 * i);
    } else if (op.typ == 4 || op.typ == 5) {
      size = 17 + value;
      if (value > left || left < size) return fail(FBK_E_INVALID, "roaring ops log: op data truncated - expected " + std::to_string(size) + ", got " + std::to_string(left));
      h = fnv1a32(h, d + 13, 4 + value);
      op.img_off = off + 17;
      op.img_len = value;
    } else {
      return fail(FBK_E_INVALID, "roaring ops log: unknown op type: " + std::to_string(op.typ));
    }
    if (rd32(d + 9) != h) return fail(FBK_E_INVALID, "roaring ops log: checksum mismatch: type " + std::to_string(op.typ) + " at offset " + std::to_string(off));
    ops.push_back(std::move(op));
    off += size;
  }
  return FBK_OK;
}

// positions (ascending, distinct) -> array containers in a synthetic image: payloads only, the containers are
// described directly (what wire_parse would have produced)
void positions_image(const std::vector<uint64_t>& pos, std::vector<uint8_t>& img, std::vector<WireContainer>& cs) {
  img.assign(16, 0);  // (payload offsets below the header size never occur in a real image)
  for (size_t i = 0; i < pos.size();) {
    const uint64_t key = pos[i] >> 16;
    size_t j = i;
    while (j < pos.size() && (pos[j] >> 16) == key) ++j;
    WireContainer c;
    c.key = key;
    c.src = img.size();
    c.type = FBK_TYPE_ARRAY;
    c.n = c.len = uint32_t(j - i);
    c.bytes = c.n * 2;
    c.mode = 0;
    for (size_t k = i; k < j; ++k) {
      img.push_back(uint8_t(pos[k]));
      img.push_back(uint8_t(pos[k] >> 8));
    }
    while (img.size() & 15) img.push_back(0);
    cs.push_back(c);
    i = j;
  }
}

}  // namespace
