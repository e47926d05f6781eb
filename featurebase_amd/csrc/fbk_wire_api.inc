// fbk_wire_api.inc — host side of the serialised-roaring entry points (included by fbk.hip).
// The images are parsed by fbk_wire_parse.h (plain C++); the payload movement is done on the device
// (fbk_wire_kernels.hip.h).

namespace {

// Shared tail of the serialised uploads: containers (ascending keys) located inside `blob` ->
// batch rows (distinct key >> 4) + one device unpack launch.
int32_t wire_upload(fbk_ctx* ctx, const uint8_t* blob, uint64_t len, const std::vector<WireContainer>& cs,
                    fbk_batch** out_batch, uint64_t* out_row_ids, uint32_t row_cap, uint32_t* out_n_rows, const char* what,
                    const std::vector<uint64_t>* forced_rows = nullptr) {
  // rows of the batch: the distinct key >> 4 of the containers, or (ops-log replay: several images laid out over
  // one common row list) an ascending list that contains them all — rows without a container are all nil
  std::vector<uint64_t> row_ids;
  if (forced_rows) row_ids = *forced_rows;
  else
    for (const WireContainer& c : cs)
      if (row_ids.empty() || row_ids.back() != (c.key >> 4)) row_ids.push_back(c.key >> 4);
  if (row_ids.size() > (1u << 27)) return fail(FBK_E_INVALID, std::string(what) + ": too many rows");
  if (out_n_rows) *out_n_rows = uint32_t(row_ids.size());
  if (out_row_ids) {
    if (row_ids.size() > row_cap) return fail(FBK_E_CAPACITY, "row id buffer too small");
    std::memcpy(out_row_ids, row_ids.data(), row_ids.size() * 8);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  fbk_batch* b = new (std::nothrow) fbk_batch();
  if (!b) return fail(FBK_E_NOMEM, "host allocation failed");
  b->ctx = ctx;
  b->n_rows = uint32_t(row_ids.size());
  const uint64_t n_slots = uint64_t(b->n_rows) * fbk::kSlots;
  b->h_slots.assign(n_slots, Slot{0, 0, 0});
  b->h_keys.assign(n_slots, 0);
  std::vector<fbk::WireDesc> descs(cs.size());
  uint64_t off = 0, row = 0;
  bool dense = n_slots > 0 && cs.size() == n_slots;
  for (size_t i = 0; i < cs.size(); ++i) {
    const WireContainer& c = cs[i];
    while (row < row_ids.size() && row_ids[row] != (c.key >> 4)) ++row;
    if (row == row_ids.size()) {
      delete b;
      return fail(FBK_E_INVALID, std::string(what) + ": container key outside the row list");
    }
    const uint64_t s = row * fbk::kSlots + (c.key & 15);
    b->h_slots[s] = Slot{off, c.len, fbk::make_tn(c.type, c.n)};
    b->h_keys[s] = c.key;
    if (c.type != FBK_TYPE_BITMAP || off != s * 8192ull) dense = false;
    descs[i] = fbk::WireDesc{c.src, off, c.bytes, c.mode};
    off += align16(c.bytes);
  }
  b->arena_bytes = off;
  b->dense = dense;
  DevBuf dblob, ddesc;
  hipError_t e = ctx_malloc(ctx, reinterpret_cast<void**>(&b->d_arena), std::max<uint64_t>(off, 16));
  if (e == hipSuccess) e = ctx_malloc(ctx, reinterpret_cast<void**>(&b->d_slots), std::max<uint64_t>(n_slots, 1) * sizeof(Slot));
  if (e == hipSuccess) e = dblob.alloc(ctx, std::max<uint64_t>(len, 16));
  if (e == hipSuccess) e = ddesc.alloc(ctx, std::max<uint64_t>(descs.size(), 1) * sizeof(fbk::WireDesc));
  if (e == hipSuccess && len) e = hipMemcpyAsync(dblob.p, blob, len, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && !descs.empty())
    e = hipMemcpyAsync(ddesc.p, descs.data(), descs.size() * sizeof(fbk::WireDesc), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && n_slots)
    e = hipMemcpyAsync(b->d_slots, b->h_slots.data(), n_slots * sizeof(Slot), hipMemcpyHostToDevice, ctx->stream);
  // The image's headers are untrusted: after the unpack, every container is checked on the device
  // (sorted arrays, ordered runs) and its cardinality recounted (k_validate_recount) — a header N
  // that under-reports would otherwise overflow buffers sized from it (fbk_bsi_distinct) and
  // mis-fire the `n == 65536` shortcuts of the counting kernels.
  DevBuf dbad;
  uint32_t h_bad = 0;
  if (e == hipSuccess) e = dbad.alloc(ctx, 16);
  if (e == hipSuccess) e = hipMemsetAsync(dbad.p, 0, 16, ctx->stream);
  if (e == hipSuccess && !descs.empty()) {
    hipLaunchKernelGGL(fbk::k_wire_copy, dim3(uint32_t((descs.size() + 3) / 4)), dim3(256), 0, ctx->stream, dblob.as<uint8_t>(),
                       b->d_arena, ddesc.as<fbk::WireDesc>(), uint64_t(descs.size()));
    hipLaunchKernelGGL(fbk::k_validate_recount, dim3(uint32_t((n_slots + 3) / 4)), dim3(256), 0, ctx->stream, b->d_slots, b->d_arena,
                       n_slots, dbad.as<uint32_t>());
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(b->h_slots.data(), b->d_slots, n_slots * sizeof(Slot), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, dbad.p, 4, hipMemcpyDeviceToHost, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    free_batch_storage(b);
    return fail(e == hipErrorOutOfMemory ? FBK_E_NOMEM : FBK_E_HIP, std::string(what) + " upload: " + hipGetErrorString(e));
  }
  if (h_bad) {
    free_batch_storage(b);
    return fail(FBK_E_INVALID, std::string(what) + ((h_bad & 1u) ? ": array container not strictly ascending" : ": run container intervals overlap or are unordered"));
  }
  // containers whose recount is zero become nil on both sides (the reference never stores an empty container)
  bool changed = false;
  for (uint64_t s = 0; s < n_slots; ++s) {
    Slot& hs = b->h_slots[s];
    if (fbk::slot_type(hs) != fbk::kTypeNil && fbk::slot_n(hs) == 0) {
      hs = Slot{0, 0, 0};
      b->dense = false;
      changed = true;
    }
  }
  if (changed) {
    e = hipMemcpy(b->d_slots, b->h_slots.data(), n_slots * sizeof(Slot), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      free_batch_storage(b);
      return fail(FBK_E_HIP, std::string(what) + " upload: " + hipGetErrorString(e));
    }
  }
  *out_batch = b;
  return FBK_OK;
}

int32_t upload_roaring_with_ops(fbk_ctx* ctx, const uint8_t* blob, uint64_t len, const std::vector<WireContainer>& base, uint64_t ops_off,
                                fbk_batch** out_batch, uint64_t* out_row_ids, uint32_t row_cap, uint32_t* out_n_rows) {
  std::vector<WireOp> ops;
  if (int32_t rc = ops_parse(blob, len, ops_off, ops)) return rc;
  // nested images: containers only (ImportRoaringBits iterates containers, roaring.go:2380-2391; the reference drops
  // the error of a malformed nested image — here it is reported)
  std::vector<std::vector<WireContainer>> nested(ops.size());
  std::vector<uint64_t> rows;
  for (const WireContainer& c : base) rows.push_back(c.key >> 4);
  for (size_t i = 0; i < ops.size(); ++i) {
    if (ops[i].typ >= 4) {
      uint64_t inner_ops = 0;
      if (int32_t rc = wire_parse(blob + ops[i].img_off, ops[i].img_len, nested[i], &inner_ops)) return rc;
      for (WireContainer& c : nested[i]) {
        c.src += ops[i].img_off;  // offsets relative to the outer blob
        rows.push_back(c.key >> 4);
      }
    } else {
      for (uint64_t v : ops[i].values) rows.push_back(v >> 20);
    }
  }
  std::sort(rows.begin(), rows.end());
  rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
  if (rows.size() > (1u << 27)) return fail(FBK_E_INVALID, "roaring: too many rows");
  if (out_n_rows) *out_n_rows = uint32_t(rows.size());
  if (out_row_ids) {
    if (rows.size() > row_cap) return fail(FBK_E_CAPACITY, "row id buffer too small");
    std::memcpy(out_row_ids, rows.data(), rows.size() * 8);
  }
  fbk_batch* cur = nullptr;
  if (int32_t rc = wire_upload(ctx, blob, len, base, &cur, nullptr, 0, nullptr, "roaring", &rows)) return rc;
  std::vector<uint32_t> ident(rows.size());
  for (size_t i = 0; i < ident.size(); ++i) ident[i] = uint32_t(i);
  // cur = cur <op> other (both laid out over `rows`); other is consumed
  auto fold = [&](int32_t op, fbk_batch* other) -> int32_t {
    fbk_batch* next = nullptr;
    const int32_t rc = fbk_setop(ctx, op, cur, ident.data(), other, ident.data(), ident.size(), FBK_SETOP_OPTIMIZE, &next, nullptr);
    (void)fbk_batch_free(ctx, other);
    if (rc) return rc;
    (void)fbk_batch_free(ctx, cur);
    cur = next;
    return FBK_OK;
  };
  std::vector<std::pair<uint64_t, uint64_t>> pending;  // (position, sequence << 1 | add)
  uint64_t seq = 0;
  auto flush = [&]() -> int32_t {
    if (pending.empty()) return FBK_OK;
    std::sort(pending.begin(), pending.end());
    std::vector<uint64_t> added, removed;
    for (size_t i = 0; i < pending.size(); ++i)
      if (i + 1 == pending.size() || pending[i + 1].first != pending[i].first)  // the last op on this position
        ((pending[i].second & 1) ? added : removed).push_back(pending[i].first);
    pending.clear();
    for (int pass = 0; pass < 2; ++pass) {
      const std::vector<uint64_t>& pos = pass == 0 ? added : removed;
      if (pos.empty()) continue;
      std::vector<uint8_t> img;
      std::vector<WireContainer> cs;
      positions_image(pos, img, cs);
      fbk_batch* delta = nullptr;
      if (int32_t rc = wire_upload(ctx, img.data(), img.size(), cs, &delta, nullptr, 0, nullptr, "roaring ops", &rows)) return rc;
      if (int32_t rc = fold(pass == 0 ? FBK_OP_OR : FBK_OP_ANDNOT, delta)) return rc;
    }
    return FBK_OK;
  };
  int32_t rc = FBK_OK;
  for (size_t i = 0; i < ops.size() && !rc; ++i) {
    const WireOp& op = ops[i];
    if (op.typ < 4) {
      for (uint64_t v : op.values) pending.emplace_back(v, (seq++ << 1) | ((op.typ & 1) ? 0u : 1u));  // types 0, 2 add; 1, 3 remove
    } else {
      rc = flush();
      if (!rc && !nested[i].empty()) {
        fbk_batch* img = nullptr;
        rc = wire_upload(ctx, blob, len, nested[i], &img, nullptr, 0, nullptr, "roaring ops", &rows);
        if (!rc) rc = fold(op.typ == 4 ? FBK_OP_OR : FBK_OP_ANDNOT, img);
      }
    }
  }
  if (!rc) rc = flush();
  if (rc) {
    (void)fbk_batch_free(ctx, cur);
    return rc;
  }
  *out_batch = cur;
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_batch_upload_roaring(fbk_ctx* ctx, const void* data, uint64_t len, fbk_batch** out_batch,
                                 uint64_t* out_row_ids, uint32_t row_cap, uint32_t* out_n_rows) try {
  FBK_ENTER(ctx);
  if (!ctx || !out_batch || (len && !data)) return fail(FBK_E_INVALID, "NULL argument");
  *out_batch = nullptr;
  if (out_n_rows) *out_n_rows = 0;
  std::vector<WireContainer> cs;
  const uint8_t* blob = static_cast<const uint8_t*>(data);
  uint64_t ops_off = len;
  if (int32_t rc = wire_parse(blob, len, cs, &ops_off)) return rc;
  if (ops_off < len)  // a file image with an ops log behind its containers: Bitmap.UnmarshalBinary replays it (unmarshal_binary.go:66-95)
    return upload_roaring_with_ops(ctx, blob, len, cs, ops_off, out_batch, out_row_ids, row_cap, out_n_rows);
  return wire_upload(ctx, blob, len, cs, out_batch, out_row_ids, row_cap, out_n_rows, "roaring");
} FBK_ABI_CATCH(ctx)

int32_t fbk_rbf_find_root(const void* file, uint64_t len, const char* name, uint32_t* out_pgno) try {
  if (!file || !name || !out_pgno) return fail(FBK_E_INVALID, "NULL argument");
  *out_pgno = 0;
  return rbf_find_root(static_cast<const uint8_t*>(file), len, name, out_pgno);
} FBK_ABI_CATCH(nullptr)

int32_t fbk_batch_upload_rbf(fbk_ctx* ctx, const void* file, uint64_t len, uint32_t root_pgno, fbk_batch** out_batch,
                             uint64_t* out_row_ids, uint32_t row_cap, uint32_t* out_n_rows) try {
  FBK_ENTER(ctx);
  if (!ctx || !out_batch || !file) return fail(FBK_E_INVALID, "NULL argument");
  *out_batch = nullptr;
  if (out_n_rows) *out_n_rows = 0;
  std::vector<WireContainer> cs;
  const uint8_t* f = static_cast<const uint8_t*>(file);
  std::vector<uint8_t> visited;
  if (int32_t rc = rbf_walk(f, len, root_pgno, 0, cs, visited)) return rc;
  return wire_upload(ctx, f, len, cs, out_batch, out_row_ids, row_cap, out_n_rows, "rbf");
} FBK_ABI_CATCH(ctx)

static int32_t roaring_layout(fbk_batch* b, std::vector<uint64_t>* slots_out, uint64_t* total) {
  uint64_t n = 0, payload = 0, prev_key = 0;
  for (uint64_t s = 0; s < b->h_slots.size(); ++s) {
    const Slot& hs = b->h_slots[s];
    const uint32_t t = fbk::slot_type(hs);
    if (t == fbk::kTypeNil || fbk::slot_n(hs) == 0) continue;  // `if c.N() > 0`, roaring.go:1768
    if (n && b->h_keys[s] <= prev_key) return fail(FBK_E_INVALID, "roaring: batch keys are not strictly ascending in (row, slot) order");
    if (t == fbk::kTypeArray && hs.len > 65535u + 1) return fail(FBK_E_INVALID, "roaring: array too long");
    prev_key = b->h_keys[s];
    payload += t == fbk::kTypeArray ? uint64_t(hs.len) * 2 : t == fbk::kTypeRun ? 2 + uint64_t(hs.len) * 4 : 8192ull;
    ++n;
    if (slots_out) slots_out->push_back(s);
  }
  *total = kHeaderBaseSize + n * 16 + payload;
  return FBK_OK;
}

int32_t fbk_batch_roaring_size(fbk_ctx* ctx, const fbk_batch* batch, uint64_t* out_bytes) try {
  FBK_ENTER(ctx);
  if (!batch || !out_bytes) return fail(FBK_E_INVALID, "NULL argument");
  fbk_batch* b = const_cast<fbk_batch*>(batch);
  if (!ctx) ctx = b->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = refresh_slots(b)) return rc;
  return roaring_layout(b, nullptr, out_bytes);
} FBK_ABI_CATCH(ctx)

int32_t fbk_batch_download_roaring(fbk_ctx* ctx, const fbk_batch* batch, void* out, uint64_t cap, uint64_t* out_len) try {
  FBK_ENTER(ctx);
  if (!batch || !out_len) return fail(FBK_E_INVALID, "NULL argument");
  fbk_batch* b = const_cast<fbk_batch*>(batch);
  if (!ctx) ctx = b->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (int32_t rc = refresh_slots(b)) return rc;
  std::vector<uint64_t> live;
  uint64_t total = 0;
  if (int32_t rc = roaring_layout(b, &live, &total)) return rc;
  *out_len = total;
  if (!out || cap < total) return fail(FBK_E_CAPACITY, "download buffer too small (use fbk_batch_roaring_size)");
  uint8_t* o = static_cast<uint8_t*>(out);
  const uint64_t n = live.size();
  wr32(o, kMagicNumber);  // cookie: MagicNumber | storageVersion(0) << 16 | flags(0) << 24
  wr32(o + 4, uint32_t(n));
  uint8_t* h = o + kHeaderBaseSize;
  const uint64_t payload0 = kHeaderBaseSize + n * 16;
  std::vector<fbk::WireDesc> descs(n);
  uint64_t off = payload0;
  for (uint64_t i = 0; i < n; ++i, h += 12) {
    const Slot& hs = b->h_slots[live[i]];
    const uint32_t t = fbk::slot_type(hs);
    wr64(h, b->h_keys[live[i]]);
    wr16(h + 8, uint16_t(t));
    wr16(h + 10, uint16_t(fbk::slot_n(hs) - 1));
    wr32(o + payload0 - n * 4 + i * 4, uint32_t(off));  // u32 offsets wrap past 4 GiB, as the reference's do
    const uint32_t bytes = t == fbk::kTypeArray ? hs.len * 2 : t == fbk::kTypeRun ? hs.len * 4 : 8192u;
    const uint64_t pre = t == fbk::kTypeRun ? 2 : 0;
    descs[i] = fbk::WireDesc{hs.off, off - payload0 + pre, bytes, t == fbk::kTypeRun ? 2u : 0u};
    off += pre + bytes;
  }
  if (n == 0) return FBK_OK;
  DevBuf dblob, ddesc;
  const uint64_t pbytes = total - payload0;
  HIP_TRY(dblob.alloc(ctx, std::max<uint64_t>(pbytes, 16)));
  HIP_TRY(ddesc.alloc(ctx, n * sizeof(fbk::WireDesc)));
  HIP_TRY(hipMemcpyAsync(ddesc.p, descs.data(), n * sizeof(fbk::WireDesc), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(fbk::k_wire_copy, dim3(uint32_t((n + 3) / 4)), dim3(256), 0, ctx->stream, b->d_arena, dblob.as<uint8_t>(),
                     ddesc.as<fbk::WireDesc>(), n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(o + payload0, dblob.p, pbytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
