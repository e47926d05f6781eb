// fbk_matrix_sum_api.inc — fbk_count_matrix_sum: GroupBy with aggregate=Sum(field=v) in one pass over the operands per shard
// (fbk_matrix_sum.hip.h).  Included by fbk.hip before fbk_prepared_api.inc, whose fbk_query_count_matrix_sum keeps an MsumPlan.
//
// The matrix kernel reads dense rows.  Operands of batches that are not dense are densified a chunk of shards at a time
// (k_densify_rows) into scratch held by the plan; the chunk bytes of the BSI values share that budget:
//   per shard: n_chunks MiB of chunk bytes + 128 KiB per densified row (n_a, n_b, 1 filter row, depth + 2 BSI rows, each for the
//   batches that are not dense) + 16 bytes per pair of per-shard sums and counts;
//   most = max(1, min(n_shards, kMsumScratch / that)), chunk = ceil(n_shards / ceil(n_shards / most)): the shards dealt evenly
//   over the fewest chunks.  (fbk.h documents the arithmetic: the tests rely on it.)

namespace {

constexpr uint64_t kMsumScratch = 1ull << 30;

struct MsumPlan {
  const fbk_batch *a = nullptr, *b = nullptr, *f = nullptr, *bsi = nullptr;
  uint32_t n_a = 0, n_b = 0, n_shards = 0, depth = 0, n_chunks = 0, chunk = 0;
  bool da = false, db = false, df = false, dbsi = false;  // densified per chunk (the batch is not dense)
  DevBuf rows;
  // A, B, filter, BSI base rows as given; identity lists of densified rows; the BSI rows of every shard (densified BSI)
  const uint32_t *ra = nullptr, *rb = nullptr, *rf = nullptr, *rbase = nullptr, *ia = nullptr, *ib = nullptr, *i1 = nullptr, *ibase = nullptr,
                 *rall = nullptr;
  DevBuf chunks, ta, tb, tf, tbsi, dshard, result;
  uint64_t width() const { return uint64_t(n_a) * n_b; }
};

uint32_t msum_chunks_of(uint32_t depth) { return (depth + fbk::kMsumChunkBits - 1) / fbk::kMsumChunkBits; }

int32_t msum_args_ok(const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b,
                     const fbk_batch* filter, const uint32_t* rows_f, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth,
                     uint32_t n_shards) {
  if (!bsi || (n_shards && !base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (!b && n_b != 1) return fail(FBK_E_INVALID, "count_matrix_sum: without B rows (the one-field GroupBy) n_b must be 1");
  if (b) {
    if (int32_t rc = count_matrix_args_ok(a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  } else if (int32_t rc = count_matrix_args_ok(a, rows_a, n_a, a, rows_a, 1, filter, rows_f, n_shards)) {
    return rc;
  }
  if (n_a > 4096 || n_b > 4096) return fail(FBK_E_INVALID, "count_matrix_sum: at most 4096 rows per side");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (int32_t rc = check_rows(rows_a, uint64_t(n_shards) * n_a, a->n_rows, "count_matrix_sum A")) return rc;
  if (b)
    if (int32_t rc = check_rows(rows_b, uint64_t(n_shards) * n_b, b->n_rows, "count_matrix_sum B")) return rc;
  if (filter)
    if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "count_matrix_sum filter")) return rc;
  for (uint32_t s = 0; s < n_shards; ++s)
    if (uint64_t(base_rows[s]) + 2 + bit_depth > bsi->n_rows)
      return fail(FBK_E_INVALID, "bsi: fragment rows (exists, sign, bit planes) exceed the batch");
  return FBK_OK;
}

// Validated arguments -> row lists on the device, scratch and result allocated: everything a run needs (n_shards > 0, width > 0).
int32_t msum_prepare(fbk_ctx* ctx, MsumPlan& p, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                     uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth,
                     uint32_t n_shards) {
  p.a = a, p.b = b, p.f = filter, p.bsi = bsi;
  p.n_a = n_a, p.n_b = n_b, p.n_shards = n_shards, p.depth = bit_depth, p.n_chunks = msum_chunks_of(bit_depth);
  p.da = !a->dense, p.db = b && !b->dense, p.df = filter && !filter->dense, p.dbsi = !bsi->dense;
  const uint64_t row_bytes = uint64_t(fbk::kSlots) * 8192, rps = uint64_t(bit_depth) + 2;
  const uint64_t per_shard = p.n_chunks * fbk::kMsumChunkBytes +
                             row_bytes * ((p.da ? n_a : 0) + (p.db ? n_b : 0) + (p.df ? 1 : 0) + (p.dbsi ? rps : 0)) + 16 * p.width();
  // at most kMsumScratch per chunk, and the shards dealt evenly over the chunks that takes (no short last chunk)
  const uint64_t most = std::max<uint64_t>(1, std::min<uint64_t>(n_shards, kMsumScratch / per_shard));
  const uint64_t passes = (n_shards + most - 1) / most;
  p.chunk = uint32_t((n_shards + passes - 1) / passes);
  const uint32_t c = p.chunk;
  std::vector<uint32_t> ia(p.da ? uint64_t(c) * n_a : 0), ib(p.db ? uint64_t(c) * n_b : 0), i1(c), ibase(p.dbsi ? c : 0),
      all(p.dbsi ? uint64_t(n_shards) * rps : 0);
  for (uint64_t i = 0; i < ia.size(); ++i) ia[i] = uint32_t(i);
  for (uint64_t i = 0; i < ib.size(); ++i) ib[i] = uint32_t(i);
  for (uint32_t i = 0; i < c; ++i) i1[i] = i;
  for (uint64_t i = 0; i < ibase.size(); ++i) ibase[i] = uint32_t(i * rps);
  for (uint32_t s = 0; s < n_shards && p.dbsi; ++s)
    for (uint64_t r = 0; r < rps; ++r) all[uint64_t(s) * rps + r] = uint32_t(base_rows[s] + r);
  const uint32_t* d[9];
  if (int32_t rc = upload_rows_multi(ctx,
                                     {{rows_a, uint64_t(n_shards) * n_a, UINT32_MAX},
                                      {rows_b, b ? uint64_t(n_shards) * n_b : 0, UINT32_MAX},
                                      {rows_f, filter ? uint64_t(n_shards) : 0, UINT32_MAX},
                                      {base_rows, n_shards, UINT32_MAX},
                                      {ia.data(), ia.size(), UINT32_MAX},
                                      {ib.data(), ib.size(), UINT32_MAX},
                                      {i1.data(), i1.size(), UINT32_MAX},
                                      {ibase.data(), ibase.size(), UINT32_MAX},
                                      {all.data(), all.size(), UINT32_MAX}},
                                     p.rows, d))
    return rc;
  p.ra = d[0], p.rb = d[1], p.rf = d[2], p.rbase = d[3], p.ia = d[4], p.ib = d[5], p.i1 = d[6], p.ibase = d[7], p.rall = d[8];
  if (p.n_chunks) HIP_TRY(p.chunks.alloc(ctx, uint64_t(c) * p.n_chunks * fbk::kMsumChunkBytes));
  if (p.da) HIP_TRY(p.ta.alloc(ctx, uint64_t(c) * n_a * row_bytes));
  if (p.db) HIP_TRY(p.tb.alloc(ctx, uint64_t(c) * n_b * row_bytes));
  if (p.df) HIP_TRY(p.tf.alloc(ctx, uint64_t(c) * row_bytes));
  if (p.dbsi) HIP_TRY(p.tbsi.alloc(ctx, uint64_t(c) * rps * row_bytes));
  HIP_TRY(p.dshard.alloc(ctx, uint64_t(c) * 2 * p.width() * 8));
  HIP_TRY(p.result.alloc(ctx, 2 * p.width() * 8));
  return FBK_OK;
}

// One execution, launch-only: p.result = {sums [n_a * n_b] (u64, wrapping), counts [n_a * n_b]}.
int32_t msum_enqueue(fbk_ctx* ctx, MsumPlan& p) {
  if (p.a->dense == p.da || (p.b && p.b->dense == p.db) || (p.f && p.f->dense == p.df) || p.bsi->dense == p.dbsi)
    return fail(FBK_E_INVALID, "count_matrix_sum: a batch changed its layout since the query was prepared");
  const uint64_t width = p.width();
  const uint32_t rps = p.depth + 2, n_a = p.n_a, n_b = p.n_b;
  HIP_TRY(hipMemsetAsync(p.result.p, 0, 2 * width * 8, ctx->stream));
  KernelSpan span(ctx);
  for (uint32_t s0 = 0; s0 < p.n_shards; s0 += p.chunk) {
    const uint32_t ns = std::min(p.chunk, p.n_shards - s0);
    // operands of this chunk: dense batches as they are, the others densified (k_densify_rows, three sources per launch)
    const uint8_t *arA = p.a->d_arena, *arB = p.b ? p.b->d_arena : nullptr, *arF = p.f ? p.f->d_arena : nullptr, *arS = p.bsi->d_arena;
    const uint32_t *ra = p.ra + uint64_t(s0) * n_a, *rb = p.b ? p.rb + uint64_t(s0) * n_b : nullptr, *rf = p.f ? p.rf + s0 : nullptr, *rs = p.rbase + s0;
    std::vector<fbk::DensifySrc> srcs;
    if (p.da) {
      srcs.push_back({p.a->d_slots, p.a->d_arena, ra, uint64_t(ns) * n_a, p.ta.as<uint8_t>()});
      arA = p.ta.as<uint8_t>(), ra = p.ia;
    }
    if (p.db) {
      srcs.push_back({p.b->d_slots, p.b->d_arena, rb, uint64_t(ns) * n_b, p.tb.as<uint8_t>()});
      arB = p.tb.as<uint8_t>(), rb = p.ib;
    }
    if (p.df) {
      srcs.push_back({p.f->d_slots, p.f->d_arena, rf, uint64_t(ns), p.tf.as<uint8_t>()});
      arF = p.tf.as<uint8_t>(), rf = p.i1;
    }
    if (p.dbsi) {
      srcs.push_back({p.bsi->d_slots, p.bsi->d_arena, p.rall + uint64_t(s0) * rps, uint64_t(ns) * rps, p.tbsi.as<uint8_t>()});
      arS = p.tbsi.as<uint8_t>(), rs = p.ibase;
    }
    for (size_t k0 = 0; k0 < srcs.size(); k0 += 3) {
      fbk::DensifyArgs da{};
      uint64_t cells = 0;
      for (size_t k = k0; k < std::min(srcs.size(), k0 + 3); ++k) {
        da.src[k - k0] = srcs[k];
        cells += srcs[k].n_rows * fbk::kSlots;
      }
      hipLaunchKernelGGL(fbk::k_densify_rows, dim3(uint32_t((cells + 3) / 4)), dim3(256), 0, ctx->stream, da);
    }
    if (p.n_chunks)
      hipLaunchKernelGGL(fbk::k_msum_chunks, dim3(ns * 128u), dim3(256), 0, ctx->stream, arS, rs, ns, p.depth, p.n_chunks, p.chunks.as<uint8_t>());
    HIP_TRY(hipMemsetAsync(p.dshard.p, 0, uint64_t(ns) * 2 * width * 8, ctx->stream));
    const uint32_t tiles = ((n_a + 31) / 32) * ((n_b + 31) / 32);
    uint32_t spb = 16;  // slots per block: whole shards while the grid still holds ~2048 blocks, fewer slots (more atomics) below
    while (spb > 1 && uint64_t(ns) * (16 / spb) * tiles < 2048) spb >>= 1;
    const dim3 grid(uint32_t(uint64_t(ns) * (16 / spb) * tiles));
    const uint8_t* ch = p.chunks.as<uint8_t>();
    u64* out = p.dshard.as<u64>();
#define FBK_MSUM(CC)                                                                                                                           \
  do {                                                                                                                                         \
    if (arF)                                                                                                                                   \
      hipLaunchKernelGGL((fbk::k_msum_mfma<CC, true>), grid, dim3(256), 0, ctx->stream, arA, ra, n_a, arB, rb, n_b, arF, rf, arS, rs, c0, p.n_chunks, \
                         shift, cnt, ns, spb, out);                                                                                            \
    else                                                                                                                                       \
      hipLaunchKernelGGL((fbk::k_msum_mfma<CC, false>), grid, dim3(256), 0, ctx->stream, arA, ra, n_a, arB, rb, n_b, arF, rf, arS, rs, c0,        \
                         p.n_chunks, shift, cnt, ns, spb, out);                                                                                \
  } while (0)
    // chunks in launches of at most three (a depth-64 field: four launches over the same rows); the first one also counts
    for (uint32_t m0 = 0; m0 < std::max<uint32_t>(p.n_chunks, 1); m0 += fbk::kMsumPerLaunch) {
      const uint32_t cc = std::min(fbk::kMsumPerLaunch, p.n_chunks - std::min(m0, p.n_chunks));
      const uint8_t* c0 = ch ? ch + uint64_t(m0) * fbk::kMsumChunkBytes : nullptr;
      const uint32_t shift = fbk::kMsumChunkBits * m0, cnt = m0 == 0;
      if (cc == 0) FBK_MSUM(0);
      else if (cc == 1) FBK_MSUM(1);
      else if (cc == 2) FBK_MSUM(2);
      else FBK_MSUM(3);
    }
#undef FBK_MSUM
    hipLaunchKernelGGL(fbk::k_reduce_shards, dim3(uint32_t((2 * width + 255) / 256), std::min<uint32_t>(ns, 64)), dim3(256), 0, ctx->stream, p.dshard.as<u64>(), ns,
                       2 * width, p.result.as<u64>());
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// the result of the last run to the host
int32_t msum_read(fbk_ctx* ctx, MsumPlan& p, int64_t* out_sums, uint64_t* out_counts) {
  D2H back(ctx);
  if (out_sums) HIP_TRY(back.add(out_sums, p.result.p, p.width() * 8));
  if (out_counts) HIP_TRY(back.add(out_counts, p.result.as<u64>() + p.width(), p.width() * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_count_matrix_sum(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                             uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, const fbk_batch* bsi, const uint32_t* base_rows,
                             uint32_t bit_depth, uint32_t n_shards, int64_t* out_sums, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !out_sums || !out_counts) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = msum_args_ok(a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards)) return rc;
  const uint64_t width = uint64_t(n_a) * n_b;
  std::memset(out_sums, 0, width * 8);
  std::memset(out_counts, 0, width * 8);
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  MsumPlan p;
  if (int32_t rc = msum_prepare(ctx, p, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards)) return rc;
  if (int32_t rc = msum_enqueue(ctx, p)) return rc;
  return msum_read(ctx, p, out_sums, out_counts);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
