// fbk_matrix_sum_api.inc — fbk_count_matrix_sum: GroupBy with aggregate=Sum(field=v) in one pass over the operands per shard
// (fbk_matrix_sum.hip.h).  Included by fbk.hip before fbk_prepared_api.inc, whose fbk_query_count_matrix_sum keeps an MsumPlan.
//
// The matrix kernel reads dense rows (fbk_dense_operands.inc), a chunk of shards at a time.  The chunk bytes of the BSI values
// share the chunk's budget, kMsumScratch: per shard n_chunks MiB of chunk bytes + 128 KiB per densified row + 16 bytes per pair of
// per-shard sums and counts.  (fbk.h documents the arithmetic: the tests rely on it.)

namespace {

constexpr uint64_t kMsumScratch = 1ull << 30;

struct MsumPlan {
  uint32_t n_a = 0, n_b = 0, n_shards = 0, depth = 0, n_chunks = 0, chunk = 0;
  DenseOperands ops;
  int A = 0, B = 0, F = 0, S = 0;  // its operands: A rows, B rows, the filter row, the BSI fragment
  DevBuf chunks, dshard, result;
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
  return bsi_rows_ok(base_rows, n_shards, bit_depth, bsi->n_rows);
}

// Validated arguments -> row lists on the device, scratch and result allocated: everything a run needs (n_shards > 0, width > 0).
int32_t msum_prepare(fbk_ctx* ctx, MsumPlan& p, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                     uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth,
                     uint32_t n_shards) {
  p.n_a = n_a, p.n_b = n_b, p.n_shards = n_shards, p.depth = bit_depth, p.n_chunks = msum_chunks_of(bit_depth);
  p.A = p.ops.add(a, rows_a, n_a), p.B = p.ops.add(b, rows_b, n_b), p.F = p.ops.add(filter, rows_f, 1);
  p.S = p.ops.add(bsi, base_rows, bit_depth + 2, true);
  p.chunk = even_chunk(n_shards, kMsumScratch, p.n_chunks * fbk::kMsumChunkBytes + kDenseRowBytes * p.ops.densified_rows() + 16 * p.width());
  const uint32_t c = p.chunk;
  if (int32_t rc = p.ops.upload(ctx, n_shards, c)) return rc;
  if (p.n_chunks) HIP_TRY(p.chunks.alloc(ctx, uint64_t(c) * p.n_chunks * fbk::kMsumChunkBytes));
  HIP_TRY(p.dshard.alloc(ctx, uint64_t(c) * 2 * p.width() * 8));
  HIP_TRY(p.result.alloc(ctx, 2 * p.width() * 8));
  return FBK_OK;
}

// One execution, launch-only: p.result = {sums [n_a * n_b] (u64, wrapping), counts [n_a * n_b]}.
int32_t msum_enqueue(fbk_ctx* ctx, MsumPlan& p) {
  if (p.ops.layout_changed()) return fail(FBK_E_INVALID, "count_matrix_sum: a batch changed its layout since the query was prepared");
  const uint64_t width = p.width();
  const uint32_t n_a = p.n_a, n_b = p.n_b;
  HIP_TRY(hipMemsetAsync(p.result.p, 0, 2 * width * 8, ctx->stream));
  KernelSpan span(ctx);
  for (uint32_t s0 = 0; s0 < p.n_shards; s0 += p.chunk) {
    const uint32_t ns = std::min(p.chunk, p.n_shards - s0);
    p.ops.densify(ctx, s0, ns);
    const DenseView A = p.ops.view(p.A, s0), B = p.ops.view(p.B, s0), F = p.ops.view(p.F, s0), S = p.ops.view(p.S, s0);
    if (p.n_chunks)
      hipLaunchKernelGGL(fbk::k_msum_chunks, dim3(ns * 128u), dim3(256), 0, ctx->stream, S.arena, S.rows, ns, p.depth, p.n_chunks, p.chunks.as<uint8_t>());
    HIP_TRY(hipMemsetAsync(p.dshard.p, 0, uint64_t(ns) * 2 * width * 8, ctx->stream));
    namespace mp = fbk_count_matrix_plan;  // slots per block: whole shards while the grid still holds ~2048 blocks
    const uint32_t tiles = mp::tiles32(n_a, n_b);
    const uint32_t spb = mp::slots_per_block(tiles, ns, mp::kSumFloor, mp::kSumEnough, 0);
    const dim3 grid(uint32_t(uint64_t(ns) * (16 / spb) * tiles));
    const uint8_t* ch = p.chunks.as<uint8_t>();
    u64* out = p.dshard.as<u64>();
#define FBK_MSUM(CC)                                                                                                                           \
  do {                                                                                                                                         \
    if (F.arena)                                                                                                                               \
      hipLaunchKernelGGL((fbk::k_msum_mfma<CC, true>), grid, dim3(256), 0, ctx->stream, A.arena, A.rows, n_a, B.arena, B.rows, n_b, F.arena, F.rows,  \
                         S.arena, S.rows, c0, p.n_chunks, shift, cnt, ns, spb, out);                                                           \
    else                                                                                                                                       \
      hipLaunchKernelGGL((fbk::k_msum_mfma<CC, false>), grid, dim3(256), 0, ctx->stream, A.arena, A.rows, n_a, B.arena, B.rows, n_b, F.arena, F.rows, \
                         S.arena, S.rows, c0, p.n_chunks, shift, cnt, ns, spb, out);                                                           \
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
