// fbk_matrix_sum_api.inc — fbk_count_matrix_sum: GroupBy with aggregate=Sum(field=v) in one pass over the operands per shard
// (fbk_matrix_sum.hip.h).  Included by fbk.hip before fbk_prepared_api.inc, whose fbk_query_count_matrix_sum keeps an MsumPlan.
//
// The matrix kernel reads dense rows (fbk_dense_operands.inc), a chunk of shards at a time.  The chunk bytes of the BSI values
// share the chunk's budget, kMsumScratch: per shard n_chunks MiB of chunk bytes + 128 KiB per densified row + 16 bytes per pair of
// per-shard sums and counts.  (fbk.h documents the arithmetic: the tests rely on it.)

namespace {

constexpr uint64_t kMsumScratch = 1ull << 30;

struct MsumPlan {
  GroupFieldOperands gf;  // its operands, with n_a, n_b, depth, n_shards and the chunk
  uint32_t n_chunks = 0;
  DevBuf chunks, dshard, result;
  uint64_t width() const { return uint64_t(gf.n_a) * gf.n_b; }
};

uint32_t msum_chunks_of(uint32_t depth) { return (depth + fbk::kMsumChunkBits - 1) / fbk::kMsumChunkBits; }

// The operand arguments of every GroupBy aggregate over an int field (g.a != nullptr is the caller's check).
int32_t msum_args_ok(const GroupFieldArgs& g) {
  if (!g.bsi || (g.n_shards && !g.base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (!g.b && g.n_b != 1) return fail(FBK_E_INVALID, "count_matrix_sum: without B rows (the one-field GroupBy) n_b must be 1");
  if (g.b) {
    if (int32_t rc = count_matrix_args_ok(g.a, g.rows_a, g.n_a, g.b, g.rows_b, g.n_b, g.filter, g.rows_f, g.n_shards)) return rc;
  } else if (int32_t rc = count_matrix_args_ok(g.a, g.rows_a, g.n_a, g.a, g.rows_a, 1, g.filter, g.rows_f, g.n_shards)) {
    return rc;
  }
  if (g.n_a > 4096 || g.n_b > 4096) return fail(FBK_E_INVALID, "count_matrix_sum: at most 4096 rows per side");
  if (g.bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (int32_t rc = check_rows(g.rows_a, uint64_t(g.n_shards) * g.n_a, g.a->n_rows, "count_matrix_sum A")) return rc;
  if (g.b)
    if (int32_t rc = check_rows(g.rows_b, uint64_t(g.n_shards) * g.n_b, g.b->n_rows, "count_matrix_sum B")) return rc;
  if (g.filter)
    if (int32_t rc = check_rows(g.rows_f, g.n_shards, g.filter->n_rows, "count_matrix_sum filter")) return rc;
  return bsi_rows_ok(g.base_rows, g.n_shards, g.bit_depth, g.bsi->n_rows);
}

// Validated arguments -> row lists on the device, scratch and result allocated: everything a run needs (n_shards > 0, width > 0).
int32_t msum_prepare(fbk_ctx* ctx, MsumPlan& p, const GroupFieldArgs& g) {
  p.n_chunks = msum_chunks_of(g.bit_depth);
  p.gf.add(g, g.bit_depth);
  const uint32_t c = even_chunk(g.n_shards, kMsumScratch, p.n_chunks * fbk::kMsumChunkBytes + kDenseRowBytes * p.gf.ops.densified_rows() + 16 * p.width());
  if (int32_t rc = p.gf.upload(ctx, c)) return rc;
  if (p.n_chunks) HIP_TRY(p.chunks.alloc(ctx, uint64_t(c) * p.n_chunks * fbk::kMsumChunkBytes));
  HIP_TRY(p.dshard.alloc(ctx, uint64_t(c) * 2 * p.width() * 8));
  HIP_TRY(p.result.alloc(ctx, 2 * p.width() * 8));
  return FBK_OK;
}

// One execution, launch-only: p.result = {sums [n_a * n_b] (u64, wrapping), counts [n_a * n_b]}.
int32_t msum_enqueue(fbk_ctx* ctx, MsumPlan& p) {
  GroupFieldOperands& gf = p.gf;
  if (gf.ops.layout_changed()) return fail(FBK_E_INVALID, "count_matrix_sum: a batch changed its layout since the query was prepared");
  const uint64_t width = p.width();
  const uint32_t n_a = gf.n_a, n_b = gf.n_b;
  HIP_TRY(hipMemsetAsync(p.result.p, 0, 2 * width * 8, ctx->stream));
  KernelSpan span(ctx);
  if (int32_t rc = gf.ops.for_each_chunk(ctx, true, DenseOperands::Densify::together, [&](uint32_t s0, uint32_t ns) -> int32_t {
    const auto [A, B, F, S] = gf.views(s0);
    if (p.n_chunks)
      hipLaunchKernelGGL(fbk::k_msum_chunks, dim3(ns * 128u), dim3(256), 0, ctx->stream, S.arena, S.rows, ns, gf.depth, p.n_chunks, p.chunks.as<uint8_t>());
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
    return FBK_OK;
  })) return rc;
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
  const GroupFieldArgs args{a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards};
  if (int32_t rc = msum_args_ok(args)) return rc;
  const uint64_t width = args.width();
  std::memset(out_sums, 0, width * 8);
  std::memset(out_counts, 0, width * 8);
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  MsumPlan p;
  if (int32_t rc = msum_prepare(ctx, p, args)) return rc;
  if (int32_t rc = msum_enqueue(ctx, p)) return rc;
  return msum_read(ctx, p, out_sums, out_counts);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
