// fbk_matrix_distinct_api.inc — fbk_count_matrix_distinct: GroupBy with aggregate=Count(Distinct(field=v)) for all (A row, B row)
// groups in one call (fbk_matrix_distinct.hip.h).  Included by fbk.hip after fbk_matrix_sum_api.inc, whose argument checks and
// count pass it reuses.
//
// Three stages on the context's stream:
//   1. the sorted distinct values U of exists ∩ F over all shards (bsi_distinct_device: fbk_bsi_distinct's kernels, unchanged);
//   2. per tile of the presence bitmap, k_mdist_scatter over the operands of every shard, then k_mdist_popcount;
//   3. (out_counts) fbk_count_matrix_sum's count pass: k_msum_mfma without value chunks, exists as the bit planes' row.
// Operands of batches that are not dense are densified a chunk of shards at a time (fbk_dense_operands.inc): in stage 1 by
// bsi_distinct_device (the BSI rows and the filter), in stage 2 again (every operand; stage 2 needs U first), in stage 3 by the
// count pass.  Stage 2's arithmetic (fbk.h documents it: the tests rely on it):
//   presence tile: wb = ceil(n_b / 64) words per (A row, rank), m64 = m rounded up to 64, row = 8 * wb * m64 bytes per A row;
//     n_a * row <= kMdistPresence: one tile;  else 64 * row <= kMdistPresence: ta = floor(kMdistPresence / row) rounded down
//     to a multiple of 64 A rows, all ranks;  else ta = min(n_a, 64) A rows, tr = floor(kMdistPresence / (8 * wb * ta))
//     rounded down to a multiple of 64 ranks.
//   densify chunk: 128 KiB per densified row of a shard, at most kMdistScratch.  With more than one chunk, every tile densifies
//     every chunk again.

namespace {

constexpr uint64_t kMdistPresence = 128ull << 20;
constexpr uint64_t kMdistScratch = 1ull << 30;

struct MdistTiles {
  uint32_t ta = 0;  // A rows per tile
  uint64_t tr = 0;  // ranks per tile (a multiple of 64)
};

MdistTiles mdist_tiles(uint32_t n_a, uint32_t n_b, uint64_t m) {
  const uint64_t wb = (uint64_t(n_b) + 63) / 64, m64 = (m + 63) / 64 * 64, row = 8 * wb * m64;
  MdistTiles t;
  if (uint64_t(n_a) * row <= kMdistPresence) {
    t.ta = n_a, t.tr = m64;
  } else if (64 * row <= kMdistPresence) {
    t.ta = uint32_t(kMdistPresence / row / 64 * 64), t.tr = m64;
  } else {
    t.ta = std::min<uint32_t>(n_a, 64), t.tr = kMdistPresence / (8 * wb * t.ta) / 64 * 64;
  }
  return t;
}

}  // namespace

extern "C" {

int32_t fbk_count_matrix_distinct(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                  const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                  const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                                  uint64_t* out_distinct, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !out_distinct) return fail(FBK_E_INVALID, "NULL argument");
  const GroupFieldArgs args{a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards};
  if (int32_t rc = msum_args_ok(args)) return rc;
  const uint64_t width = args.width();
  std::memset(out_distinct, 0, width * 8);
  if (out_counts) std::memset(out_counts, 0, width * 8);
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  // stage 1: U
  DevBuf duniq;
  u64 m = 0;
  if (int32_t rc = bsi_distinct_device(ctx, bsi, base_rows, n_shards, bit_depth, filter, rows_f, duniq, m)) return rc;
  if (m > 0) {
    // stage 2: operands (densified a chunk of shards at a time), presence tiles
    GroupFieldOperands gf;
    gf.add(args, bit_depth);
    if (int32_t rc = gf.upload(ctx, even_chunk(n_shards, kMdistScratch, kDenseRowBytes * gf.ops.densified_rows()))) return rc;
    DevBuf pres, result;
    const MdistTiles t = mdist_tiles(n_a, n_b, m);
    const uint32_t wb = (n_b + 63) / 64, tr = uint32_t(t.tr);
    const uint64_t m64 = (m + 63) / 64 * 64;
    HIP_TRY(pres.alloc(ctx, uint64_t(t.ta) * wb * tr * 8));
    HIP_TRY(result.alloc(ctx, width * 8));
    HIP_TRY(hipMemsetAsync(result.p, 0, width * 8, ctx->stream));
    for (uint32_t a0 = 0; a0 < n_a; a0 += t.ta) {
      const uint32_t na = std::min(t.ta, n_a - a0);
      for (uint64_t r0 = 0; r0 < m64; r0 += tr) {
        HIP_TRY(hipMemsetAsync(pres.p, 0, uint64_t(na) * wb * tr * 8, ctx->stream));
        gf.for_each_chunk(ctx, a0 == 0 && r0 == 0, [&](const GroupFieldViews& v, uint32_t, uint32_t ns) {
          gf.launch(fbk::k_mdist_scatter, gf.walk_grid(ns), 0, ctx, v, ns, a0, na, duniq.as<long long>(), uint32_t(m), uint32_t(r0), tr, pres.as<u64>());
        });
        // popcount: enough parts of the rank range for ~8192 wavefronts
        const uint64_t pairs = uint64_t(na) * wb;
        const uint32_t splits = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(tr / 64, 8192 / pairs)));
        hipLaunchKernelGGL(fbk::k_mdist_popcount, dim3(uint32_t((pairs * splits + 3) / 4)), dim3(256), 0, ctx->stream, pres.as<u64>(), na, n_b,
                           tr, a0, splits, result.as<u64>());
      }
    }
    HIP_TRY(hipGetLastError());
    D2H back(ctx);
    HIP_TRY(back.add(out_distinct, result.p, width * 8));
    HIP_TRY(back.finish());
  }
  if (out_counts) {
    // stage 3: the columns of every group, fbk_count_matrix_sum's pass at depth 0
    MsumPlan p;
    GroupFieldArgs counts_args = args;
    counts_args.bit_depth = 0;
    if (int32_t rc = msum_prepare(ctx, p, counts_args)) return rc;
    if (int32_t rc = msum_enqueue(ctx, p)) return rc;
    if (int32_t rc = msum_read(ctx, p, nullptr, out_counts)) return rc;
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
