// fbk_moments_api.inc — fbk_bsi_moments: n, Σx, Σy, Σx², Σy², Σxy of two int fields over exists_x ∩ exists_y ∩ filter
// (fbk_moments.hip.h), what SQL VAR and CORR are functions of.  Included by fbk.hip after fbk_matrix_sum_api.inc.
//
// The kernel reads dense rows (fbk_dense_operands.inc), a chunk of shards at a time; the rules — chunks per depth, rows of the
// Gram matrix, the densify chunk, the fold of the chunk-pair sums into 128-bit moments — are fbk_moments_plan.h's.  (fbk.h
// documents the chunk arithmetic: the tests rely on it.)

#include "fbk_moments_plan.h"

namespace {

int32_t moments_args_ok(const fbk_ctx* ctx, const fbk_batch* x, const uint32_t* base_rows_x, uint32_t depth_x, const fbk_batch* y,
                        const uint32_t* base_rows_y, uint32_t depth_y, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards,
                        const fbk_moments* out) {
  namespace mp = fbk_moments_plan;
  if (!ctx || !x || !base_rows_x || !out || (y && !base_rows_y) || (filter && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  if (!y && depth_y != 0) return fail(FBK_E_INVALID, "bsi_moments: without y (the one-field form) depth_y must be 0");
  if (depth_x > mp::kMaxDepth || depth_y > mp::kMaxDepth) return fail(FBK_E_INVALID, "bit depth > 64");
  if (n_shards > mp::kMaxShards) return fail(FBK_E_INVALID, "bsi_moments: at most 2^28 shards per call");
  if (int32_t rc = bsi_rows_ok(base_rows_x, n_shards, depth_x, x->n_rows)) return rc;
  if (y)
    if (int32_t rc = bsi_rows_ok(base_rows_y, n_shards, depth_y, y->n_rows)) return rc;
  if (filter)
    if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "bsi_moments filter")) return rc;
  return FBK_OK;
}

fbk_i128 moments_i128(unsigned __int128 v) { return {uint64_t(v), int64_t(uint64_t(v >> 64))}; }

}  // namespace

extern "C" {

int32_t fbk_bsi_moments(fbk_ctx* ctx, const fbk_batch* x, const uint32_t* base_rows_x, uint32_t depth_x, const fbk_batch* y,
                        const uint32_t* base_rows_y, uint32_t depth_y, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards,
                        fbk_moments* out) try {
  FBK_ENTER(ctx);
  namespace mp = fbk_moments_plan;
  if (int32_t rc = moments_args_ok(ctx, x, base_rows_x, depth_x, y, base_rows_y, depth_y, filter, rows_f, n_shards, out)) return rc;
  std::memset(out, 0, sizeof(*out));
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;

  DenseOperands ops;
  const int kX = ops.add(x, base_rows_x, depth_x + 2, true), kY = ops.add(y, base_rows_y, depth_y + 2, true), kF = ops.add(filter, rows_f, 1);
  // (the plan header restates DenseOperands' count so that the stand-alone check covers it: they must agree)
  const uint64_t densified = mp::densified_rows(!x->dense, depth_x, y != nullptr, y && !y->dense, depth_y, filter != nullptr, filter && !filter->dense);
  const uint32_t chunk = mp::densify_chunk(n_shards, densified);
  if (densified != ops.densified_rows()) return fail(FBK_E_HIP, "bsi_moments: fbk_moments_plan.h and fbk_dense_operands.inc disagree on the densified rows");
  if (int32_t rc = ops.upload(ctx, n_shards, chunk)) return rc;
  // one partial matrix per block, as many blocks per CU as are resident (kMomBlocksPerCU): the blocks walk their units of 16 stripes round robin.  pack: the column
  // blocks that share the tile (a stripe is pack * 1024 columns)
  const uint32_t pack = mp::packing(mp::rows(depth_x, y ? depth_y : 0).n);
  const uint64_t units_per_shard = fbk::kSlots * 8192 / (128 * pack) / fbk::kMomUnitStripes;
  const uint32_t max_blocks = uint32_t(std::min<uint64_t>(uint64_t(chunk) * units_per_shard, uint64_t(std::max(ctx->n_cu, 1)) * fbk::kMomBlocksPerCU));
  DevBuf partial, result;
  HIP_TRY(partial.alloc(ctx, uint64_t(max_blocks) * mp::kCells * 8));
  HIP_TRY(result.alloc(ctx, mp::kCells * 8));
  HIP_TRY(hipMemsetAsync(result.p, 0, mp::kCells * 8, ctx->stream));
  {
    KernelSpan span(ctx);
    ops.for_each_chunk(ctx, true, DenseOperands::Densify::together, [&](uint32_t s0, uint32_t ns) {
      const DenseView X = ops.view(kX, s0), Y = ops.view(kY, s0), F = ops.view(kF, s0);
      const fbk::MomentsArgs args{X.arena, X.rows, Y.arena, Y.rows, F.arena, F.rows, depth_x, depth_y, ns};
      const dim3 grid(uint32_t(std::min<uint64_t>(uint64_t(ns) * units_per_shard, max_blocks)));
      if (pack == 4) hipLaunchKernelGGL(fbk::k_bsi_moments<4>, grid, dim3(256), 0, ctx->stream, args, partial.as<long long>());
      else if (pack == 2) hipLaunchKernelGGL(fbk::k_bsi_moments<2>, grid, dim3(256), 0, ctx->stream, args, partial.as<long long>());
      else hipLaunchKernelGGL(fbk::k_bsi_moments<1>, grid, dim3(256), 0, ctx->stream, args, partial.as<long long>());
      hipLaunchKernelGGL(fbk::k_reduce_shards, dim3(mp::kCells / 256, std::min<uint32_t>(grid.x, 64)), dim3(256), 0, ctx->stream, partial.as<u64>(), grid.x,
                         uint64_t(mp::kCells), result.as<u64>());
    });
  }
  HIP_TRY(hipGetLastError());
  int64_t cells[mp::kCells];
  {
    D2H back(ctx);
    HIP_TRY(back.add(cells, result.p, sizeof(cells)));
    HIP_TRY(back.finish());  // the call's one synchronisation
  }
  const mp::Sums s = mp::fold(cells, depth_x, y ? depth_y : 0);
  out->n = s.n;
  out->sum_x = moments_i128(s.x), out->sum_xx = moments_i128(s.xx);
  if (y) out->sum_y = moments_i128(s.y), out->sum_yy = moments_i128(s.yy), out->sum_xy = moments_i128(s.xy);
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
