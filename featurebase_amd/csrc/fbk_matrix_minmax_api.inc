// fbk_matrix_minmax_api.inc — fbk_count_matrix_minmax: GroupBy with Min / Max of an int field for all (A row, B row) groups in one
// call (fbk_matrix_minmax.hip.h).  Included by fbk.hip after fbk_matrix_distinct_api.inc; the argument checks are
// fbk_count_matrix_sum's (msum_args_ok).
//
// Both kernel paths read dense rows, a chunk of shards at a time, through GroupFieldOperands (fbk_group_field.inc), by the chunk
// arithmetic of fbk_count_matrix_distinct's stage 2; which path runs, the descent's grid and the chunk are fbk_minmax_plan.h's rules.  (fbk.h
// documents the arithmetic: the tests rely on it.)  The scatter path with counts walks the operands twice (k_minmax_holders needs the
// final magnitudes); with more than one chunk it densifies every chunk again for the second walk.

#include "fbk_minmax_plan.h"

extern "C" {

int32_t fbk_count_matrix_minmax(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards, uint32_t flags,
                                int64_t* out_min, int64_t* out_max, uint64_t* out_min_counts, uint64_t* out_max_counts) try {
  FBK_ENTER(ctx);
  namespace mp = fbk_minmax_plan;
  if (!ctx || !a || !out_min || !out_max) return fail(FBK_E_INVALID, "NULL argument");
  if (!out_min_counts != !out_max_counts) return fail(FBK_E_INVALID, "count_matrix_minmax: pass both count outputs or neither");
  if (flags > FBK_MINMAX_SCATTER) return fail(FBK_E_INVALID, "count_matrix_minmax: unknown flags");
  const GroupFieldArgs args{a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, bsi, base_rows, bit_depth, n_shards};
  if (int32_t rc = msum_args_ok(args)) return rc;
  const uint32_t path = mp::path(n_a, n_b, flags);
  if (!path) return fail(FBK_E_INVALID, "count_matrix_minmax: FBK_MINMAX_DESCENT takes at most 1024 groups (n_a * n_b)");
  const uint64_t width = args.width();
  const bool want_counts = out_min_counts != nullptr;
  std::fill(out_min, out_min + width, INT64_MAX);
  std::fill(out_max, out_max + width, INT64_MIN);
  if (want_counts) std::memset(out_min_counts, 0, width * 8), std::memset(out_max_counts, 0, width * 8);
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;

  GroupFieldOperands gf;
  gf.add(args, bit_depth);
  const uint32_t chunk = mp::densify_chunk(n_shards, gf.ops.densified_rows());
  if (int32_t rc = gf.upload(ctx, chunk)) return rc;
  DevBuf result, state, partial;  // result: min [width], max [width], min counts [width], max counts [width]
  HIP_TRY(result.alloc(ctx, width * 8 * 4));
  long long *d_min = result.as<long long>(), *d_max = d_min + width;
  u64 *d_cmin = want_counts ? result.as<u64>() + 2 * width : nullptr, *d_cmax = want_counts ? d_cmin + width : nullptr;
  if (path == mp::kDescent) {
    const uint32_t tiles = mp::tiles_of(width), cells_p = tiles * 64, max_grid = mp::descent_grid(chunk, width);
    HIP_TRY(partial.alloc(ctx, uint64_t(max_grid) * cells_p * sizeof(fbk::MinmaxPartial)));
    HIP_TRY(state.alloc(ctx, width * sizeof(fbk::MinmaxPartial)));
    KernelSpan span(ctx);
    gf.for_each_chunk(ctx, true, [&](const GroupFieldViews& v, uint32_t s0, uint32_t ns) {
      const uint32_t grid = mp::descent_grid(ns, width);
      gf.launch(fbk::k_minmax_descent, dim3(grid, tiles), 0, ctx, v, ns, partial.as<fbk::MinmaxPartial>());
      hipLaunchKernelGGL(fbk::k_minmax_fold, dim3(uint32_t((width + 3) / 4)), dim3(256), 0, ctx->stream, partial.as<fbk::MinmaxPartial>(), grid, cells_p,
                         uint32_t(width), state.as<fbk::MinmaxPartial>(), int(s0 == 0), int(s0 + ns == n_shards), d_min, d_max, d_cmin, d_cmax);
    });
  } else {
    HIP_TRY(state.alloc(ctx, width * 48));  // [width][4] magnitudes, then [width][2] counts
    u64 *d_state = state.as<u64>(), *d_counts = d_state + width * 4;
    hipLaunchKernelGGL(fbk::k_minmax_init, dim3(uint32_t((width + 255) / 256)), dim3(256), 0, ctx->stream, d_state, d_counts, width);
    KernelSpan span(ctx);
    for (int pass = 0; pass < (want_counts ? 2 : 1); ++pass)
      gf.for_each_chunk(ctx, pass == 0, [&](const GroupFieldViews& v, uint32_t, uint32_t ns) {
        if (pass == 0) gf.launch(fbk::k_minmax_scatter, gf.walk_grid(ns), 0, ctx, v, ns, d_state);
        else gf.launch(fbk::k_minmax_holders, gf.walk_grid(ns), 0, ctx, v, ns, d_state, d_counts);
      });
    hipLaunchKernelGGL(fbk::k_minmax_finish, dim3(uint32_t((width + 255) / 256)), dim3(256), 0, ctx->stream, d_state, d_counts, width, d_min, d_max, d_cmin,
                       d_cmax);
  }
  HIP_TRY(hipGetLastError());
  D2H back(ctx);
  HIP_TRY(back.add(out_min, d_min, width * 8));
  HIP_TRY(back.add(out_max, d_max, width * 8));
  if (want_counts) {
    HIP_TRY(back.add(out_min_counts, d_cmin, width * 8));
    HIP_TRY(back.add(out_max_counts, d_cmax, width * 8));
  }
  HIP_TRY(back.finish());  // the call's one synchronisation
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
