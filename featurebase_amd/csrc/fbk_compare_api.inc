// fbk_compare_api.inc — fbk_bsi_compare: the Row (or only the per-shard counts) of value_x op value_y over two int fields
// (fbk_compare.hip.h).  Included by fbk.hip after fbk_moments_api.inc.
//
// One launch of k_bsi_compare_slot, one wavefront per (shard, slot), on the operands' containers as they are encoded; the rules —
// the offset k = base_x - base_y, the instance, the plane steps, the final combination — are fbk_compare_plan.h's.  The output
// goes through CellOutput and finish_output exactly as run_bsi_program's does.

#include "fbk_compare_plan.h"

namespace {

int32_t compare_args_ok(const fbk_ctx* ctx, const fbk_batch* x, const uint32_t* base_rows_x, uint32_t depth_x, const fbk_batch* y,
                        const uint32_t* base_rows_y, uint32_t depth_y, int32_t op, const fbk_batch* filter, const uint32_t* rows_f,
                        uint32_t n_shards, uint32_t flags, fbk_batch** out_batch, const uint64_t* out_counts) {
  namespace cp = fbk_compare_plan;
  if (!ctx || !x || !y || (n_shards && (!base_rows_x || !base_rows_y)) || (filter && n_shards && !rows_f)) return fail(FBK_E_INVALID, "NULL argument");
  if (!out_batch && !out_counts) return fail(FBK_E_INVALID, "bsi_compare: out_batch and out_counts are both NULL");
  if (depth_x > cp::kMaxDepth || depth_y > cp::kMaxDepth) return fail(FBK_E_INVALID, "bit depth > 64");
  if (!cp::combine(op).ok) return fail(FBK_E_INVALID, "invalid range operation");
  if (flags & ~uint32_t(FBK_SETOP_OPTIMIZE | FBK_COMPARE_PATH_OFFSET)) return fail(FBK_E_INVALID, "unknown flags");
  if (n_shards >= cp::kMaxShards) return fail(FBK_E_INVALID, "bsi_compare: at most 2^27 - 1 shards per call");
  if (int32_t rc = bsi_rows_ok(base_rows_x, n_shards, depth_x, x->n_rows)) return rc;
  if (int32_t rc = bsi_rows_ok(base_rows_y, n_shards, depth_y, y->n_rows)) return rc;
  if (filter)
    if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "bsi_compare filter")) return rc;
  return FBK_OK;
}

template <int WRITE>
void launch_compare(bool general, uint32_t n_shards, hipStream_t st, const fbk::CompareArgs& a) {
  const dim3 grid(uint32_t(uint64_t(n_shards) * fbk::kSlots));
  if (general) hipLaunchKernelGGL((fbk::k_bsi_compare_slot<true, WRITE>), grid, dim3(64), 0, st, a);
  else hipLaunchKernelGGL((fbk::k_bsi_compare_slot<false, WRITE>), grid, dim3(64), 0, st, a);
}

}  // namespace

extern "C" {

int32_t fbk_bsi_compare(fbk_ctx* ctx, const fbk_batch* x, const uint32_t* base_rows_x, uint32_t depth_x, int64_t base_x, const fbk_batch* y,
                        const uint32_t* base_rows_y, uint32_t depth_y, int64_t base_y, int32_t op, const fbk_batch* filter, const uint32_t* rows_f,
                        uint32_t n_shards, uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  namespace cp = fbk_compare_plan;
  if (out_batch) *out_batch = nullptr;
  if (int32_t rc = compare_args_ok(ctx, x, base_rows_x, depth_x, y, base_rows_y, depth_y, op, filter, rows_f, n_shards, flags, out_batch, out_counts)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;

  const cp::Offset k = cp::offset(base_x, base_y);
  const cp::Combine cb = cp::combine(op);
  DevBuf drows, dcnt;
  CellOutput out;  // (unused by the count-only form: no arena, no descriptors)
  if (out_batch)
    if (int32_t rc = out.alloc(ctx, n_shards, n_shards, "bsi compare")) return rc;
  if (n_shards == 0) {
    if (out_batch) *out_batch = out.release();
    return FBK_OK;
  }
  const uint32_t* dr[3] = {nullptr, nullptr, nullptr};
  if (int32_t rc = upload_rows_multi(ctx, {{base_rows_x, n_shards, UINT32_MAX}, {base_rows_y, n_shards, UINT32_MAX}, {rows_f, filter ? uint64_t(n_shards) : 0, UINT32_MAX}},
                                     drows, dr))
    return rc;
  if (!out_batch) {
    HIP_TRY(dcnt.alloc(ctx, uint64_t(n_shards) * 8));
    HIP_TRY(hipMemsetAsync(dcnt.p, 0, uint64_t(n_shards) * 8, ctx->stream));
  }
  const bool enc = out_batch && out.kernel_encodes(flags & uint32_t(FBK_SETOP_OPTIMIZE));
  const FilterArgs f(filter, dr[2]);
  fbk::CompareArgs a{};
  a.xslots = x->d_slots, a.xarena = x->d_arena, a.xbase = dr[0];
  a.yslots = y->d_slots, a.yarena = y->d_arena, a.ybase = dr[1];
  a.fslots = f.slots, a.farena = f.arena, a.frows = f.rows;
  if (out_batch) a.arenaO = out.batch()->d_arena, a.outSlots = out.batch()->d_slots, a.outRuns = out.runs(), a.out_counts = out.counts();
  else a.out_counts = dcnt.as<u64>();
  a.k_low = cp::offset_low(k), a.k_neg = k < 0;
  a.n_shards = n_shards, a.depth_x = depth_x, a.depth_y = depth_y;
  a.steps = cp::steps(depth_x, depth_y, k, flags);
  a.take_lt = cb.take_lt, a.take_gt = cb.take_gt, a.invert = cb.invert;
  a.encode = enc;
  {
    KernelSpan span(ctx);
    if (out_batch) launch_compare<1>(cp::general(k, flags), n_shards, ctx->stream, a);
    else launch_compare<0>(cp::general(k, flags), n_shards, ctx->stream, a);
  }
  if (!out_batch) {
    HIP_TRY(hipGetLastError());
    D2H back(ctx);
    HIP_TRY(back.add(out_counts, dcnt.p, uint64_t(n_shards) * 8));
    HIP_TRY(back.finish());  // the call's one synchronisation
    return FBK_OK;
  }
  if (int32_t rc = out.finish(n_shards, out_counts)) return rc;  // (synchronises)
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
