// fbk_bsi_api.inc — host side of the BSI calls (included by fbk.hip after fbk_fold_api.inc): Range (BsiRangePlan), Sum and the one-pass
// Sum(Range) (BsiSumPlan) — the two plans fbk_query_bsi_range and fbk_query_bsi_sum share with the one-shot calls — Min / Max and the
// between sum (one frame: bsi_sum_prepare's operands + download_words), Add, Distinct.

namespace {

using namespace fbk_bsi;  // BsiProg and the plane-program generators: fbk_bsi_prog.h

// Sum(Row(v op k), field = v) in one pass (k_bsi_range_sum_slot): the per-plane actions of rangeLT / rangeGT and their
// unsigned scans (fragment.go:1024-1208), with the SAME predicate rewrites as gen_lt / gen_gt / gen_ltu / gen_gtu above.
// false = one of the reference's special forms (predicate 0, saturated predicates, EQ / NEQ): the caller takes the
// two-pass path (range, then sum with the result as the filter).
bool plan_range_sum(int32_t op, uint64_t depth, int64_t pred, fbk::RangeSumPlan& pl) {
  bool gt, eq;
  switch (op) {
    case FBK_BSI_LT: gt = false, eq = false; break;
    case FBK_BSI_LTE: gt = false, eq = true; break;
    case FBK_BSI_GT: gt = true, eq = false; break;
    case FBK_BSI_GTE: gt = true, eq = true; break;
    default: return false;
  }
  if (gt && pred == -1 && !eq) pred = 0, eq = true;   // rangeGT :1116-1118
  if (!gt && pred == 1 && !eq) pred = 0, eq = true;   // rangeLT :1025-1027
  if (pred == 0 || depth == 0) return false;
  uint64_t up = abs_int64(pred);
  bool scan_gt;
  if (gt) {
    pl.scan_positive = pred >= 0;  // v > k >= 0: positives above k; v > k, k < 0: every positive + the negatives below |k|
    pl.take_other = pred < 0;
    scan_gt = pred >= 0;
  } else {
    pl.scan_positive = pred > 0;   // v < k, k > 0: every negative + the positives below k; k < 0: the negatives above |k|
    pl.take_other = pred > 0;
    scan_gt = pred < 0;
  }
  pl.depth = uint32_t(depth);
  std::memset(pl.action, 0, sizeof(pl.action));
  std::memset(pl.vhi, 0, sizeof(pl.vhi));
  auto above = [](uint64_t v, int i) { return v & ~((2ull << unsigned(i)) - 1); };  // the bits of v above bit i (i = 63: none)
  if (!scan_gt) {  // gen_ltu
    const uint64_t all_ones = go_shl(1, depth) - 1;
    if (bits_len64(up) > depth || up == all_ones) return false;
    if (eq) up++;
    const uint64_t p0 = up;
    for (int i = int(depth) - 1; i >= 0 && up > 0; --i) {
      if ((up >> unsigned(i)) & 1) {
        pl.action[i] = 4;  // matched |= remaining \ plane: these columns have 0 where the predicate has 1
        pl.vhi[i] = above(p0, i);
        up &= ~(1ull << unsigned(i));
      } else {
        pl.action[i] = 2;  // remaining \= plane
      }
    }
  } else {  // gen_gtu
    for (;;) {
      if (up == 0) return false;
      if (!eq && bits_len64(up) > depth) return false;
      if (eq) {
        up--;
        eq = false;
        continue;
      }
      break;
    }
    const uint64_t p0 = up;
    uint64_t px = up | go_shl(~0ull, depth);
    for (int i = int(depth) - 1; i >= 0 && px < ~0ull; --i) {
      if ((px >> unsigned(i)) & 1) {
        pl.action[i] = 1;  // remaining &= plane
      } else {
        pl.action[i] = 3;  // matched |= remaining & plane: 1 where the predicate has 0
        pl.vhi[i] = above(p0, i) | (1ull << unsigned(i));
        px |= 1ull << unsigned(i);
      }
    }
  }
  return true;
}

// Sum over lo <= v <= hi of the same field in one pass (k_bsi_between_sum_half): the schedule of the two scan lanes, from
// the definition of the comparison on sign-magnitude values (BetweenSumPlan).  false = two passes (lo >= hi, bounds
// beyond the field, the reference's EQ forms).
bool plan_between_sum(uint64_t depth, int64_t lo, int64_t hi, fbk::BetweenSumPlan& pl) {
  if (depth == 0 || depth > 64 || lo >= hi) return false;
  std::memset(&pl, 0, sizeof(pl));
  pl.depth = uint32_t(depth);
  const uint64_t all_ones = go_shl(1, depth) - 1;  // depth 64: ~0
  auto above = [](uint64_t v, int i) { return v & ~((2ull << unsigned(i)) - 1); };
  // "magnitude <= bound" from the top plane, on lane l
  auto le_scan = [&](int l, uint64_t bound, int from) {
    for (int i = from; i >= 0; --i) {
      if ((bound >> unsigned(i)) & 1) {
        pl.action[l][i] = 4;  // bit 0 where the bound has 1: below it whatever follows
        pl.vhi[l][i] = above(bound, i);
      } else {
        pl.action[l][i] = 2;  // bit 1 where the bound has 0: above it
      }
    }
    pl.vfin[l] = bound;
  };
  const uint64_t ulo = abs_int64(lo), uhi = abs_int64(hi);
  if (lo < 0 && hi >= 0) {  // the positives up to hi, the negatives up to |lo|
    pl.class_pos[0] = 1, pl.class_pos[1] = 0, pl.init_b = 1;
    if (uhi >= all_ones) pl.whole[0] = 1;
    else le_scan(0, uhi, int(depth) - 1);
    if (ulo >= all_ones) pl.whole[1] = 1;
    else le_scan(1, ulo, int(depth) - 1);
    return true;
  }
  uint64_t mn, mx;
  if (lo >= 0) pl.class_pos[0] = pl.class_pos[1] = 1, mn = ulo, mx = uhi;
  else pl.class_pos[0] = pl.class_pos[1] = 0, mn = uhi, mx = ulo;  // both negative: magnitudes |hi| .. |lo|
  if (mn > all_ones) return false;
  if (mx > all_ones) mx = all_ones;
  if (mn >= mx) return false;
  const int t = int(bits_len64(mn ^ mx)) - 1;  // the highest plane where the bounds differ: mn has 0, mx has 1
  for (int i = int(depth) - 1; i > t; --i) pl.action[0][i] = ((mn >> unsigned(i)) & 1) ? 1 : 2;  // the common prefix
  pl.split[t] = 1;
  for (int i = t - 1; i >= 0; --i) {  // lane 0: bit t = 0, ">= mn" on the planes below
    if ((mn >> unsigned(i)) & 1) {
      pl.action[0][i] = 1;
    } else {
      pl.action[0][i] = 3;
      pl.vhi[0][i] = above(mn, i) | (1ull << unsigned(i));
    }
  }
  pl.vfin[0] = mn;
  le_scan(1, mx, t - 1);  // lane 1: bit t = 1, "<= mx" on the planes below
  return true;
}

// What Row(v op predicate) keeps on the device (fragment.rangeOp, fragment.go:937-1303): the base row of every shard's fragment and
// the plane program.  fbk_bsi_range / fbk_bsi_range_between for their own duration, fbk_query_bsi_range between its runs.
struct BsiRangePlan {
  const fbk_batch* batch = nullptr;
  uint32_t depth = 0, n_shards = 0, prog_len = 0;
  DevBuf dbase, dprog;
};

// validates and uploads the base rows and the program (read by a queued copy: `prog` outlives the stream's next drain).
// `what` names the call in the message of a failed allocation.
int32_t bsi_range_prepare(fbk_ctx* ctx, BsiRangePlan& P, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                          const BsiProg& prog, const char* what) {
  P.batch = batch;
  P.depth = bit_depth;
  P.n_shards = n_shards;
  P.prog_len = uint32_t(prog.v.size());
  if (int32_t rc = upload_rows(ctx, base_rows, n_shards, batch->n_rows, P.dbase)) return rc;
  hipError_t e = P.dprog.alloc(ctx, std::max<size_t>(prog.v.size(), 1) * 4);
  if (e == hipSuccess && !prog.v.empty()) e = hipMemcpyAsync(P.dprog.p, prog.v.data(), prog.v.size() * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? FBK_E_NOMEM : FBK_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  return FBK_OK;
}

// launch only, one wavefront per (shard, slot): the result rows into the cells of `o`, their cardinalities added to
// d_counts[s].  encode: the kernel applies optimize() itself; d_runs (may be NULL): the run count of every cell.
void bsi_range_launch(fbk_ctx* ctx, BsiRangePlan& P, fbk_batch* o, uint32_t* d_runs, u64* d_counts, bool encode) {
  KernelSpan span(ctx);
  hipLaunchKernelGGL(fbk::k_bsi_range_slot, dim3(uint32_t(uint64_t(P.n_shards) * fbk::kSlots)), dim3(64), 0, ctx->stream, P.batch->d_slots, P.batch->d_arena,
                     P.dbase.as<uint32_t>(), P.n_shards, P.dprog.as<uint32_t>(), P.prog_len, uint32_t(P.depth + 2), o->d_arena, o->d_slots, d_runs, d_counts,
                     uint32_t(encode));
}

// a run of the prepared form: memset + the launch into the query's output batch (8 KiB cells, no run counts)
int32_t bsi_range_enqueue(fbk_ctx* ctx, BsiRangePlan& P, fbk_batch* o, u64* d_counts) {
  HIP_TRY(hipMemsetAsync(d_counts, 0, uint64_t(P.n_shards) * 8, ctx->stream));
  bsi_range_launch(ctx, P, o, nullptr, d_counts, false);
  HIP_TRY(hipGetLastError());
  slots_rewritten(o);
  return FBK_OK;
}

int32_t run_bsi_program(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint64_t n_shards,
                        uint64_t bit_depth, const BsiProg& prog, uint32_t flags, fbk_batch** out_batch,
                        uint64_t* out_counts) {
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  BsiRangePlan P;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_shards, n_shards, "bsi range")) return rc;
  if (int32_t rc = bsi_range_prepare(ctx, P, batch, base_rows, uint32_t(n_shards), uint32_t(bit_depth), prog, "bsi range")) return rc;
  if (n_shards) {
    bsi_range_launch(ctx, P, out.batch(), out.runs(), out.counts(), out.kernel_encodes(flags));
    if (int32_t rc = out.finish(n_shards, out_counts)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
}

// ---- the per-shard BSI aggregates (Sum, Min / Max, the range sums): one frame ------------------------------------------
// check the arguments, take the lock, upload the operands (bsi_sum_prepare), launch into W words per shard, download them
// (download_words), fold them on the host.

// pointers and depth; the outputs may be NULL only without shards (then the call returns FBK_OK right after this)
int32_t bsi_aggregate_args_ok(const fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                              const fbk_batch* filter, const uint32_t* rows_f, const void* out_a, const void* out_b) {
  if (!ctx || !batch || (n_shards && (!base_rows || !out_a || !out_b)) || (filter && n_shards && !rows_f))
    return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  return FBK_OK;
}

// the words a launch left in `d`, on the host once this returns (one synchronisation)
int32_t download_words(fbk_ctx* ctx, const void* d, uint64_t n_words, std::vector<u64>& h) {
  h.resize(n_words);
  D2H back(ctx);
  HIP_TRY(back.add(h.data(), d, n_words * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
}

// The two-pass form of a range sum, the reference's own two steps: the range as a Row (`rng`, owned from here on: freed on every
// path), then fragment.sum with that Row (∩ the caller's filter) as the filter.  Called WITHOUT the context's lock: the public
// entry points used here take it themselves.
int32_t bsi_sum_over_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth, fbk_batch* rng,
                           const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums, uint64_t* out_counts) {
  struct Owned {
    fbk_ctx* ctx;
    fbk_batch* b;
    ~Owned() { (void)fbk_batch_free(ctx, b); }
  } row{ctx, rng};
  std::vector<uint32_t> ident(n_shards);
  for (uint32_t s = 0; s < n_shards; ++s) ident[s] = s;
  if (filter) {
    fbk_batch* both = nullptr;
    const int32_t rc = fbk_setop(ctx, FBK_OP_AND, row.b, ident.data(), filter, rows_f, n_shards, 0, &both, nullptr);
    (void)fbk_batch_free(ctx, row.b);
    row.b = both;  // (NULL after a failure)
    if (rc) return rc;
  }
  return fbk_bsi_sum(ctx, batch, base_rows, n_shards, bit_depth, row.b, ident.data(), out_sums, out_counts);
}

// launch only: d3[s] = {psum, nsum, count} of shard s (zeroed here)
int32_t bsi_sum_launch(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* d_base, uint32_t n_shards, uint32_t bit_depth, const fbk_batch* filter,
                       const uint32_t* d_rf, u64* d3) {
  HIP_TRY(hipMemsetAsync(d3, 0, uint64_t(n_shards) * 24, ctx->stream));
  const FilterArgs f(filter, d_rf);
  {
    KernelSpan span(ctx);
    // one wavefront per (shard, slot)
    hipLaunchKernelGGL(fbk::k_bsi_sum_slot, dim3(uint32_t(uint64_t(n_shards) * fbk::kSlots)), dim3(64), 0, ctx->stream,
                       batch->d_slots, batch->d_arena, d_base, n_shards, bit_depth, f.slots, f.arena, d_rf, d3);
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// What fragment.sum keeps on the device — Sum over exists ∩ filter, or Sum(Row(v op predicate), field = v) in one pass (`ranged`):
// the base row and the filter's row of every shard (one allocation, one copy) and, ranged, the RangeSumPlan.  fbk_bsi_sum and
// fbk_bsi_range_sum for their own duration, fbk_query_bsi_sum between its runs.  A run leaves words() raw u64 per shard.
// (Min / Max and the between sum prepare one for its operands alone.)
struct BsiSumPlan {
  const fbk_batch *batch = nullptr, *filter = nullptr;
  uint32_t depth = 0, n_shards = 0;
  DevBuf rows;
  const uint32_t *d_base = nullptr, *d_rf = nullptr;  // (d_rf: NULL without a filter)
  bool ranged = false;
  fbk::RangeSumPlan range{};
  DevBuf drange;
  uint32_t words() const { return ranged ? 4 : 3; }
};

// validates and uploads the row lists (and the range plan: range != NULL)
int32_t bsi_sum_prepare(fbk_ctx* ctx, BsiSumPlan& P, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                        const fbk_batch* filter, const uint32_t* rows_f, const fbk::RangeSumPlan* range) {
  P.batch = batch;
  P.filter = filter;
  P.depth = bit_depth;
  P.n_shards = n_shards;
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  const uint32_t* dr[2] = {nullptr, nullptr};
  if (int32_t rc = upload_rows_multi(ctx, {{base_rows, n_shards, batch->n_rows}, {rows_f, filter ? uint64_t(n_shards) : 0, filter ? filter->n_rows : UINT32_MAX}}, P.rows, dr))
    return rc;
  P.d_base = dr[0];
  P.d_rf = filter ? dr[1] : nullptr;
  if (range) {
    P.ranged = true;
    P.range = *range;
    HIP_TRY(P.drange.alloc(ctx, sizeof(P.range)));
    HIP_TRY(hipMemcpyAsync(P.drange.p, &P.range, sizeof(P.range), hipMemcpyHostToDevice, ctx->stream));
  }
  return FBK_OK;
}

// launch only (memset + one kernel) into d_raw [n_shards * P.words()]
int32_t bsi_sum_enqueue(fbk_ctx* ctx, BsiSumPlan& P, u64* d_raw) {
  if (!P.ranged) return bsi_sum_launch(ctx, P.batch, P.d_base, P.n_shards, P.depth, P.filter, P.d_rf, d_raw);
  HIP_TRY(hipMemsetAsync(d_raw, 0, uint64_t(P.n_shards) * 32, ctx->stream));
  const FilterArgs f(P.filter, P.d_rf);
  const fbk::RangeSumPlan* d_plan = P.drange.as<fbk::RangeSumPlan>();
  {
    KernelSpan span(ctx);
    if (P.batch->dense) {  // half a container per wavefront, three planes in flight (four measured equal in round 3 and were dropped in round 5)
      auto kern = P.range.take_other ? fbk::k_bsi_range_sum_half<true, 3> : fbk::k_bsi_range_sum_half<false, 3>;
      hipLaunchKernelGGL(kern, dim3(uint32_t(uint64_t(P.n_shards) * fbk::kSlots * 2)), dim3(64), 0, ctx->stream, P.batch->d_arena, P.d_base, P.n_shards, d_plan,
                         f.slots, f.arena, P.d_rf, d_raw);
    } else {
      auto kern = P.range.take_other ? fbk::k_bsi_range_sum_slot<true> : fbk::k_bsi_range_sum_slot<false>;
      hipLaunchKernelGGL(kern, dim3(uint32_t(uint64_t(P.n_shards) * fbk::kSlots)), dim3(64), 0, ctx->stream, P.batch->d_slots, P.batch->d_arena, P.d_base,
                         P.n_shards, d_plan, f.slots, f.arena, P.d_rf, d_raw);
    }
  }
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// The host folds of the raw words; either output may be NULL.
// {psum, nsum, count} per shard: Total() = int64(psum) - int64(nsum) (roaring/filter.go:1106-1108)
void bsi_sum_fold(const u64* h3, uint32_t n_shards, int64_t* sums, uint64_t* counts) {
  for (uint32_t s = 0; s < n_shards; ++s) {
    if (sums) sums[s] = int64_t(h3[s * 3 + 0] - h3[s * 3 + 1]);
    if (counts) counts[s] = h3[s * 3 + 2];
  }
}
// {scanned class magnitudes, other class magnitudes, count scanned, count other} per shard: which of the classes is positive
// decides the signs (Total(), as above)
void bsi_range_sum_fold(const fbk::RangeSumPlan& pl, const u64* h4, uint32_t n_shards, int64_t* sums, uint64_t* counts) {
  for (uint32_t s = 0; s < n_shards; ++s) {
    const uint64_t sm = h4[s * 4 + 0], so = h4[s * 4 + 1];
    if (sums) sums[s] = int64_t(pl.scan_positive ? sm - so : so - sm);
    if (counts) counts[s] = h4[s * 4 + 2] + h4[s * 4 + 3];
  }
}

// the raw words of a run at d_raw -> per-shard (sum, count) on the host (one synchronisation)
int32_t bsi_sum_read(fbk_ctx* ctx, const BsiSumPlan& P, const void* d_raw, int64_t* sums, uint64_t* counts) {
  std::vector<u64> h;
  if (int32_t rc = download_words(ctx, d_raw, uint64_t(P.n_shards) * P.words(), h)) return rc;
  if (P.ranged) bsi_range_sum_fold(P.range, h.data(), P.n_shards, sums, counts);
  else bsi_sum_fold(h.data(), P.n_shards, sums, counts);
  return FBK_OK;
}

// the one-shot form of both: prepare, one run into a buffer of its own, read
int32_t bsi_sum_locked(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth, const fbk_batch* filter,
                       const uint32_t* rows_f, const fbk::RangeSumPlan* range, int64_t* out_sums, uint64_t* out_counts) {
  BsiSumPlan P;
  DevBuf draw;
  if (int32_t rc = bsi_sum_prepare(ctx, P, batch, base_rows, n_shards, bit_depth, filter, rows_f, range)) return rc;
  HIP_TRY(draw.alloc(ctx, uint64_t(n_shards) * P.words() * 8));
  if (int32_t rc = bsi_sum_enqueue(ctx, P, draw.as<u64>())) return rc;
  return bsi_sum_read(ctx, P, draw.p, out_sums, out_counts);
}

}  // namespace

extern "C" {

int32_t fbk_bsi_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums,
                    uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_sums, out_counts)) return rc;
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return bsi_sum_locked(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, nullptr, out_sums, out_counts);
} FBK_ABI_CATCH(ctx)

// The host fold of k_bsi_minmax_slot's records (also k_expr_agg_slot's): h2[(s * 16 + slot) * 2] = {magnitude, count | scan flag}
// -> Min (mode 0) / Max (mode 1) of shard s and the number of columns that hold it; (0, 0) where nothing qualifies.
static void bsi_minmax_fold(const u64* h2, uint32_t n_shards, uint32_t mode, int64_t* out_vals, uint64_t* out_counts) {
  for (uint32_t s = 0; s < n_shards; ++s) {
    // fragment.min (fragment.go:754-779): negatives present => -(maxUnsigned over them), else
    // minUnsigned over everything considered; fragment.max (:803-830) with positives.  "present" is
    // the OR over the slots; maxUnsigned / minUnsigned over the row = max / min of the slots' values.
    bool decided = false;  // some slot holds columns of the deciding sign
    for (int sl = 0; sl < fbk::kSlots; ++sl)
      if (h2[(uint64_t(s) * fbk::kSlots + sl) * 2 + 1] >> 63) decided = true;
    uint64_t mag = 0, cnt = 0;
    for (int sl = 0; sl < fbk::kSlots; ++sl) {
      const uint64_t v = h2[(uint64_t(s) * fbk::kSlots + sl) * 2];
      const uint64_t cw = h2[(uint64_t(s) * fbk::kSlots + sl) * 2 + 1];
      const uint64_t c = cw & ~(1ull << 63);
      if (c == 0 || bool(cw >> 63) != decided) continue;  // empty slot / a slot without columns of the deciding sign
      if (cnt == 0 || (decided ? v > mag : v < mag)) {
        mag = v;
        cnt = c;
      } else if (v == mag) {
        cnt += c;
      }
    }
    const bool negate = decided ? (mode == 0) : (mode == 1);
    const int64_t best = int64_t(negate ? (0ull - mag) : mag);
    out_vals[s] = cnt ? best : 0;
    out_counts[s] = cnt;
  }
}

// Min (mode 0) / Max (mode 1) per shard.  The caller holds ctx->mu, has set the device and checked the pointers; n_shards != 0.
// Also fbk_bsi_distinct_rows' window when arithmetic does not bound it.
static int32_t bsi_minmax_locked(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                                 uint32_t bit_depth, uint32_t mode, const fbk_batch* filter, const uint32_t* rows_f,
                                 int64_t* out_vals, uint64_t* out_counts) {
  BsiSumPlan ops;  // (for its operands: base rows and the filter's rows on the device)
  if (int32_t rc = bsi_sum_prepare(ctx, ops, batch, base_rows, n_shards, bit_depth, filter, rows_f, nullptr)) return rc;
  // one wavefront per (shard, slot), folded per shard on the host: min over a shard = the smallest of
  // its slots' minima, its count = the sum over the slots that reach it (max alike)
  const uint64_t n_out = uint64_t(n_shards) * fbk::kSlots;
  DevBuf d2;
  HIP_TRY(d2.alloc(ctx, n_out * 16));
  const FilterArgs f(filter, ops.d_rf);
  {
    KernelSpan span(ctx);
    hipLaunchKernelGGL(fbk::k_bsi_minmax_slot, dim3(uint32_t(n_out)), dim3(64), 0, ctx->stream, batch->d_slots, batch->d_arena,
                       ops.d_base, n_shards, bit_depth, mode, f.slots, f.arena, f.rows, d2.as<u64>());
  }
  HIP_TRY(hipGetLastError());
  std::vector<u64> h2;
  if (int32_t rc = download_words(ctx, d2.p, n_out * 2, h2)) return rc;
  bsi_minmax_fold(h2.data(), n_shards, mode, out_vals, out_counts);
  return FBK_OK;
}

static int32_t bsi_minmax(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                          uint32_t bit_depth, uint32_t mode, const fbk_batch* filter, const uint32_t* rows_f,
                          int64_t* out_vals, uint64_t* out_counts) {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_vals, out_counts)) return rc;
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return bsi_minmax_locked(ctx, batch, base_rows, n_shards, bit_depth, mode, filter, rows_f, out_vals, out_counts);
}

int32_t fbk_bsi_min(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_vals,
                    uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  return bsi_minmax(ctx, batch, base_rows, n_shards, bit_depth, 0, filter, rows_f, out_vals, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_max(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_vals,
                    uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  return bsi_minmax(ctx, batch, base_rows, n_shards, bit_depth, 1, filter, rows_f, out_vals, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_add(fbk_ctx* ctx, const fbk_batch* x, const uint32_t* rows_x, uint32_t depth_x, const fbk_batch* y,
                    const uint32_t* rows_y, uint32_t depth_y, uint64_t n_groups, uint32_t flags, fbk_batch** out_batch) try {
  FBK_ENTER(ctx);
  if (!ctx || !x || !y || !out_batch || (n_groups && ((depth_x && !rows_x) || (depth_y && !rows_y))))
    return fail(FBK_E_INVALID, "NULL argument");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  if (depth_x > 64 || depth_y > 64) return fail(FBK_E_INVALID, "bsi_add: at most 64 planes per operand");
  *out_batch = nullptr;
  const uint32_t D = std::max(depth_x, depth_y);
  if (n_groups * (D + 1) > (1ull << 27)) return fail(FBK_E_INVALID, "too many groups in one call");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  DevBuf drx, dry;
  CellOutput out;
  if (int32_t rc = out.alloc(ctx, n_groups * (D + 1), 0, "bsi_add")) return rc;
  if (int32_t rc = upload_rows(ctx, rows_x, n_groups * depth_x, x->n_rows, drx)) return rc;
  if (int32_t rc = upload_rows(ctx, rows_y, n_groups * depth_y, y->n_rows, dry)) return rc;
  if (n_groups) {
    hipLaunchKernelGGL(fbk::k_bsi_add, dim3(uint32_t(n_groups * fbk::kSlots)), dim3(256), 0, ctx->stream, x->d_slots, x->d_arena,
                       drx.as<uint32_t>(), depth_x, y->d_slots, y->d_arena, dry.as<uint32_t>(), depth_y, n_groups, out.batch()->d_arena,
                       out.batch()->d_slots, out.runs());
    if (int32_t rc = out.finish(flags, 0, nullptr)) return rc;
  }
  (void)hipStreamSynchronize(ctx->stream);
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

// blocks per (shard, slot) of k_bsi_values: enough of them for ~8 blocks per CU (each covers 16 / split rounds of 1024 columns per wave)
static uint32_t bsi_values_split(uint32_t n_shards) {
  uint32_t split = 1;
  while (split < 16 && uint64_t(n_shards) * fbk::kSlots * split < 2048) split <<= 1;
  return split;
}

// The device half of fbk_bsi_distinct: the sorted distinct values of exists ∩ filter over the shards, left on the device in `duniq`
// (n_unique of them).  Also the first stage of fbk_count_matrix_distinct.  The caller holds ctx->mu and has checked the pointers.
static int32_t bsi_distinct_device(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                                   const fbk_batch* filter, const uint32_t* rows_f, DevBuf& duniq, u64& n_unique) {
  n_unique = 0;
  fbk_batch* bb = const_cast<fbk_batch*>(batch);
  if (int32_t rc = refresh_slots(bb)) return rc;
  uint64_t upper = 0;  // at most one value per existing column
  if (int32_t rc = bsi_rows_ok(base_rows, n_shards, bit_depth, batch->n_rows)) return rc;
  for (uint32_t s = 0; s < n_shards; ++s)
    for (int sl = 0; sl < fbk::kSlots; ++sl) upper += fbk::slot_n(batch->h_slots[uint64_t(base_rows[s]) * fbk::kSlots + sl]);
  if (filter)
    if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "bsi_distinct filter")) return rc;
  if (upper == 0) return FBK_OK;
  if (upper >= (1ull << 31)) return fail(FBK_E_INVALID, "bsi_distinct: more than 2^31 values in one call (split the shard list)");
  DevBuf dvals, dsorted, dcur, dtmp, dbase, dcounts;
  HIP_TRY(dvals.alloc(ctx, upper * 8));
  HIP_TRY(dcur.alloc(ctx, 32));  // [0] the running total of values (k_bsi_cell_scan's carry), [1] the number of distinct values, [2] (uint32) the count-mismatch flag
  HIP_TRY(hipMemsetAsync(dcur.p, 0, 32, ctx->stream));
  HIP_TRY(dbase.alloc(ctx, (uint64_t(n_shards) * fbk::kSlots + 1) * 8));
  if (filter) HIP_TRY(dcounts.alloc(ctx, uint64_t(n_shards) * fbk::kSlots * 4));
  uint32_t* d_flag = reinterpret_cast<uint32_t*>(dcur.as<u64>() + 2);
  // Array / run containers among the planes or in the filter: both are densified, a chunk of shards at a time (<= ~4 GiB).
  const bool densify = !batch->dense || (filter && !filter->dense);
  const uint32_t rps = bit_depth + 2;  // rows per shard
  const uint32_t chunk = densify ? uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(n_shards, (4ull << 30) / ((rps + 1) * kDenseRowBytes)))) : n_shards;
  DenseOperands ops;
  const int kS = ops.add(batch, base_rows, rps, true, densify), kF = ops.add(filter, rows_f, 1, false, densify);
  if (int32_t rc = ops.upload(ctx, n_shards, chunk)) return rc;
  // Where a cell's values go is known before the transpose runs (k_bsi_cell_scan): without a filter the stored cardinalities of the
  // exists row are the counts, with one a count pass over exists ∩ filter comes first.
  ops.for_each_chunk(ctx, true, DenseOperands::Densify::together, [&](uint32_t s0, uint32_t ns) {
    const DenseView S = ops.view(kS, s0), F = ops.view(kF, s0);
    u64* cb = dbase.as<u64>() + uint64_t(s0) * fbk::kSlots;  // (the chunk's last entry is the next chunk's first: the same number)
    if (filter)
      hipLaunchKernelGGL(fbk::k_bsi_cell_counts, dim3((ns * fbk::kSlots + 3) / 4), dim3(256), 0, ctx->stream, S.arena, S.rows, ns, F.arena, F.rows,
                         dcounts.as<uint32_t>());
    hipLaunchKernelGGL(fbk::k_bsi_cell_scan, dim3(1), dim3(1024), 0, ctx->stream, batch->d_slots, ops.rows(kS, s0),
                       filter ? dcounts.as<uint32_t>() : (const uint32_t*)nullptr, ns * fbk::kSlots, cb, dcur.as<u64>());
    hipLaunchKernelGGL(fbk::k_bsi_values, dim3(ns * fbk::kSlots * bsi_values_split(ns)), dim3(256), 0, ctx->stream, S.arena, S.rows, ns, bit_depth, F.arena, F.rows,
                       dvals.as<long long>(), u64(upper), cb, d_flag, bsi_values_split(ns));
  });
  HIP_TRY(hipGetLastError());
  u64 h_cur[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h_cur, dcur.p, 24, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const u64 n_emit = h_cur[0];
  if (uint32_t(h_cur[2]) != 0)
    return fail(FBK_E_INVALID, "bsi_distinct: an exists row holds another number of columns than its stored cardinality says");
  if (n_emit == 0) return FBK_OK;
  if (n_emit > upper)
    return fail(FBK_E_INVALID, "bsi_distinct: the exists rows hold more columns than their stored cardinalities say (" +
                                   std::to_string(n_emit) + " > " + std::to_string(upper) + ")");
  // sort + unique (SignedRow.Union over shards is a set union of the values, executor.go:1196)
  HIP_TRY(dsorted.alloc(ctx, n_emit * 8));
  HIP_TRY(duniq.alloc(ctx, n_emit * 8));
  size_t t1 = 0, t2 = 0;
  u64* d_nu = dcur.as<u64>() + 1;
  HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, t1, dvals.as<long long>(), dsorted.as<long long>(), int(n_emit), 0, 64, ctx->stream));
  HIP_TRY(hipcub::DeviceSelect::Unique(nullptr, t2, dsorted.as<long long>(), duniq.as<long long>(), d_nu, int(n_emit), ctx->stream));
  HIP_TRY(dtmp.alloc(ctx, std::max<size_t>(std::max(t1, t2), 16)));
  size_t tb = std::max(t1, t2);
  HIP_TRY(hipcub::DeviceRadixSort::SortKeys(dtmp.p, tb, dvals.as<long long>(), dsorted.as<long long>(), int(n_emit), 0, 64, ctx->stream));
  tb = std::max(t1, t2);
  HIP_TRY(hipcub::DeviceSelect::Unique(dtmp.p, tb, dsorted.as<long long>(), duniq.as<long long>(), d_nu, int(n_emit), ctx->stream));
  HIP_TRY(hipMemcpyAsync(&n_unique, d_nu, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return FBK_OK;
}

int32_t fbk_bsi_distinct(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                         uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_values,
                         uint64_t cap, uint64_t* out_n) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_n || (n_shards && !base_rows) || (filter && n_shards && !rows_f) || (cap && !out_values))
    return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  *out_n = 0;
  if (n_shards == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  DevBuf duniq;
  u64 n_unique = 0;
  if (int32_t rc = bsi_distinct_device(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, duniq, n_unique)) return rc;
  *out_n = n_unique;
  if (n_unique == 0) return FBK_OK;
  if (n_unique > cap) return fail(FBK_E_CAPACITY, "bsi_distinct: " + std::to_string(n_unique) + " distinct values, buffer holds " + std::to_string(cap));
  HIP_TRY(hipMemcpyAsync(out_values, duniq.p, n_unique * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op,
                      uint32_t bit_depth, int64_t predicate, uint32_t flags, fbk_batch** out_batch,
                      uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_batch || (n_shards && !base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  *out_batch = nullptr;
  BsiProg prog;
  if (!gen_range_op(prog, op, bit_depth, predicate)) return fail(FBK_E_INVALID, "invalid range operation");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return run_bsi_program(ctx, batch, base_rows, n_shards, bit_depth, prog, flags, out_batch, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op,
                          uint32_t bit_depth, int64_t predicate, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums,
                          uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_sums, out_counts)) return rc;
  if (op < FBK_BSI_EQ || op > FBK_BSI_GTE) return fail(FBK_E_INVALID, "invalid range operation");
  if (n_shards == 0) return FBK_OK;
  fbk::RangeSumPlan pl;
  if (!plan_range_sum(op, bit_depth, predicate, pl)) {
    fbk_batch* rng = nullptr;
    if (int32_t rc = fbk_bsi_range(ctx, batch, base_rows, n_shards, op, bit_depth, predicate, 0, &rng, nullptr)) return rc;
    return bsi_sum_over_range(ctx, batch, base_rows, n_shards, bit_depth, rng, filter, rows_f, out_sums, out_counts);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return bsi_sum_locked(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, &pl, out_sums, out_counts);
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range_sum_plan(int32_t op, uint32_t bit_depth, int64_t predicate, uint8_t* out_actions, uint64_t* out_vhi,
                               uint32_t* out_scan_positive, uint32_t* out_take_other) try {
  if (!out_actions || !out_vhi || !out_scan_positive || !out_take_other) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (op < FBK_BSI_EQ || op > FBK_BSI_GTE) return fail(FBK_E_INVALID, "invalid range operation");
  fbk::RangeSumPlan pl;
  if (!plan_range_sum(op, bit_depth, predicate, pl)) return 1;  // the two-pass path
  std::memcpy(out_actions, pl.action, 64);
  std::memcpy(out_vhi, pl.vhi, 64 * 8);
  *out_scan_positive = pl.scan_positive;
  *out_take_other = pl.take_other;
  return FBK_OK;
} FBK_ABI_CATCH(nullptr)

int32_t fbk_bsi_between_sum_plan(uint32_t bit_depth, int64_t lo, int64_t hi, uint8_t* out_actions, uint64_t* out_vhi, uint8_t* out_split,
                                 uint64_t* out_vfin, uint32_t* out_flags) try {
  if (!out_actions || !out_vhi || !out_split || !out_vfin || !out_flags) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  fbk::BetweenSumPlan pl;
  if (!plan_between_sum(bit_depth, lo, hi, pl)) return 1;  // the two-pass path
  std::memcpy(out_actions, pl.action, 128);
  std::memcpy(out_vhi, pl.vhi, 128 * 8);
  std::memcpy(out_split, pl.split, 64);
  out_vfin[0] = pl.vfin[0], out_vfin[1] = pl.vfin[1];
  out_flags[0] = pl.class_pos[0], out_flags[1] = pl.class_pos[1], out_flags[2] = pl.init_b, out_flags[3] = pl.whole[0], out_flags[4] = pl.whole[1];
  return FBK_OK;
} FBK_ABI_CATCH(nullptr)

int32_t fbk_bsi_range_between_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                                  int64_t lo, int64_t hi, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (int32_t rc = bsi_aggregate_args_ok(ctx, batch, base_rows, n_shards, bit_depth, filter, rows_f, out_sums, out_counts)) return rc;
  if (n_shards == 0) return FBK_OK;
  fbk::BetweenSumPlan pl;
  // the one-pass kernel keeps four fragments per wavefront: dense batches only (half a container per wavefront)
  if (!batch->dense || !plan_between_sum(bit_depth, lo, hi, pl)) {
    fbk_batch* rng = nullptr;
    if (int32_t rc = fbk_bsi_range_between(ctx, batch, base_rows, n_shards, bit_depth, lo, hi, 0, &rng, nullptr)) return rc;
    return bsi_sum_over_range(ctx, batch, base_rows, n_shards, bit_depth, rng, filter, rows_f, out_sums, out_counts);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  BsiSumPlan ops;  // (for its operands: base rows and the filter's rows on the device)
  if (int32_t rc = bsi_sum_prepare(ctx, ops, batch, base_rows, n_shards, bit_depth, filter, rows_f, nullptr)) return rc;
  DevBuf d4, dplan;
  HIP_TRY(d4.alloc(ctx, uint64_t(n_shards) * 32));
  HIP_TRY(hipMemsetAsync(d4.p, 0, uint64_t(n_shards) * 32, ctx->stream));
  HIP_TRY(dplan.alloc(ctx, sizeof(pl)));
  HIP_TRY(hipMemcpyAsync(dplan.p, &pl, sizeof(pl), hipMemcpyHostToDevice, ctx->stream));
  const FilterArgs f(filter, ops.d_rf);
  {
    KernelSpan span(ctx);
    // half a container per wavefront, bsi_planes_ahead planes in flight (the quarter-container form of round 3 was removed
    // again: slower once the planes in flight were counted by hand, and two of its instantiations failed the in-flight check)
    auto kern = fbk::k_bsi_between_sum_part<8, 3>;
    hipLaunchKernelGGL(kern, dim3(uint32_t(uint64_t(n_shards) * fbk::kSlots * 2)), dim3(64), 0, ctx->stream, batch->d_arena, ops.d_base, n_shards,
                       dplan.as<fbk::BetweenSumPlan>(), f.slots, f.arena, f.rows, d4.as<u64>());
  }
  HIP_TRY(hipGetLastError());
  std::vector<u64> h4;
  if (int32_t rc = download_words(ctx, d4.p, uint64_t(n_shards) * 4, h4)) return rc;
  for (uint32_t s = 0; s < n_shards; ++s) {
    const uint64_t s0 = h4[s * 4 + 0], s1 = h4[s * 4 + 1];
    out_sums[s] = int64_t((pl.class_pos[0] ? s0 : 0ull - s0) + (pl.class_pos[1] ? s1 : 0ull - s1));
    out_counts[s] = h4[s * 4 + 2] + h4[s * 4 + 3];
  }
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_bsi_range_between(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                              uint32_t bit_depth, int64_t lo, int64_t hi, uint32_t flags, fbk_batch** out_batch,
                              uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !batch || !out_batch || (n_shards && !base_rows)) return fail(FBK_E_INVALID, "NULL argument");
  if (bit_depth > 64) return fail(FBK_E_INVALID, "bit depth > 64");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  *out_batch = nullptr;
  BsiProg prog;
  gen_between(prog, bit_depth, lo, hi);
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return run_bsi_program(ctx, batch, base_rows, n_shards, bit_depth, prog, flags, out_batch, out_counts);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
