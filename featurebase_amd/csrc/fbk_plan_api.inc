// fbk_plan_api.inc — pair plans (fbk_plan_*) and the two one-shot calls built on them, fbk_intersection_count and fbk_setop.
// Included by fbk.hip after fbk_output.inc and before fbk_dense_operands.inc.
//
// A plan is a prepared list of row pairs (A.rows_a[i], B.rows_b[i]) whose index arrays and output buffers live on the device,
// so that the hot path is launch-only: no host allocation, no H2D copy, no synchronisation between steps.  It is the unit one
// (query, node) batch call from mapperLocal (executor.go:6742) becomes.  The plan OWNS its device buffers (DevBuf) and its
// output batch: deleting it returns them to the pool.  The caller of `delete` has drained the stream (fbk_plan_free, the
// one-shot calls).

struct fbk_plan {
  fbk_ctx* ctx = nullptr;
  const fbk_batch* a = nullptr;
  const fbk_batch* b = nullptr;
  uint64_t n_pairs = 0;
  DevBuf d_rows_a, d_rows_b;  // uint32_t[n_pairs] each
  DevBuf d_own_counts;        // u64[n_pairs], unless the caller gave its own buffer
  u64* d_counts = nullptr;    // n_pairs: d_own_counts' block or the caller's buffer (which outlives the plan)
  DevBuf d_total;             // u64
  DevBuf d_done;              // uint32_t: ticket counter of the fused count + total kernel (zeroed at creation, kept at 0 between launches)
  std::unique_ptr<fbk_batch, decltype(&free_batch_storage)> out{nullptr, free_batch_storage};  // lazily created by the first set-op enqueue
  DevBuf d_runs;              // uint32_t per output slot: run count (optimize pass)
  std::vector<uint32_t> h_rows_a, h_rows_b;
  // k_icount2: the (pair, slot) item records resolved once per plan (re-resolved when a batch's descriptors were
  // rewritten since) and one count per wave, summed per pair by k_sum_wave_counts
  DevBuf d_items, d_wave_counts;  // Slot[2 * 16 * n_pairs], uint32_t[16 * n_pairs]: both or neither (plan_resolve_items)
  uint64_t items_va = ~0ull, items_vb = ~0ull;
  bool last_rev = false;  // direction of the plan's last dense count (k_icount_dense_resident's `rev`; the cold kernel counts as forward)
  ~fbk_plan() {
    const fbk_plan* self = this;
    if (ctx) ctx->hot_plan.compare_exchange_strong(self, nullptr);  // (a later plan may get this address)
  }
};

namespace {

// Average encoded payload per container of a batch, in bytes.
uint64_t batch_avg_payload(const fbk_batch* b) {
  const uint64_t slots = uint64_t(b->n_rows) * fbk::kSlots;
  return slots ? b->arena_bytes / slots : 0;
}
// Which generation of the pair kernels a launch uses (option pair_kernels pins it: 1 / 2; 0 decides by the rows).
// Rows of tiny containers on BOTH sides (arrays of a few values, a handful of runs) are served better by the round-2
// kernels: there the launch of a block per item is what a kernel costs, not decode work or latency (BenchmarkCtOps
// matrix, profiles/ctops_r03.txt: Ary16 x Ary16 10.5 us with k_icount, 18 us with k_icount2).
bool use_pair_kernels2(const fbk_ctx* ctx, const fbk_batch* a, const fbk_batch* b, int op /* -1: count */) {
  if (ctx->opt.pair_kernels) return ctx->opt.pair_kernels >= 2;
  const uint64_t lo = std::min(batch_avg_payload(a), batch_avg_payload(b)), both = (a->arena_bytes + b->arena_bytes);
  const uint64_t slots = (uint64_t(a->n_rows) + b->n_rows) * fbk::kSlots;
  if (op >= 0) {
    // materialising operations (8 KiB written per pair whatever the operands): k_setop2 wins where at least one side
    // holds KiB-sized SPARSE containers — arrays from ~1000 values, long run lists — whose decode and load latency it
    // was built around (Ary4096 x Ary1 XOR 73 -> 53 us; config 3's rows 89 -> 69 us); with small arrays on one side and
    // small arrays or bitmaps on the other the round-2 kernel's cheaper per-item path is 10-25 % ahead
    // (BenchmarkCtOps matrix, profiles/ctops_r03.txt)
    const uint64_t big_sparse = std::max(a->dense ? 0 : batch_avg_payload(a), b->dense ? 0 : batch_avg_payload(b));
    return big_sparse >= 1536;
  }
  if (!slots || both < 256 * slots) return false;
  // one side tiny: when the other one is all bitmaps (or there is nothing on one side at all) the items are probes of a
  // few dwords in global memory in either generation, and the round-2 kernel's four-wave blocks launch faster
  // (Ary1 x BM512 7.4 us vs 9.3); against big arrays / run lists the table + probe form wins (Ary4096 x Ary1 48 -> 27 us)
  if (lo < 256 && (a->arena_bytes == 0 || b->arena_bytes == 0 || (batch_avg_payload(a) < 256 ? b->dense : a->dense))) return false;
  return true;
}
// Waves per block of the round-3 pair kernels (option pair_wpb pins it).  One-wave blocks release a wave's LDS table the
// moment IT ends, which is what heterogeneous items (runs next to arrays) need; when one side's containers are tiny the
// items are all alike and short, and four waves per block quarter the number of blocks to launch.
int pair_wpb_for(const fbk_ctx* ctx, const fbk_batch* a, const fbk_batch* b) {
  if (ctx->opt.pair_wpb) return ctx->opt.pair_wpb >= 4 ? 4 : 1;  // (normalised once: 1 or 4.  Two-wave blocks were built and measured in round 4: count 182 against 166-173 us, set-ops equal — profiles/r04_pairs_wpb_ab.json — and removed)
  return std::min(batch_avg_payload(a), batch_avg_payload(b)) < 256 ? 4 : 1;
}

// The plan's item records: {A's descriptor, B's descriptor} per (pair, slot), resolved on the device once per version of the
// two batches (k_resolve_items) — the pair kernels then start with ONE scalar round trip instead of row index -> descriptor.
// Allocated with the per-wave count vector of the count kernel: both buffers or neither (a plan that got only the first, out
// of memory on the second, must not take the resolved path next time).
int32_t plan_resolve_items(fbk_ctx* ctx, fbk_plan* p) {
  const uint64_t n_items = p->n_pairs * fbk::kSlots;
  if (!p->d_items.p || !p->d_wave_counts.p) {
    HIP_TRY(p->d_items.ensure(ctx, std::max<uint64_t>(n_items, 1) * 2 * sizeof(Slot)));
    if (hipError_t e = p->d_wave_counts.ensure(ctx, std::max<uint64_t>(n_items, 1) * sizeof(uint32_t)); e != hipSuccess) {
      p->d_items.reset();
      HIP_TRY(e);
    }
    p->items_va = p->items_vb = ~0ull;
  }
  if (n_items && (p->items_va != p->a->version || p->items_vb != p->b->version)) {
    hipLaunchKernelGGL(fbk::k_resolve_items, dim3(uint32_t((n_items + 255) / 256)), dim3(256), 0, ctx->stream, p->a->d_slots, p->d_rows_a.as<uint32_t>(),
                       p->b->d_slots, p->d_rows_b.as<uint32_t>(), p->n_pairs, p->d_items.as<Slot>());
    HIP_TRY(hipGetLastError());
    p->items_va = p->a->version;
    p->items_vb = p->b->version;
  }
  return FBK_OK;
}

template <int OP>
void launch_setop(bool dense, fbk_plan* p, hipStream_t st, bool want_runs, const Slot* items) {
  const uint32_t blocks = uint32_t(p->n_pairs * fbk::kSlots / 4);
  const uint32_t *rows_a = p->d_rows_a.as<uint32_t>(), *rows_b = p->d_rows_b.as<uint32_t>();
  uint32_t* runs = want_runs ? p->d_runs.as<uint32_t>() : nullptr;
  // (the in-kernel optimize() — mode 2 — only when the caller asked for optimize(): plain set-ops keep their bitmap cells)
  const uint32_t direct = want_runs ? uint32_t(p->ctx->opt.setop_direct_encode) : 0u;
#ifdef FBK_EXPERIMENTS  // (option pair_ablate, timing experiments on k_setop2: item classes skipped, emission without its stores — WRONG results)
  const uint32_t direct2 = direct | 0x100u | (uint32_t(p->ctx->opt.pair_ablate) << 16);
#else
  const uint32_t direct2 = direct | 0x100u;  // k_setop2 only: Intersect / Difference whose result is a subset of an array operand by table + probe (an A/B option until round 5)
#endif
  if (dense)
    hipLaunchKernelGGL(fbk::k_setop_dense<OP>, dim3(blocks), dim3(256), 0, st, p->a->d_arena, rows_a, p->b->d_arena, rows_b, p->out->d_arena, p->out->d_slots);
  else if (use_pair_kernels2(p->ctx, p->a, p->b, OP == 0 ? FBK_OP_AND : OP == 1 ? FBK_OP_OR : OP == 2 ? FBK_OP_XOR : FBK_OP_ANDNOT) && pair_wpb_for(p->ctx, p->a, p->b) == 4)
    hipLaunchKernelGGL((fbk::k_setop2<OP, 4>), dim3(blocks), dim3(256), 0, st, p->a->d_slots, p->a->d_arena, rows_a, p->b->d_slots, p->b->d_arena, rows_b,
                       p->n_pairs, p->out->d_arena, p->out->d_slots, runs, direct2, (const Slot*)nullptr);
  else if (use_pair_kernels2(p->ctx, p->a, p->b, OP == 0 ? FBK_OP_AND : OP == 1 ? FBK_OP_OR : OP == 2 ? FBK_OP_XOR : FBK_OP_ANDNOT))
  {
    // Intersect / Difference with optimize(): most results come from the probe paths — the register-lean instance (18 instead of 16 waves per CU;
    // setop_direct_encode = 0 / 1 run the common instance + the separate re-encode pass: the byte-for-byte cross-check).  Union / Xor with
    // optimize() send every item down the general path: there the lean instance loses 3 % (509 -> 524 us, profiles/r06_setop2_occupancy.txt)
    constexpr bool kHasProbe = OP == 0 || OP == 3;
    if (kHasProbe && direct == 2u)
      hipLaunchKernelGGL((fbk::k_setop2<OP, 1, kHasProbe>), dim3(uint32_t(p->n_pairs * fbk::kSlots)), dim3(64), 0, st, p->a->d_slots, p->a->d_arena, rows_a,
                         p->b->d_slots, p->b->d_arena, rows_b, p->n_pairs, p->out->d_arena, p->out->d_slots, runs, direct2, items);
    else
      hipLaunchKernelGGL((fbk::k_setop2<OP, 1>), dim3(uint32_t(p->n_pairs * fbk::kSlots)), dim3(64), 0, st, p->a->d_slots, p->a->d_arena, rows_a,
                         p->b->d_slots, p->b->d_arena, rows_b, p->n_pairs, p->out->d_arena, p->out->d_slots, runs, direct2, items);
  }
  else
    hipLaunchKernelGGL(fbk::k_setop<OP>, dim3(blocks), dim3(256), 0, st, p->a->d_slots, p->a->d_arena, rows_a, p->b->d_slots, p->b->d_arena, rows_b,
                       p->n_pairs, p->out->d_arena, p->out->d_slots, runs, direct);
}

int32_t plan_create_locked(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, const fbk_batch* b,
                           const uint32_t* rows_b, uint64_t n_pairs, void* ext_counts, std::unique_ptr<fbk_plan>& out_plan) {
  if (n_pairs > (1ull << 27)) return fail(FBK_E_INVALID, "too many pairs in one plan");
  for (uint64_t i = 0; i < n_pairs; ++i)
    if (rows_a[i] >= a->n_rows || rows_b[i] >= b->n_rows) return fail(FBK_E_INVALID, "row index out of range");
  std::unique_ptr<fbk_plan> p(new (std::nothrow) fbk_plan());
  if (!p) return fail(FBK_E_NOMEM, "host allocation failed");
  p->ctx = ctx;
  p->a = a;
  p->b = b;
  p->n_pairs = n_pairs;
  p->h_rows_a.assign(rows_a, rows_a + n_pairs);
  p->h_rows_b.assign(rows_b, rows_b + n_pairs);
  const uint64_t rb = std::max<uint64_t>(n_pairs, 1) * sizeof(uint32_t);
  hipError_t e = p->d_rows_a.alloc(ctx, rb);
  if (e == hipSuccess) e = p->d_rows_b.alloc(ctx, rb);
  if (e == hipSuccess) e = p->d_total.alloc(ctx, sizeof(u64));
  if (e == hipSuccess) e = p->d_done.alloc(ctx, sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemsetAsync(p->d_done.p, 0, sizeof(uint32_t), ctx->stream);
  if (e == hipSuccess && !ext_counts) e = p->d_own_counts.alloc(ctx, std::max<uint64_t>(n_pairs, 1) * sizeof(u64));
  p->d_counts = ext_counts ? static_cast<u64*>(ext_counts) : p->d_own_counts.as<u64>();
  if (e == hipSuccess && n_pairs) {
    e = hipMemcpyAsync(p->d_rows_a.p, rows_a, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_rows_b.p, rows_b, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? FBK_E_NOMEM : FBK_E_HIP, std::string("plan: ") + hipGetErrorString(e));
  }
  out_plan = std::move(p);
  return FBK_OK;
}

// |A ∩ B| of a plan over all-bitmap rows: pure streaming kernels.
int32_t plan_icount_dense(fbk_ctx* ctx, fbk_plan* p, u64* fused_total, u64* accum) {
  const uint32_t np = uint32_t(p->n_pairs);
  const uint32_t *rows_a = p->d_rows_a.as<uint32_t>(), *rows_b = p->d_rows_b.as<uint32_t>();
  // slots-per-block 16 = one block per row pair, plain store; smaller groups = more blocks + one atomicAdd per block.
  const int spb = int(ctx->opt.dense_spb);
  // A plan whose rows the Infinity Cache can hold, counted again with nothing else enqueued on the context in between
  // (hot_plan): the rows are where the last launch left them, and k_icount_dense_resident reads them in the reverse
  // of that launch's order — what was read last, and is surest to be resident still, first.  Everything else, the
  // plan's first count included, is cold data to this context: the non-temporal kernel below, unchanged.
  // (Not seen from here: other contexts, forks and processes on the device.  A hot launch after they evicted the rows
  // reads HBM with plain loads — DESIGN.md §9 has the cost.)
  const bool hot = spb == 16 && ctx->hot_plan.load() == p &&
                   fbk::dense_footprint_bound(p->n_pairs, p->a->n_rows, p->b->n_rows, p->a == p->b) <= fbk::kDenseResidentMaxBytes;
  if (hot) {
    // one block per compute unit: at 256 MiB 35.0 us against 38.1-39.5 with two to four (and 41.5 for the non-temporal kernel) —
    // the fewer blocks walk the rows at a time, the closer a launch is to the mirror of the one before (profiles/dense_resident.txt)
    const uint32_t grid = std::min<uint32_t>(np, uint32_t(ctx->n_cu > 0 ? ctx->n_cu : 256));
    p->last_rev = !p->last_rev;
    hipLaunchKernelGGL(fbk::k_icount_dense_resident<false>, dim3(grid), dim3(256), 0, ctx->stream, p->a->d_arena, rows_a, p->b->d_arena,
                       rows_b, p->d_counts, fused_total, p->d_done.as<uint32_t>(), np, accum, p->last_rev ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    return FBK_OK;  // (still the context's hot plan)
  }
  if (spb != 16) HIP_TRY(hipMemsetAsync(p->d_counts, 0, p->n_pairs * sizeof(u64), ctx->stream));
#define FBK_LAUNCH_DENSE(S)                                                                                       \
  hipLaunchKernelGGL(fbk::k_icount_dense<S>, dim3(np*(16 / S)), dim3(256), 0, ctx->stream, p->a->d_arena,         \
                     rows_a, p->b->d_arena, rows_b, p->d_counts, fused_total, p->d_done.as<uint32_t>(), np, accum)
  switch (spb) {
    case 1: FBK_LAUNCH_DENSE(1); break;
    case 2: FBK_LAUNCH_DENSE(2); break;
    case 4: FBK_LAUNCH_DENSE(4); break;
    case 8: FBK_LAUNCH_DENSE(8); break;
    default: FBK_LAUNCH_DENSE(16); break;
  }
#undef FBK_LAUNCH_DENSE
  HIP_TRY(hipGetLastError());
  // the plan is hot from here on, unless a call that is not quiet is running on the context right now (another thread's:
  // whatever it enqueues may come after this launch)
  p->last_rev = false;
  ctx->hot_plan.store(p);
  if (ctx->loud_calls.load() != 0) ctx->hot_plan.store(nullptr);
  return FBK_OK;
}

// |A ∩ B| of a plan over encoded rows: k_icount, or k_icount2 — from the plan's resolved item records where its blocks are one wave.
int32_t plan_icount_encoded(fbk_ctx* ctx, fbk_plan* p, u64* fused_total, u64* accum) {
  const uint32_t *rows_a = p->d_rows_a.as<uint32_t>(), *rows_b = p->d_rows_b.as<uint32_t>();
  ctx->hot_plan.store(nullptr);  // (the count entry points are quiet: a count over encoded rows ends a dense plan's residency here)
  const bool pk2 = use_pair_kernels2(ctx, p->a, p->b, -1);
  // (resolved item records + a count per wave pay for their second launch only where the items are heavy: one-wave blocks)
  const bool resolved = pk2 && pair_wpb_for(ctx, p->a, p->b) == 1;
  if (!resolved) HIP_TRY(hipMemsetAsync(p->d_counts, 0, p->n_pairs * sizeof(u64), ctx->stream));
  if (resolved)
    if (int32_t rc = plan_resolve_items(ctx, p)) return rc;
  if (pk2) {
#define FBK_LAUNCH_ICOUNT2(W)                                                                                                              \
  hipLaunchKernelGGL((fbk::k_icount2<W>), dim3(uint32_t((p->n_pairs * fbk::kSlots + W - 1) / W)), dim3(64 * W), 0, ctx->stream, p->a->d_slots, \
                     p->a->d_arena, rows_a, p->b->d_slots, p->b->d_arena, rows_b, p->n_pairs, p->d_counts, pair_flags,                      \
                     resolved ? p->d_items.as<Slot>() : (const Slot*)nullptr, resolved ? p->d_wave_counts.as<uint32_t>() : (uint32_t*)nullptr)
#ifdef FBK_EXPERIMENTS
    const uint32_t pair_flags = 3u | (uint32_t(ctx->opt.pair_ablate & 255) << 8) | (uint32_t(ctx->opt.pair_stamp) << 16);
#else
    constexpr uint32_t pair_flags = 3u;  // bit 0: the small-array / probe paths, bit 1: array x run items probe the run container's table (both were A/B options until round 5)
#endif
    if (pair_wpb_for(ctx, p->a, p->b) == 4) FBK_LAUNCH_ICOUNT2(4);
    else FBK_LAUNCH_ICOUNT2(1);
#undef FBK_LAUNCH_ICOUNT2
    if (resolved)
      hipLaunchKernelGGL(fbk::k_sum_wave_counts, dim3(uint32_t((p->n_pairs + 255) / 256)), dim3(256), 0, ctx->stream, p->d_wave_counts.as<uint32_t>(),
                         uint32_t(fbk::kSlots), p->n_pairs, p->d_counts);
  } else {
    hipLaunchKernelGGL(fbk::k_icount, dim3(uint32_t(p->n_pairs) * (fbk::kSlots / 4)), dim3(256), 0, ctx->stream, p->a->d_slots, p->a->d_arena, rows_a,
                       p->b->d_slots, p->b->d_arena, rows_b, p->n_pairs, p->d_counts, 1u);
  }
  if (fused_total) hipLaunchKernelGGL(fbk::k_sum_u64, dim3(1), dim3(256), 0, ctx->stream, p->d_counts, p->n_pairs, fused_total);
  if (accum) hipLaunchKernelGGL(fbk::k_sum_u64_add, dim3(1), dim3(256), 0, ctx->stream, p->d_counts, p->n_pairs, accum);
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

int32_t plan_icount_enqueue_locked(fbk_ctx* ctx, fbk_plan* p, u64* fused_total = nullptr, u64* accum = nullptr) {
  if (p->n_pairs == 0) {
    if (fused_total) HIP_TRY(hipMemsetAsync(fused_total, 0, sizeof(u64), ctx->stream));
    return FBK_OK;
  }
  return p->a->dense && p->b->dense ? plan_icount_dense(ctx, p, fused_total, accum) : plan_icount_encoded(ctx, p, fused_total, accum);
}

int32_t plan_setop_enqueue_locked(fbk_ctx* ctx, fbk_plan* p, int32_t op, bool want_runs) {
  const uint64_t n_slots = p->n_pairs * fbk::kSlots;
  if (!p->out) {
    // the output keys are derived from the inputs' host slot tables: refresh them if an input is
    // itself the output of an asynchronous operation
    if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(p->a))) return rc;
    if (int32_t rc = refresh_slots(const_cast<fbk_batch*>(p->b))) return rc;
    fbk_batch* o = nullptr;
    if (int32_t rc = alloc_cell_batch(ctx, p->n_pairs, &o, "setop output")) return rc;
    p->out.reset(o);
    o->borrowed = true;
    for (uint64_t i = 0; i < p->n_pairs; ++i)
      for (int s = 0; s < fbk::kSlots; ++s) {
        const uint64_t ia = uint64_t(p->h_rows_a[i]) * fbk::kSlots + s, ib = uint64_t(p->h_rows_b[i]) * fbk::kSlots + s;
        // a nil/nil slot pair yields nil and its key is never reported
        const bool has_a = fbk::slot_type(p->a->h_slots[ia]) != fbk::kTypeNil;
        o->h_keys[i * fbk::kSlots + s] = has_a ? p->a->h_keys[ia] : p->b->h_keys[ib];
      }
  }
  if (want_runs) HIP_TRY(p->d_runs.ensure(ctx, std::max<uint64_t>(n_slots, 1) * 4));
  if (p->n_pairs == 0) return FBK_OK;
  const bool dense = p->a->dense && p->b->dense && !want_runs;
  // the one-wave-block pair kernels start from the plan's resolved item records (as the count does)
  const Slot* items = nullptr;
  if (!dense && use_pair_kernels2(ctx, p->a, p->b, op) && pair_wpb_for(ctx, p->a, p->b) == 1) {
    if (int32_t rc = plan_resolve_items(ctx, p)) return rc;
    items = p->d_items.as<Slot>();
  }
  switch (op) {
    case FBK_OP_AND: launch_setop<0>(dense, p, ctx->stream, want_runs, items); break;
    case FBK_OP_OR: launch_setop<1>(dense, p, ctx->stream, want_runs, items); break;
    case FBK_OP_XOR: launch_setop<2>(dense, p, ctx->stream, want_runs, items); break;
    default: launch_setop<3>(dense, p, ctx->stream, want_runs, items); break;
  }
  // the pair's cardinality = the sum of the n its 16 output descriptors carry (rounds 1-3: a uint64 atomic per wave onto a
  // zeroed vector; measured equal within 1 % on config 3's 8192 row pairs, and one launch instead of memset + atomics)
  hipLaunchKernelGGL(fbk::k_sum_slot_n, dim3(uint32_t((p->n_pairs + 255) / 256)), dim3(256), 0, ctx->stream, p->out->d_slots, p->n_pairs, p->d_counts);
  HIP_TRY(hipGetLastError());
  // dense kernels write the dense layout (an all-zero result cell stays an all-zero
  // bitmap in the arena, its slot says nil): the output can feed the dense kernels again
  p->out->dense = dense;
  slots_rewritten(p->out.get());
  return FBK_OK;
}

// The plan of a one-shot call.  As with CellOutput, leaving the function in any way — a failed step, an exception out of a
// std::vector — drains the context's stream before the plan's buffers return to the pool (the destructor's body runs before
// its member is destroyed).  Declared under the context's lock and after set_device.
struct OneShotPlan {
  std::unique_ptr<fbk_plan> p;
  ~OneShotPlan() {
    if (p) (void)hipStreamSynchronize(p->ctx->stream);
  }
};

}  // namespace

extern "C" {

int32_t fbk_plan_create(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, const fbk_batch* b,
                        const uint32_t* rows_b, uint64_t n_pairs, void* device_counts_or_null, fbk_plan** out_plan) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !b || !out_plan || (n_pairs && (!rows_a || !rows_b))) return fail(FBK_E_INVALID, "NULL argument");
  *out_plan = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  std::unique_ptr<fbk_plan> p;
  if (int32_t rc = plan_create_locked(ctx, a, rows_a, b, rows_b, n_pairs, device_counts_or_null, p)) return rc;
  *out_plan = p.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_free(fbk_ctx* ctx, fbk_plan* plan) try {
  FBK_ENTER(ctx);
  if (!plan) return FBK_OK;
  if (!ctx) ctx = plan->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  delete plan;
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_intersection_count(fbk_ctx* ctx, fbk_plan* plan) try {
  FBK_ENTER_QUIET(ctx);
  if (!ctx || !plan) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return plan_icount_enqueue_locked(ctx, plan);
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_intersection_count_total(fbk_ctx* ctx, fbk_plan* plan, void* device_total_or_null) try {
  FBK_ENTER_QUIET(ctx);
  if (!ctx || !plan) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  u64* dst = device_total_or_null ? static_cast<u64*>(device_total_or_null) : plan->d_total.as<u64>();
  return plan_icount_enqueue_locked(ctx, plan, dst);
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_intersection_count_accumulate(fbk_ctx* ctx, fbk_plan* plan, void* device_accum) try {
  FBK_ENTER_QUIET(ctx);
  if (!ctx || !plan || !device_accum) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return plan_icount_enqueue_locked(ctx, plan, nullptr, static_cast<u64*>(device_accum));
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_setop(fbk_ctx* ctx, fbk_plan* plan, int32_t op, uint32_t flags) try {
  FBK_ENTER(ctx);
  if (!ctx || !plan) return fail(FBK_E_INVALID, "NULL argument");
  if (op < 0 || op > 3) return fail(FBK_E_INVALID, "unknown set operation");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  const bool opt = (flags & FBK_SETOP_OPTIMIZE) != 0;
  if (opt && ctx->opt.setop_direct_encode != 2)
    return fail(FBK_E_INVALID, "FBK_SETOP_OPTIMIZE on a plan needs option setop_direct_encode = 2 (optimize() inside the kernel); the separate re-encode pass sizes its output on the host: use fbk_setop");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  return plan_setop_enqueue_locked(ctx, plan, op, opt);
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_total(fbk_ctx* ctx, fbk_plan* plan, void* device_total_or_null) try {
  FBK_ENTER_QUIET(ctx);
  if (!ctx || !plan) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  u64* dst = device_total_or_null ? static_cast<u64*>(device_total_or_null) : plan->d_total.as<u64>();
  hipLaunchKernelGGL(fbk::k_sum_u64, dim3(1), dim3(256), 0, ctx->stream, plan->d_counts, plan->n_pairs, dst);
  HIP_TRY(hipGetLastError());
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_read(fbk_ctx* ctx, fbk_plan* plan, uint64_t* out_counts, uint64_t* out_total) try {
  FBK_ENTER_QUIET(ctx);
  if (!ctx || !plan) return fail(FBK_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  if (out_counts && plan->n_pairs)
    HIP_TRY(hipMemcpyAsync(out_counts, plan->d_counts, plan->n_pairs * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  if (out_total) HIP_TRY(hipMemcpyAsync(out_total, plan->d_total.p, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_output(fbk_ctx* ctx, fbk_plan* plan, fbk_batch** out_batch) try {
  FBK_ENTER(ctx);
  if (!plan || !out_batch) return fail(FBK_E_INVALID, "NULL argument");
  (void)ctx;
  *out_batch = plan->out.get();
  if (!plan->out) return fail(FBK_E_INVALID, "plan has no set-op output yet");
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_plan_detach_output(fbk_ctx* ctx, fbk_plan* plan, fbk_batch** out_batch) try {
  FBK_ENTER(ctx);
  if (!plan || !out_batch) return fail(FBK_E_INVALID, "NULL argument");
  if (!ctx) ctx = plan->ctx;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (!plan->out) return fail(FBK_E_INVALID, "plan has no set-op output yet");
  plan->out->borrowed = false;  // the caller's from here on: nothing rewrites it in place any more (fbk_batch_compact accepts it)
  *out_batch = plan->out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

// ---- one-shot calls (plan + enqueue + read) --------------------------------------------

int32_t fbk_intersection_count(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, const fbk_batch* b,
                               const uint32_t* rows_b, uint64_t n_pairs, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !b || (n_pairs && (!rows_a || !rows_b || !out_counts))) return fail(FBK_E_INVALID, "NULL argument");
  if (n_pairs == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  OneShotPlan shot;
  if (int32_t rc = plan_create_locked(ctx, a, rows_a, b, rows_b, n_pairs, nullptr, shot.p)) return rc;
  fbk_plan* p = shot.p.get();
  if (int32_t rc = plan_icount_enqueue_locked(ctx, p)) return rc;
  D2H back(ctx);
  hipError_t e = back.add(out_counts, p->d_counts, n_pairs * sizeof(u64));
  if (e == hipSuccess) e = back.finish();
  if (e != hipSuccess) return fail(FBK_E_HIP, std::string("intersection_count: ") + hipGetErrorString(e));
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

int32_t fbk_setop(fbk_ctx* ctx, int32_t op, const fbk_batch* a, const uint32_t* rows_a, const fbk_batch* b,
                  const uint32_t* rows_b, uint64_t n_pairs, uint32_t flags, fbk_batch** out_batch,
                  uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!ctx || !a || !b || !out_batch || (n_pairs && (!rows_a || !rows_b))) return fail(FBK_E_INVALID, "NULL argument");
  if (op < 0 || op > 3) return fail(FBK_E_INVALID, "unknown set operation");
  if (flags & ~FBK_SETOP_OPTIMIZE) return fail(FBK_E_INVALID, "unknown flags");
  *out_batch = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  OneShotPlan shot;
  if (int32_t rc = plan_create_locked(ctx, a, rows_a, b, rows_b, n_pairs, nullptr, shot.p)) return rc;
  fbk_plan* p = shot.p.get();
  const bool opt = (flags & FBK_SETOP_OPTIMIZE) != 0;
  if (int32_t rc = plan_setop_enqueue_locked(ctx, p, op, opt)) return rc;
  if (out_counts && n_pairs)
    if (hipError_t e = hipMemcpyAsync(out_counts, p->d_counts, n_pairs * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream); e != hipSuccess)
      return fail(FBK_E_HIP, std::string("setop: ") + hipGetErrorString(e));
  int32_t rc = FBK_OK;
  if (opt && ctx->opt.setop_direct_encode != 2) rc = optimize_cells(ctx, p->out.get(), p->d_runs.as<uint32_t>());  // (mode 2: the kernel has encoded already)
  else if (opt && ctx->opt.setop_compact) rc = compact_cells(ctx, p->out.get());  // ... into the head of 8 KiB cells: the caller owns this batch, it gets a right-sized arena
  if (!rc) rc = refresh_slots(p->out.get());
  if (rc) return rc;
  if (hipError_t e = hipStreamSynchronize(ctx->stream); e != hipSuccess) return fail(FBK_E_HIP, std::string("setop: ") + hipGetErrorString(e));
  p->out->borrowed = false;
  *out_batch = p->out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
