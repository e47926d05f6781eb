// fbk_count_matrix_api.inc — fbk_count_matrix: the GroupBy count matrix and its TopK shape (many rows against one).  Included by fbk.hip
// after fbk_query_api.inc and before fbk_matrix_sum_api.inc, which calls count_matrix_args_ok; fbk_count_matrix_select
// (fbk_group_select_api.inc), fbk_query_count_matrix (fbk_prepared_api.inc) and fbk_group_count_matrix (fbk_group_api.inc) run a
// MatrixPlan through the same calls.  The rules — which kernel, shards per pass, slots per block, tiles — are fbk_count_matrix_plan.h's.
//
// Unlike its siblings (MsumPlan, CubePlan) the count matrix reads the ENCODED batches and picks among four kernels:
// k_rows_vs_filter, the dense matrix-core kernel, the matrix-core kernel with the in-kernel decode, the generic pair kernel.
#include "fbk_count_matrix_plan.h"

namespace {

// The prepared program of a count matrix over encoded rows (fbk_matrix_fused.hip.h): row tables and resolved array items
// of every (shard, 32 x 32 tile, container slot) of ONE pass.  It depends on the descriptors of the three batches (their
// versions; the shadow descriptor tables when the heavy containers are shadowed) and on the row lists; a prepared query keeps
// it between runs, a one-shot call builds it, uses it and drops it.
struct FxProgram {
  DevBuf prog, items, cursor;
  uint64_t va = ~0ull, vb = ~0ull, vf = ~0ull;
  const void *sa = nullptr, *sb = nullptr, *sf = nullptr, *ra = nullptr, *rb = nullptr, *rf = nullptr;
  uint32_t pn = 0, n_a = 0, n_b = 0;
  uint64_t n_items = 0;
  bool valid = false;
};

// A count matrix from validated arguments to its totals: the row lists on the device and what a run keeps for the next one.
struct MatrixPlan {
  const fbk_batch *a = nullptr, *b = nullptr, *filter = nullptr;
  uint32_t n_a = 0, n_b = 0, n_shards = 0;
  bool keep_per_shard = false;  // the caller reads the per-shard matrices: ONE pass over all shards
  bool kept = false;            // a prepared query's plan, run again and again: it resolves the row records and keeps the fused program
  DevBuf dshard;                // the per-shard matrices of one pass
  DevBuf rows;                  // the three row lists, one allocation
  const uint32_t* dr[3] = {nullptr, nullptr, nullptr};  // A, B, filter
  RowRecords recs;              // the TopK shape of a kept plan: the resolved records of A's rows
  FxProgram fx;                 // a kept plan over encoded rows: the program of a pass that spans all shards
  uint64_t width() const { return uint64_t(n_a) * n_b; }
};

// shards [p0, p0 + pn) of a plan: their rows (rf: nullptr without a filter), d_out = dshard [pn][width] zeroed, recs: the resolved
// records of these shards' A rows or nullptr
struct MatrixPass {
  uint32_t p0, pn;
  const uint32_t *ra, *rb, *rf;
  u64* d_out;
  const Slot* recs;
};

int32_t count_matrix_args_ok(const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                             uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards) {
  if (!a || !b || (n_shards && n_a && !rows_a) || (n_shards && n_b && !rows_b) || (filter && n_shards && !rows_f))
    return fail(FBK_E_INVALID, "NULL argument");
  // a matrix is bounded by its nA x nB result; the TopK / TopN shape (one B row) takes fields with
  // millions of rows
  if (n_b == 1 ? n_a > (1u << 22) : (n_a > 4096 || n_b > 4096))
    return fail(FBK_E_INVALID, "count_matrix: at most 4096 rows per side (2^22 rows against a single row)");
  return FBK_OK;
}

// Validated arguments -> the three row-index lists checked and made device resident in ONE copy (n_shards > 0, width > 0).
int32_t matrix_prepare(fbk_ctx* ctx, MatrixPlan& p, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b,
                       uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, bool keep_per_shard) {
  p.a = a, p.b = b, p.filter = filter, p.n_a = n_a, p.n_b = n_b, p.n_shards = n_shards, p.keep_per_shard = keep_per_shard;
  if (int32_t rc = check_rows(rows_a, uint64_t(n_shards) * n_a, a->n_rows, "count_matrix A")) return rc;
  if (int32_t rc = check_rows(rows_b, uint64_t(n_shards) * n_b, b->n_rows, "count_matrix B")) return rc;
  return upload_rows_multi(ctx,
                           {{rows_a, uint64_t(n_shards) * n_a, UINT32_MAX}, {rows_b, uint64_t(n_shards) * n_b, UINT32_MAX},
                            {rows_f, filter ? uint64_t(n_shards) : 0, filter ? filter->n_rows : UINT32_MAX}},
                           p.rows, p.dr);
}

int32_t fused_program_build(fbk_ctx* ctx, FxProgram& fp, const fbk_batch* a, const Slot* sla, const uint4* wa, const uint32_t* ra, uint32_t n_a, const fbk_batch* b,
                            const Slot* slb, const uint4* wb, const uint32_t* rb, uint32_t n_b, const fbk_batch* filter, const Slot* slf, const uint4* wf,
                            const uint32_t* rf, uint32_t pn, bool kept = false) {
  const uint64_t vf = filter ? filter->version : 0;
  if (fp.valid && fp.va == a->version && fp.vb == b->version && fp.vf == vf && fp.sa == sla && fp.sb == slb && fp.sf == slf && fp.ra == ra && fp.rb == rb && fp.rf == rf &&
      fp.pn == pn && fp.n_a == n_a && fp.n_b == n_b)
    return FBK_OK;
  fp.valid = false;
  const uint64_t agroups = (n_a + 31) / 32, btiles = (n_b + 31) / 32;
  const uint64_t units = uint64_t(pn) * agroups * btiles * fbk::kSlots;
  // items: k_fused_program emits ceil(values / 128) items per array row OCCURRENCE and stage.  A first guess — every row an item in
  // every stage plus one per 256 payload bytes of the three arenas, at most 4 M items (64 MB) — is right when every batch row is
  // listed about once; the kernel counts what it needs whether or not it fits (one atomic per unit), so a pass that lists rows
  // many times over (duplicates in a row list, one row broadcast to every shard) or a small pass over a multi-GB batch gets a
  // second launch with exactly that many.
  const uint64_t guess = units * uint64_t(fbk::kFxNR) * fbk::kFxStages + (a->arena_bytes * btiles + b->arena_bytes * agroups + (filter ? filter->arena_bytes * agroups * btiles : 0)) / 256 + 64;
  uint64_t cap = std::min<uint64_t>(guess, 4ull << 20);
  HIP_TRY(fp.prog.ensure(ctx, units * sizeof(fbk::FxProg)));
  HIP_TRY(fp.cursor.ensure(ctx, 16));
  const dim3 grid(uint32_t((units + 3) / 4));
  u64 cur[2] = {0, 0};
  for (int attempt = 0;; ++attempt) {
    if (cap > 0xFFFFFFFFull) return fail(FBK_E_INVALID, "count_matrix: more than 2^32 array items in one pass (lower matrix_pass_kb)");
    HIP_TRY(fp.items.ensure(ctx, std::max<uint64_t>(cap, 1) * sizeof(fbk::FxItem)));
    HIP_TRY(hipMemsetAsync(fp.cursor.p, 0, 16, ctx->stream));
    if (filter)
      hipLaunchKernelGGL(fbk::k_fused_program<true>, grid, dim3(256), 0, ctx->stream, sla, a->d_arena, wa, ra, n_a, slb, b->d_arena, wb, rb, n_b, slf, filter->d_arena, wf, rf, pn,
                         fp.prog.as<fbk::FxProg>(), fp.items.as<fbk::FxItem>(), fp.cursor.as<u64>(), u64(cap));
    else
      hipLaunchKernelGGL(fbk::k_fused_program<false>, grid, dim3(256), 0, ctx->stream, sla, a->d_arena, wa, ra, n_a, slb, b->d_arena, wb, rb, n_b, (const Slot*)nullptr,
                         (const uint8_t*)nullptr, (const uint4*)nullptr, (const uint32_t*)nullptr, pn, fp.prog.as<fbk::FxProg>(), fp.items.as<fbk::FxItem>(), fp.cursor.as<u64>(),
                         u64(cap));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cur, fp.cursor.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!cur[1]) break;
    if (attempt || cur[0] <= cap) return fail(FBK_E_INVALID, "count_matrix: the program's item area was too small (a corrupt window index?)");
    cap = cur[0];  // what the pass needs: counted by the launch that did not fit
  }
  fp.n_items = cur[0];
  // the item area was sized by a guess: a program that
  // stays — a prepared query's — keeps only what was written (the items' indexes are relative to the area: nothing else moves)
  if (kept && fp.n_items * sizeof(fbk::FxItem) * 2 < cap * sizeof(fbk::FxItem) && cap * sizeof(fbk::FxItem) > (8u << 20)) {
    DevBuf tight;
    if (tight.alloc(ctx, std::max<uint64_t>(fp.n_items, 1) * sizeof(fbk::FxItem)) == hipSuccess) {
      HIP_TRY(hipMemcpyAsync(tight.p, fp.items.p, fp.n_items * sizeof(fbk::FxItem), hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      std::swap(tight.p, fp.items.p);
      std::swap(tight.cap, fp.items.cap);
      std::swap(tight.c, fp.items.c);
    } else {
      (void)hipGetLastError();
    }
  }
  fp.va = a->version, fp.vb = b->version, fp.vf = vf, fp.sa = sla, fp.sb = slb, fp.sf = slf, fp.ra = ra, fp.rb = rb, fp.rf = rf, fp.pn = pn, fp.n_a = n_a, fp.n_b = n_b;
  fp.valid = true;
  return FBK_OK;
}

// THE launch of k_rows_vs_filter (the count matrix's TopK shape below, TopN over a filter row in fbk_topn_api.inc): pn shards,
// shard s counts rows ra[s][0 .. n_a) of `a` against row rf[s] of `f` into d_out [pn][n_a] (zeroed by the caller); recs: the
// resolved records of a's rows or nullptr.  The rows per block are fbk_expr::rows_per_block with no tree to re-evaluate (L = 0).
void launch_rows_vs_filter(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* ra, uint32_t n_a, const fbk_batch* f, const uint32_t* rf, uint32_t pn, u64* d_out,
                           const Slot* recs) {
  const uint32_t rpb = fbk_expr::rows_per_block(n_a, pn, 0);
  const uint32_t chunks = (n_a + rpb - 1) / rpb;
  hipLaunchKernelGGL(fbk::k_rows_vs_filter, dim3(pn * 16 * chunks), dim3(256), 0, ctx->stream, a->d_slots, a->d_arena, ra, n_a, f->d_slots, f->d_arena, rf, pn, rpb,
                     d_out, recs);
}

// many rows x one row (doTopK / fragment.top): the single B row is the filter of k_rows_vs_filter
void matrix_pass_rows_vs_filter(fbk_ctx* ctx, const MatrixPlan& p, const MatrixPass& s) {
  launch_rows_vs_filter(ctx, p.a, s.ra, p.n_a, p.b, s.rb, s.pn, s.d_out, s.recs);
}

// The dense count-matrix launch: the matrix-core kernel (fbk_matrix_mfma.hip.h), every container a bitmap at a fixed address.
// A block covers `spb` of a shard's 16 slots: whole shards (plain stores) when that still gives
// two blocks per CU, otherwise fewer slots per block (atomic adds into the per-shard matrix);
// FBK_MATRIX_SPB=1|2|4|8|16 pins it (tests walk every value).
void matrix_pass_dense(fbk_ctx* ctx, const MatrixPlan& p, const MatrixPass& s) {
  namespace mp = fbk_count_matrix_plan;
  const uint8_t *arenaA = p.a->d_arena, *arenaB = p.b->d_arena, *arenaF = p.filter ? p.filter->d_arena : nullptr;
  const uint32_t *rowsA = s.ra, *rowsB = s.rb, *rowsF = s.rf;
  const uint32_t n_a = p.n_a, n_b = p.n_b, n_shards = s.pn;
  u64* out_shard = s.d_out;
  const mp::DenseTiles t = mp::dense_tiles(n_a, n_b);
  const uint32_t tm = t.tm, tn = t.tn, tiles = t.tiles;
  const uint32_t spb = mp::slots_per_block(tiles, n_shards, mp::kDenseFloor, mp::kDenseEnough, uint32_t(ctx->opt.matrix_spb));
  uint32_t blocks = n_shards * (16 / spb) * tiles;
  // A single-tile matrix (the HBM-bound shape) takes its units by TICKET, long units first (fbk_matrix_mfma.hip.h): the XCDs do not
  // run at one pace, and a launch by block id gives each an eighth of the work whatever its pace.  matrix_tickets = 0 pins the
  // launch by block id (the A/B and the cross-check).
  fbk::MmTickets tk{0, 0, 0, 0};
  uint32_t* d_ticket = nullptr;
  if (tiles == 1 && ctx->opt.matrix_tickets && fbk::mm_ticket_plan(n_shards, spb, 2u * uint32_t(std::max(ctx->n_cu, 1)), tk) && ticket_counter(ctx, &d_ticket) == FBK_OK)
    blocks = tk.grid;
  constexpr int W = fbk::kMmWaves, D = fbk::kMmDepth, AUX = fbk::kMmAux;
#define FBK_MM(F, TM, TN, P4)                                                                                                        \
  hipLaunchKernelGGL((fbk::k_count_matrix_mfma<F, W, D, AUX, TM, TN, P4>), dim3(blocks), dim3(W * 64), 0, ctx->stream, arenaA, rowsA, \
                     n_a, arenaB, rowsB, n_b, arenaF, rowsF, n_shards, spb, out_shard, d_ticket, tk.tier0_shards, tk.tier1_shards, tk.tier_spb)
#define FBK_MM_F(TM, TN)                      \
  do {                                        \
    if (arenaF && fp4) FBK_MM(true, TM, TN, true);   \
    else if (arenaF) FBK_MM(true, TM, TN, false);    \
    else if (fp4) FBK_MM(false, TM, TN, true);       \
    else FBK_MM(false, TM, TN, false);               \
  } while (0)
  // matrix_fp4: 1 / 0 pins the FP4 matrix instruction, -1: matrices of several tiles (matrix-core
  // bound) use it, a single 32 x 32 tile (HBM-bound) stays on the i8 instruction
  const bool fp4 = ctx->opt.matrix_fp4 == 1 || (ctx->opt.matrix_fp4 < 0 && tiles > 1);
  if (tm == 2 && tn == 2) FBK_MM_F(2, 2);
  else if (tm == 2) FBK_MM_F(2, 1);
  else if (tn == 2) FBK_MM_F(1, 2);
  else FBK_MM_F(1, 1);
#undef FBK_MM_F
#undef FBK_MM
}

#ifdef FBK_EXPERIMENTS
// option matrix_fused_ablate: the low five bits make the fused kernel skip work, 32 asks for the cycle stamps below; the product library has none of it
uint32_t fused_ablate(const fbk_ctx* ctx) { return uint32_t(ctx->opt.matrix_fused_ablate); }

// timing experiment (option matrix_fused_ablate, bit 32): the instrumented build of the fused kernel on a program of its own; the
// cycle stamps of the grid's middle block go to stderr
int32_t fused_cycle_stamps(fbk_ctx* ctx, const MatrixPlan& p, const MatrixPass& s, const Slot* sla, const uint4* wa, const Slot* slb, const uint4* wb, const Slot* slf,
                           const uint4* wf, uint32_t spb, uint32_t blocks, uint32_t abl) {
  DevBuf dprof;
  constexpr size_t kProfWords = size_t(fbk::kFxWaves) * 24 * 8;
  HIP_TRY(dprof.alloc(ctx, kProfWords * 8));
  HIP_TRY(hipMemsetAsync(dprof.p, 0, kProfWords * 8, ctx->stream));
  FxProgram fpp;
  if (int32_t rc = fused_program_build(ctx, fpp, p.a, sla, wa, s.ra, p.n_a, p.b, slb, wb, s.rb, p.n_b, p.filter, slf, wf, s.rf, s.pn)) return rc;
  hipLaunchKernelGGL((fbk::k_count_matrix_fusedq<true, true>), dim3(blocks), dim3(fbk::kFxWaves * 64), 0, ctx->stream, fpp.prog.as<fbk::FxProg>(),
                     fpp.items.as<fbk::FxItem>(), p.n_a, p.n_b, s.pn, spb, s.d_out, dprof.as<u64>(), abl & 31u);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  std::vector<u64> h(kProfWords);
  HIP_TRY(hipMemcpyAsync(h.data(), dprof.p, kProfWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  u64 t0 = ~0ull;
  for (u64 v : h)
    if (v) t0 = std::min(t0, v);
  std::fprintf(stderr, "[fused prof] block %u of %u; per stage and wave, cycles since the block's first stamp: start/loads/bitmaps/arrays/runs/barrier\n", blocks / 2, blocks);
  for (uint32_t st = 0; st < 24; ++st) {
    if (!h[(size_t(fbk::kFxConsumers) * 24 + st) * 8 + 5] && !h[(0 * 24 + st) * 8 + 5]) continue;
    for (uint32_t w = 0; w < uint32_t(fbk::kFxWaves); ++w) {
      const u64* q = &h[(size_t(w) * 24 + st) * 8];
      std::fprintf(stderr, "st %2u %c%-2u", st, w < uint32_t(fbk::kFxConsumers) ? 'c' : 'p', w);
      for (int k = 0; k < 6; ++k) std::fprintf(stderr, " %7lld", q[k] ? (long long)(q[k] - t0) : -1ll);
      std::fprintf(stderr, "\n");
    }
  }
  return FBK_OK;
}
#else
constexpr uint32_t fused_ablate(const fbk_ctx*) { return 0; }
#endif

// array / run containers among the rows: decoded inside the matrix-core kernel, a stage of 8192
// bit positions at a time (fbk_matrix_fused.hip.h) — the encoded payload is the only HBM traffic
// and no temporary rows are allocated.  ~400 us against 681 + 347 us for densify + dense kernel on
// 256 shards of config 3's rows; the kernel is bound by instruction issue (DESIGN.md section 9).
// matrix_fused=0 selects the generic pair kernel.  span: restarted once the program stands, which is preparation, not the kernel.
int32_t matrix_pass_fused(fbk_ctx* ctx, MatrixPlan& p, const MatrixPass& s, KernelSpan& span) {
  namespace mp = fbk_count_matrix_plan;
  const fbk_batch *a = p.a, *b = p.b, *filter = p.filter;
  const uint32_t n_a = p.n_a, n_b = p.n_b, pn = s.pn;
  const uint32_t tiles = mp::tiles32(n_a, n_b);
  const uint32_t spb = mp::slots_per_block(tiles, pn, mp::kFusedFloor, mp::fused_enough(ctx->n_cu), uint32_t(ctx->opt.matrix_spb));
  const uint32_t blocks = pn * (16 / spb) * tiles;
  const uint32_t abl = fused_ablate(ctx);
  // the batches' window indexes (16 bytes per container, built on first use) are what the kernel's work lists come from
  const uint4 *wa = nullptr, *wb = nullptr, *wf = nullptr;
  if (int32_t rc = window_index(ctx, a, &wa)) return rc;
  if (int32_t rc = window_index(ctx, b, &wb)) return rc;
  if (filter)
    if (int32_t rc = window_index(ctx, filter, &wf)) return rc;
  // heavy containers (runs, long arrays) as dense shadows, built per batch on first use (option matrix_shadow)
  const Slot *sla = a->d_slots, *slb = b->d_slots, *slf = filter ? filter->d_slots : nullptr;
  bool sha = false, shb = false, shf = false;
  if (int32_t rc = heavy_shadow(ctx, a, &sla, &sha)) return rc;
  if (int32_t rc = heavy_shadow(ctx, b, &slb, &shb)) return rc;
  if (filter)
    if (int32_t rc = heavy_shadow(ctx, filter, &slf, &shf)) return rc;
#ifdef FBK_EXPERIMENTS
  if (filter && (abl & 32u)) return fused_cycle_stamps(ctx, p, s, sla, wa, slb, wb, slf, wf, spb, blocks, abl);
#endif
  // the prepared program (row tables + resolved array items), then the kernel that runs it.  A kept plan's program serves a pass
  // that spans all shards; any other pass — of a one-shot call, or one of several — builds its own, uses it and drops it.
  FxProgram pass_program;
  const bool keep = p.kept && s.p0 == 0 && pn == p.n_shards;
  FxProgram& fp = keep ? p.fx : pass_program;
  if (int32_t rc = fused_program_build(ctx, fp, a, sla, wa, s.ra, n_a, b, slb, wb, s.rb, n_b, filter, slf, wf, s.rf, pn, keep)) return rc;
  span.restart();
  const fbk::FxProg* pp = fp.prog.as<fbk::FxProg>();
  const fbk::FxItem* pi = fp.items.as<fbk::FxItem>();
  if (filter)
    hipLaunchKernelGGL((fbk::k_count_matrix_fusedq<true, false>), dim3(blocks), dim3(fbk::kFxWaves * 64), 0, ctx->stream, pp, pi, n_a, n_b, pn, spb, s.d_out, (u64*)nullptr,
                       abl & 31u);
  else
    hipLaunchKernelGGL((fbk::k_count_matrix_fusedq<false, false>), dim3(blocks), dim3(fbk::kFxWaves * 64), 0, ctx->stream, pp, pi, n_a, n_b, pn, spb, s.d_out, (u64*)nullptr,
                       abl & 31u);
  return FBK_OK;
}

// the generic pair kernel (fbk_query_kernels.hip.h): any encoding, the B rows in launches of 256
void matrix_pass_generic(fbk_ctx* ctx, const MatrixPlan& p, const MatrixPass& s) {
  namespace mp = fbk_count_matrix_plan;
  const FilterArgs f(p.filter, s.rf);
  const uint32_t agroups = mp::generic_agroups(p.n_a);
  const uint32_t spb = mp::slots_per_block(agroups, s.pn, mp::kGenericFloor, mp::kGenericEnough, 0);
  const uint32_t blocks = s.pn * (16 / spb) * agroups;
  for (uint32_t j0 = 0; j0 < p.n_b; j0 += 256) {
    const uint32_t nbc = std::min<uint32_t>(256, p.n_b - j0);
    hipLaunchKernelGGL(fbk::k_count_matrix<mp::kGenericTA>, dim3(blocks), dim3(512), 0, ctx->stream, p.a->d_slots, p.a->d_arena, s.ra, p.n_a, p.b->d_slots, p.b->d_arena,
                       s.rb, p.n_b, j0, nbc, f.slots, f.arena, s.rf, s.pn, spb, s.d_out);
  }
}

// One execution, launch-only: the totals over the plan's shards end up in d_total (device, width uint64; accumulate: added to what it
// holds, otherwise zeroed here first) and — keep_per_shard — the per-shard matrices in p.dshard.  The caller (a one-device entry
// point, a prepared query's run, the multi-device group reduce of fbk_group_api.inc) decides how the totals leave the device.
int32_t matrix_enqueue(fbk_ctx* ctx, MatrixPlan& p, u64* d_total, bool accumulate) {
  namespace mp = fbk_count_matrix_plan;
  const uint64_t width = p.width();
  const uint32_t n_a = p.n_a, n_b = p.n_b, n_shards = p.n_shards;
  const mp::Path path = mp::path(n_a, n_b, p.filter != nullptr, p.a->dense && p.b->dense && (!p.filter || p.filter->dense), int(ctx->opt.matrix_fused));
  const Slot* recs = nullptr;  // (only a kept plan resolves them; a one-shot call's kernel gathers the descriptors itself)
  if (p.kept && path == mp::kRowsVsFilter)
    if (int32_t rc = query_row_records(ctx, p.recs, p.a, p.dr[0], n_shards, n_a, &recs)) return rc;
  // (a kept plan keeps its per-shard matrices between runs: sized for THIS run's pass — option matrix_pass_kb may have been
  // raised since the run that allocated them)
  const uint64_t pass_shards = mp::pass_shards(n_shards, width, uint64_t(ctx->opt.matrix_pass_kb), p.keep_per_shard);
  HIP_TRY(p.dshard.ensure(ctx, pass_shards * width * 8));
  if (!accumulate) HIP_TRY(hipMemsetAsync(d_total, 0, width * 8, ctx->stream));
  for (uint64_t q0 = 0; q0 < n_shards; q0 += pass_shards) {  // shards [p0, p0 + pn) -> dshard[0 .. pn)
    const uint32_t p0 = uint32_t(q0), pn = uint32_t(std::min<uint64_t>(pass_shards, n_shards - q0));
    const MatrixPass s{p0, pn, p.dr[0] + uint64_t(p0) * n_a, p.dr[1] + uint64_t(p0) * n_b, p.filter ? p.dr[2] + p0 : nullptr, p.dshard.as<u64>(),
                       recs ? recs + uint64_t(p0) * fbk::kSlots * n_a : nullptr};
    HIP_TRY(hipMemsetAsync(s.d_out, 0, uint64_t(pn) * width * 8, ctx->stream));
    {
      KernelSpan span(ctx);
      switch (path) {
        case mp::kRowsVsFilter: matrix_pass_rows_vs_filter(ctx, p, s); break;
        case mp::kDense: matrix_pass_dense(ctx, p, s); break;
        case mp::kFused:
          if (int32_t rc = matrix_pass_fused(ctx, p, s, span)) return rc;
          break;
        case mp::kGeneric: matrix_pass_generic(ctx, p, s); break;
      }
    }
    hipLaunchKernelGGL(fbk::k_reduce_shards, dim3(uint32_t((width + 255) / 256), std::min<uint32_t>(pn, 64)), dim3(256), 0, ctx->stream, s.d_out, pn, width, d_total);
    HIP_TRY(hipGetLastError());
  }
  return FBK_OK;
}

// the totals of the last run (d_total: where it wrote them) and, from a plan with keep_per_shard, the per-shard matrices to the host
int32_t matrix_read(fbk_ctx* ctx, MatrixPlan& p, const u64* d_total, uint64_t* out_total, uint64_t* out_per_shard) {
  D2H back(ctx);
  if (out_total) HIP_TRY(back.add(out_total, d_total, p.width() * 8));
  if (out_per_shard) HIP_TRY(back.add(out_per_shard, p.dshard.p, uint64_t(p.n_shards) * p.width() * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_count_matrix(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                         const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                         uint32_t n_shards, uint64_t* out_total, uint64_t* out_per_shard) try {
  FBK_ENTER(ctx);
  if (!ctx) return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = count_matrix_args_ok(a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  const uint64_t width = uint64_t(n_a) * n_b;
  if (out_total) std::memset(out_total, 0, width * 8);
  if (n_shards == 0 || width == 0) return FBK_OK;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  MatrixPlan p;
  DevBuf dtot;  // (the pooled blocks in this order: totals, row lists, per-shard matrices)
  HIP_TRY(dtot.alloc(ctx, width * 8));
  if (int32_t rc = matrix_prepare(ctx, p, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards, out_per_shard != nullptr)) return rc;
  if (int32_t rc = matrix_enqueue(ctx, p, dtot.as<u64>(), false)) return rc;
  return matrix_read(ctx, p, dtot.as<u64>(), out_total, out_per_shard);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
