// fbk_count_cube_api.inc — fbk_count_cube: GroupBy over three fields in one pass over the operands per shard
// (fbk_matrix_cube.hip.h).  Included by fbk.hip after fbk_matrix_sum_api.inc.
//
// The matrix kernel reads dense rows (fbk_dense_operands.inc), a chunk of shards at a time.  The per-shard partial cubes share the
// chunk's budget, kCubeScratch: per shard 8 bytes per cell + 128 KiB per densified row.  (fbk.h documents the arithmetic: the
// tests rely on it.)

namespace {

constexpr uint64_t kCubeScratch = 1ull << 30;
constexpr uint64_t kCubeMaxCells = 1ull << 24;

struct CubePlan {
  uint32_t n_p = 0, n_a = 0, n_b = 0;
  DenseOperands ops;
  int P = 0, A = 0, B = 0, F = 0;  // its operands: the rows of the three fields, the filter row
  DevBuf dshard, result;
  uint64_t cells() const { return uint64_t(n_p) * n_a * n_b; }
};

int32_t cube_args_ok(const fbk_batch* p, const uint32_t* rows_p, uint32_t n_p, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a,
                     const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards) {
  if (n_p > 4096 || n_a > 4096 || n_b > 4096 || uint64_t(n_p) * n_a * n_b > kCubeMaxCells)
    return fail(FBK_E_INVALID, "count_cube: at most 4096 rows per field and 2^24 groups per call: block the leading field");
  if (!p || !a || !b || (n_shards && n_p && !rows_p) || (n_shards && n_a && !rows_a) || (n_shards && n_b && !rows_b) || (filter && n_shards && !rows_f))
    return fail(FBK_E_INVALID, "NULL argument");
  if (int32_t rc = check_rows(rows_p, uint64_t(n_shards) * n_p, p->n_rows, "count_cube P")) return rc;
  if (int32_t rc = check_rows(rows_a, uint64_t(n_shards) * n_a, a->n_rows, "count_cube A")) return rc;
  if (int32_t rc = check_rows(rows_b, uint64_t(n_shards) * n_b, b->n_rows, "count_cube B")) return rc;
  if (filter)
    if (int32_t rc = check_rows(rows_f, n_shards, filter->n_rows, "count_cube filter")) return rc;
  return FBK_OK;
}

// Validated arguments -> row lists on the device, scratch and result allocated: everything a run needs (n_shards > 0, cells > 0).
int32_t cube_prepare(fbk_ctx* ctx, CubePlan& c, const fbk_batch* p, const uint32_t* rows_p, uint32_t n_p, const fbk_batch* a, const uint32_t* rows_a,
                     uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                     uint32_t n_shards) {
  c.n_p = n_p, c.n_a = n_a, c.n_b = n_b;
  c.P = c.ops.add(p, rows_p, n_p), c.A = c.ops.add(a, rows_a, n_a), c.B = c.ops.add(b, rows_b, n_b), c.F = c.ops.add(filter, rows_f, 1);
  const uint32_t chunk = even_chunk(n_shards, kCubeScratch, kDenseRowBytes * c.ops.densified_rows() + 8 * c.cells());
  if (int32_t rc = c.ops.upload(ctx, n_shards, chunk)) return rc;
  HIP_TRY(c.dshard.alloc(ctx, uint64_t(chunk) * c.cells() * 8));
  HIP_TRY(c.result.alloc(ctx, c.cells() * 8));
  return FBK_OK;
}

// One execution, launch-only: c.result = the cube [n_p * n_a * n_b] (u64).
int32_t cube_enqueue(fbk_ctx* ctx, CubePlan& c) {
  if (c.ops.layout_changed()) return fail(FBK_E_INVALID, "count_cube: a batch changed its layout since the call was prepared");
  const uint64_t cells = c.cells();
  const uint32_t n_p = c.n_p, n_a = c.n_a, n_b = c.n_b;
  HIP_TRY(hipMemsetAsync(c.result.p, 0, cells * 8, ctx->stream));
  KernelSpan span(ctx);
  namespace mp = fbk_count_matrix_plan;  // P rows per block, tiles, slots per block
  const uint32_t pt = mp::cube_pt(n_p);
  const uint64_t tiles = mp::cube_tiles(n_p, n_a, n_b);
  if (int32_t rc = c.ops.for_each_chunk(ctx, true, DenseOperands::Densify::together, [&](uint32_t s0, uint32_t ns) -> int32_t {
    const DenseView P = c.ops.view(c.P, s0), A = c.ops.view(c.A, s0), B = c.ops.view(c.B, s0), F = c.ops.view(c.F, s0);
    HIP_TRY(hipMemsetAsync(c.dshard.p, 0, uint64_t(ns) * cells * 8, ctx->stream));
    const uint32_t spb = mp::slots_per_block(tiles, ns, mp::kCubeFloor, mp::kCubeEnough, uint32_t(ctx->opt.matrix_spb));  // tests walk every value
    // a launch takes as many of the chunk's shards as a grid has block ids for
    const uint64_t per_shard = (16 / spb) * tiles;
    const uint32_t most = uint32_t(std::min<uint64_t>(ns, std::max<uint64_t>(1, uint64_t(INT32_MAX) / per_shard)));
    for (uint32_t t0 = 0; t0 < ns; t0 += most) {
      const uint32_t nt = std::min(most, ns - t0);
      const dim3 grid(uint32_t(nt * per_shard));
      const uint32_t *rp = P.rows + uint64_t(t0) * P.stride, *ra = A.rows + uint64_t(t0) * A.stride, *rb = B.rows + uint64_t(t0) * B.stride;
      const uint32_t* rf = F.rows ? F.rows + uint64_t(t0) * F.stride : nullptr;
      u64* out = c.dshard.as<u64>() + uint64_t(t0) * cells;
#define FBK_CUBE(PT, HAS_F)                                                                                                                       \
  hipLaunchKernelGGL((fbk::k_cube_mfma<PT, HAS_F>), grid, dim3(256), 0, ctx->stream, P.arena, rp, n_p, A.arena, ra, n_a, B.arena, rb, n_b, F.arena, rf, \
                     nt, spb, out)
      if (pt == 4 && F.arena) FBK_CUBE(4, true);
      else if (pt == 4) FBK_CUBE(4, false);
      else if (F.arena) FBK_CUBE(8, true);
      else FBK_CUBE(8, false);
#undef FBK_CUBE
    }
    hipLaunchKernelGGL(fbk::k_reduce_shards, dim3(uint32_t((cells + 255) / 256), std::min<uint32_t>(ns, 64)), dim3(256), 0, ctx->stream, c.dshard.as<u64>(), ns,
                       cells, c.result.as<u64>());
    return FBK_OK;
  })) return rc;
  HIP_TRY(hipGetLastError());
  return FBK_OK;
}

// the result of the last run to the host
int32_t cube_read(fbk_ctx* ctx, CubePlan& c, uint64_t* out_total) {
  D2H back(ctx);
  HIP_TRY(back.add(out_total, c.result.p, c.cells() * 8));
  HIP_TRY(back.finish());
  return FBK_OK;
}

}  // namespace

extern "C" {

int32_t fbk_count_cube(fbk_ctx* ctx, const fbk_batch* p, const uint32_t* rows_p, uint32_t n_p, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a,
                       const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards,
                       uint64_t* out_total) try {
  FBK_ENTER(ctx);
  if (int32_t rc = cube_args_ok(p, rows_p, n_p, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  if (!ctx || !out_total) return fail(FBK_E_INVALID, "NULL argument");
  const uint64_t cells = uint64_t(n_p) * n_a * n_b;
  if (n_shards == 0 || cells == 0) {
    std::memset(out_total, 0, cells * 8);
    return FBK_OK;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;
  CubePlan c;
  if (int32_t rc = cube_prepare(ctx, c, p, rows_p, n_p, a, rows_a, n_a, b, rows_b, n_b, filter, rows_f, n_shards)) return rc;
  if (int32_t rc = cube_enqueue(ctx, c)) return rc;
  return cube_read(ctx, c, out_total);
} FBK_ABI_CATCH(ctx)

}  // extern "C"
