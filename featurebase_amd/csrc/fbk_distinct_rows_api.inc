// fbk_distinct_rows_api.inc — fbk_bsi_distinct_rows (Distinct() over an int field as a device Row, the operand of a join):
// fbk_distinct_rows.hip.h.  Included by fbk.hip after fbk_quantile_api.inc.
//
// Two walks over the shards (presence, scatter) of fbk_bsi_sort's FieldOperands (fbk_sort_api.inc).  Device scratch beyond the
// output arena (fbk.h documents it): the densify chunk (<= 2^28), two presence bitmaps of <= 2^20 bytes, their word prefixes (half
// of that), the run counts and cardinalities of the output cells, the row lists.

namespace {

// the window of one sign from its smallest and largest position; false: wider than the presence bitmap
bool drow_window(uint64_t p_lo, uint64_t p_hi, u64* lo, uint32_t* span) {
  const uint64_t a = p_lo >> 20, b = p_hi >> 20;
  if (b - a >= fbk::kDrowWindowShards) return false;
  *lo = a, *span = uint32_t(b - a + 1);
  return true;
}

}  // namespace

extern "C" {

int32_t fbk_bsi_distinct_rows(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, int64_t base, const fbk_batch* filter,
                              const uint32_t* rows_f, uint32_t n_shards, uint32_t flags, fbk_batch** out_batch, uint64_t* out_shard_ids, uint64_t cap,
                              uint32_t* out_n_pos, uint32_t* out_n_neg, uint64_t* out_counts) try {
  FBK_ENTER(ctx);
  if (!out_batch || !out_n_pos || !out_n_neg || (cap && !out_shard_ids)) return fail(FBK_E_INVALID, "NULL argument");
  *out_batch = nullptr;
  *out_n_pos = *out_n_neg = 0;
  if (bit_depth > 63)
    return fail(FBK_E_INVALID, "distinct rows: bit depth > 63 (a magnitude of 2^63 and more has no position in a row); fbk_bsi_distinct returns such a field's values");
  if (flags & ~uint32_t(FBK_SETOP_OPTIMIZE)) return fail(FBK_E_INVALID, "distinct rows: unknown flags");
  if (int32_t rc = field_args_ok(ctx, bsi, base_rows, bit_depth, filter, rows_f, n_shards, 1u << 20, "distinct rows: at most 2^20 shards per call", "distinct rows filter")) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int32_t rc = set_device(ctx)) return rc;

  FieldOperands fo;  // (n_shards == 0: never uploaded, never walked)
  fo.add(bsi, base_rows, bit_depth, filter, rows_f, n_shards);
  DevBuf pres, pre, inner;

  // 1. the window of shards per sign: by arithmetic where 2^bit_depth + |base| bounds it, else from the minimum and the maximum
  fbk::DrowWindow win{};
  const uint64_t abs_base = base < 0 ? 0 - uint64_t(base) : uint64_t(base);
  bool uploaded = false;
  if (n_shards && bit_depth < 44 && abs_base < (1ull << 44) && (((1ull << bit_depth) + abs_base) >> 20) < fbk::kDrowWindowShards) {
    win.span[0] = win.span[1] = uint32_t(((1ull << bit_depth) + abs_base) >> 20) + 1;  // (stored + base stays far inside int64)
  } else if (n_shards) {
    std::vector<int64_t> mv(n_shards);
    std::vector<uint64_t> mc(n_shards);
    int64_t ext[2] = {0, 0};  // the smallest, the largest stored value
    bool any = false;
    for (uint32_t mode = 0; mode < 2; ++mode) {
      if (int32_t rc = bsi_minmax_locked(ctx, bsi, base_rows, n_shards, bit_depth, mode, filter, rows_f, mv.data(), mc.data())) return rc;
      ctx->h_stage_used = 0;  // (its row lists have left the staging area)
      bool first = true;
      for (uint32_t s = 0; s < n_shards; ++s) {
        if (!mc[s]) continue;
        if (first || (mode ? mv[s] > ext[mode] : mv[s] < ext[mode])) ext[mode] = mv[s];
        first = false, any = true;
      }
    }
    if (any) {
      int64_t vmin, vmax;
      if (__builtin_add_overflow(ext[0], base, &vmin) || __builtin_add_overflow(ext[1], base, &vmax))
        return fail(FBK_E_INVALID, "distinct rows: minimum + base or maximum + base is outside int64");
      // the outer end of a sign is the minimum / maximum; its inner end is the other one, or with values of both signs 0
      uint64_t in[2] = {uint64_t(std::max<int64_t>(vmin, 0)), 0 - uint64_t(std::min<int64_t>(vmax, -1))};
      bool ok_pos = vmax < 0 || drow_window(in[0], uint64_t(vmax), &win.lo[0], &win.span[0]);
      bool ok_neg = vmin >= 0 || drow_window(in[1], 0 - uint64_t(vmin), &win.lo[1], &win.span[1]);
      if ((!ok_pos || !ok_neg) && vmin < 0 && vmax >= 0) {
        // ... unless that is too wide a guess: one walk finds the smallest position of either sign
        if (int32_t rc = fo.upload(ctx)) return rc;
        uploaded = true;
        HIP_TRY(inner.alloc(ctx, 16));
        HIP_TRY(hipMemsetAsync(inner.p, 0xFF, 16, ctx->stream));
        fo.for_each_chunk(ctx, [&](const DenseView& S, const DenseView& F, uint32_t, uint32_t ns, dim3 grid) {
          hipLaunchKernelGGL(fbk::k_drow_inner, grid, dim3(256), 0, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, bit_depth, u64(base), inner.as<u64>());
        });
        HIP_TRY(hipGetLastError());
        D2H back(ctx);
        HIP_TRY(back.add(in, inner.p, 16));
        HIP_TRY(back.finish());
        ok_pos = drow_window(in[0], uint64_t(vmax), &win.lo[0], &win.span[0]);
        ok_neg = drow_window(in[1], 0 - uint64_t(vmin), &win.lo[1], &win.span[1]);
      }
      if (!ok_pos || !ok_neg)
        return fail(FBK_E_INVALID, "distinct rows: the values " + std::to_string(vmin) + " .. " + std::to_string(vmax) +
                                       " span more than 2^23 shards of one row (not a join key); fbk_bsi_distinct returns them as a list");
    }
  }
  const uint32_t words[2] = {(win.span[0] + 63) / 64, (win.span[1] + 63) / 64};
  win.word0[0] = 0, win.word0[1] = words[0];
  const uint32_t n_words = words[0] + words[1];

  // 2. presence: one bit per (sign, shard) some position falls in
  std::vector<uint64_t> hp(n_words);
  if (n_words) {
    if (!uploaded)
      if (int32_t rc = fo.upload(ctx)) return rc;
    HIP_TRY(pres.alloc(ctx, uint64_t(n_words) * 8));
    HIP_TRY(hipMemsetAsync(pres.p, 0, uint64_t(n_words) * 8, ctx->stream));
    fo.for_each_chunk(ctx, [&](const DenseView& S, const DenseView& F, uint32_t, uint32_t ns, dim3 grid) {
      hipLaunchKernelGGL(fbk::k_drow_presence, grid, dim3(256), 0, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, bit_depth, u64(base), win, pres.as<u64>());
    });
    HIP_TRY(hipGetLastError());
    D2H back(ctx);
    HIP_TRY(back.add(hp.data(), pres.p, uint64_t(n_words) * 8));
    HIP_TRY(back.finish());
    ctx->h_stage_used = 0;  // (row lists and presence words have left the staging area)
  }

  // 3. the output rows: the set presence bits, Pos before Neg, ascending; shard -> row by the exclusive popcount prefix per word
  std::vector<uint32_t> hpre(n_words);
  uint64_t n_sign[2] = {0, 0};
  for (uint32_t sg = 0; sg < 2; ++sg)
    for (uint32_t w = 0; w < words[sg]; ++w) {
      hpre[win.word0[sg] + w] = uint32_t(n_sign[sg]);
      n_sign[sg] += uint64_t(__builtin_popcountll(hp[win.word0[sg] + w]));
    }
  const uint64_t n = n_sign[0] + n_sign[1];
  *out_n_pos = uint32_t(n_sign[0]), *out_n_neg = uint32_t(n_sign[1]);
  if (n > cap) return fail(FBK_E_CAPACITY, "distinct rows: " + std::to_string(n) + " rows, capacity " + std::to_string(cap));
  CellOutput out;  // (declared after hpre, the source of a copy: a failure drains the stream before hpre goes)
  if (int32_t rc = out.alloc(ctx, n + 1, n + 1, "distinct rows")) return rc;
  fbk_batch* o = out.batch();
  {
    uint64_t r = 0;
    for (uint32_t sg = 0; sg < 2; ++sg)
      for (uint32_t w = 0; w < words[sg]; ++w)
        for (uint64_t x = hp[win.word0[sg] + w]; x; x &= x - 1, ++r) {
          const uint64_t shard = win.lo[sg] + uint64_t(w) * 64 + uint64_t(__builtin_ctzll(x));
          out_shard_ids[r] = shard;
          for (uint64_t sl = 0; sl < uint64_t(fbk::kSlots); ++sl) o->h_keys[r * fbk::kSlots + sl] = shard * fbk::kSlots + sl;
        }
  }

  // 4. scatter, 5. the cells' descriptors, cardinalities and run counts; then the common tail of the materialising calls
  const uint32_t n_cells = uint32_t((n + 1) * fbk::kSlots);
  HIP_TRY(hipMemsetAsync(o->d_arena, 0, o->arena_bytes, ctx->stream));
  if (n) {
    HIP_TRY(pre.alloc(ctx, uint64_t(n_words) * 4));
    HIP_TRY(hipMemcpyAsync(pre.p, hpre.data(), uint64_t(n_words) * 4, hipMemcpyHostToDevice, ctx->stream));
    fo.for_each_chunk(ctx, [&](const DenseView& S, const DenseView& F, uint32_t, uint32_t ns, dim3 grid) {
      hipLaunchKernelGGL(fbk::k_drow_scatter, grid, dim3(256), 0, ctx->stream, S.arena, S.rows, F.arena, F.rows, ns, bit_depth, u64(base), win,
                         pres.as<u64>(), pre.as<uint32_t>(), uint32_t(n_sign[0]), uint32_t(n), reinterpret_cast<u64*>(o->d_arena));
    });
  }
  hipLaunchKernelGGL(fbk::k_drow_finish, dim3((n_cells + 3) / 4), dim3(256), 0, ctx->stream, o->d_arena, n_cells, o->d_slots, out.runs(), out.counts());
  if (int32_t rc = out.finish(flags, n, out_counts)) return rc;
  (void)hipStreamSynchronize(ctx->stream);  // (hpre is the source of a copy)
  *out_batch = out.release();
  return FBK_OK;
} FBK_ABI_CATCH(ctx)

}  // extern "C"
