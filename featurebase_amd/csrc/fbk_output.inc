// fbk_output.inc — the output batch of a materialising call (included by fbk.hip before the plan code): its allocation in
// "cell" layout, the arena rewrite behind optimize() and compaction, the common tail (finish_output) and CellOutput, the
// guard that owns the batch of a one-shot call until it is handed to the caller.

namespace {

void free_batch_storage(fbk_batch* b) {
  if (!b) return;
  if (b->d_arena) (void)ctx_free(b->ctx, b->d_arena);
  if (b->d_slots) (void)ctx_free(b->ctx, b->d_slots);
  if (b->d_win) (void)ctx_free(b->ctx, b->d_win);
  if (b->d_shadow_arena) (void)ctx_free(b->ctx, b->d_shadow_arena);
  if (b->d_shadow_slots) (void)ctx_free(b->ctx, b->d_shadow_slots);
  delete b;
}

// Output batch in "cell" layout: one 8 KiB bitmap cell per (row, slot).
int32_t alloc_cell_batch(fbk_ctx* ctx, uint64_t n_rows, fbk_batch** out, const char* what = "output batch") {
  const uint64_t n_slots = n_rows * fbk::kSlots;
  std::unique_ptr<fbk_batch> o(new (std::nothrow) fbk_batch());
  if (!o) return fail(FBK_E_NOMEM, "host allocation failed");
  o->ctx = ctx;
  o->n_rows = uint32_t(n_rows);
  o->arena_bytes = n_slots * 8192ull;
  o->h_slots.assign(n_slots, Slot{0, 0, 0});
  o->h_keys.assign(n_slots, 0);
  // default keys: out_row * 16 + slot, the fragment-storage form (rowID << 4 | slot) with the output
  // row ordinal standing for the row / shard id — unique and ascending in (row, slot) order, so the
  // batch serialises (fbk_batch_download_roaring); fold / shift / plans overwrite them with the keys they
  // carry through from their inputs
  for (uint64_t s = 0; s < n_slots; ++s) o->h_keys[s] = s;
  hipError_t e = ctx_malloc(ctx, reinterpret_cast<void**>(&o->d_arena), std::max<uint64_t>(o->arena_bytes, 16));
  if (e == hipSuccess) e = ctx_malloc(ctx, reinterpret_cast<void**>(&o->d_slots), std::max<uint64_t>(n_slots, 1) * sizeof(Slot));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    free_batch_storage(o.release());
    return fail(e == hipErrorOutOfMemory ? FBK_E_NOMEM : FBK_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  *out = o.release();
  return FBK_OK;
}

// The containers of `o` move into a right-sized arena: the size of every container (plan kernel), their exclusive scan, the new
// arena and descriptor table, one write per container, then the batch swaps to the new pair.
//   encode:  Container.optimize() for every 8 KiB cell (roaring.go:3412-3461); d_runs holds the run count of every cell
//            (bitmapCountRuns).
//   !encode: the containers are in their final encodings already; nothing is decoded, and nothing is done at all when the
//            copy would save less than 1 MiB.
int32_t rewrite_arena(fbk_ctx* ctx, fbk_batch* o, const uint32_t* d_runs, bool encode) {
  const std::string what = encode ? "optimize" : "compact";
  const uint64_t n_slots = uint64_t(o->n_rows) * fbk::kSlots;
  if (n_slots == 0) return FBK_OK;
  DevBuf dtype, dbytes, doff, dblk, dblkoff, dtotal;
  const uint64_t n_blk = (n_slots + 1023) / 1024;
  if (encode) HIP_TRY(dtype.alloc(ctx, n_slots * 4));
  HIP_TRY(dbytes.alloc(ctx, n_slots * 8));
  HIP_TRY(doff.alloc(ctx, n_slots * 8));
  HIP_TRY(dblk.alloc(ctx, n_blk * 8));
  HIP_TRY(dblkoff.alloc(ctx, n_blk * 8));
  HIP_TRY(dtotal.alloc(ctx, 8));
  if (encode)
    hipLaunchKernelGGL(fbk::k_encode_plan, dim3(uint32_t((n_slots + 255) / 256)), dim3(256), 0, ctx->stream, o->d_slots,
                       d_runs, n_slots, dtype.as<uint32_t>(), dbytes.as<u64>());
  else
    hipLaunchKernelGGL(fbk::k_compact_plan, dim3(uint32_t((n_slots + 255) / 256)), dim3(256), 0, ctx->stream, o->d_slots, n_slots, dbytes.as<u64>());
  hipLaunchKernelGGL(fbk::k_scan_blocks, dim3(uint32_t(n_blk)), dim3(1024), 0, ctx->stream, dbytes.as<u64>(), doff.as<u64>(), n_slots,
                     dblk.as<u64>());
  hipLaunchKernelGGL(fbk::k_exclusive_scan, dim3(1), dim3(1024), 0, ctx->stream, dblk.as<u64>(), dblkoff.as<u64>(), n_blk,
                     dtotal.as<u64>());
  HIP_TRY(hipGetLastError());
  u64 total = 0;
  HIP_TRY(hipMemcpyAsync(&total, dtotal.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!encode && total + (1u << 20) >= o->arena_bytes) return FBK_OK;  // (nothing worth a copy)
  uint8_t* d_new = nullptr;
  Slot* d_new_slots = nullptr;
  HIP_TRY(ctx_malloc(ctx, reinterpret_cast<void**>(&d_new), std::max<u64>(total, 16)));
  hipError_t e = ctx_malloc(ctx, reinterpret_cast<void**>(&d_new_slots), n_slots * sizeof(Slot));
  if (e != hipSuccess) {
    (void)ctx_free(ctx, d_new);
    return fail(FBK_E_NOMEM, what + ": slot table allocation failed");
  }
  if (encode)
    hipLaunchKernelGGL(fbk::k_encode_write, dim3(uint32_t((n_slots + 3) / 4)), dim3(256), 0, ctx->stream, o->d_slots,
                       o->d_arena, dtype.as<uint32_t>(), doff.as<u64>(), dblkoff.as<u64>(), d_runs, n_slots, d_new, d_new_slots);
  else
    hipLaunchKernelGGL(fbk::k_compact_write, dim3(uint32_t((n_slots + 3) / 4)), dim3(256), 0, ctx->stream, o->d_slots, o->d_arena, dbytes.as<u64>(), doff.as<u64>(),
                       dblkoff.as<u64>(), n_slots, d_new, d_new_slots);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)ctx_free(ctx, d_new);
    (void)ctx_free(ctx, d_new_slots);
    return fail(FBK_E_HIP, what + ": " + hipGetErrorString(e));
  }
  (void)ctx_free(o->ctx, o->d_arena);
  (void)ctx_free(o->ctx, o->d_slots);
  o->d_arena = d_new;
  o->d_slots = d_new_slots;
  o->arena_bytes = total;
  o->dense = false;
  slots_rewritten(o);
  return FBK_OK;
}

// Container.optimize() for every cell of `o`: re-encode into a right-sized arena.
int32_t optimize_cells(fbk_ctx* ctx, fbk_batch* o, const uint32_t* d_runs) { return rewrite_arena(ctx, o, d_runs, true); }

// The containers of `o` are in their final encodings but live at the head of 8 KiB cells (a kernel applied optimize() itself):
// move them into a right-sized arena.  A batch that is handed to the caller (fragment cache, long-lived rows) then holds what
// round 3's separate re-encode pass left it with, not n_rows x 16 x 8 KiB.  No-op when nothing would be saved.
int32_t compact_cells(fbk_ctx* ctx, fbk_batch* o) { return rewrite_arena(ctx, o, nullptr, false); }

// Common tail of a materialising op: optional optimize(), refresh host slots, counts D2H.
int32_t finish_output(fbk_ctx* ctx, fbk_batch* o, uint32_t flags, const uint32_t* d_runs, const u64* d_counts,
                      uint64_t n_counts, uint64_t* out_counts, bool encoded_in_cells = false) {
  HIP_TRY(hipGetLastError());
  if (out_counts && n_counts)
    HIP_TRY(hipMemcpyAsync(out_counts, d_counts, n_counts * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  slots_rewritten(o);
  if (flags & FBK_SETOP_OPTIMIZE) {
    if (int32_t rc = optimize_cells(ctx, o, d_runs)) return rc;
  } else if (encoded_in_cells && ctx->opt.setop_compact) {
    // the kernel applied optimize() itself: the caller OWNS this batch from here on, give it a right-sized arena
    if (int32_t rc = compact_cells(ctx, o)) return rc;
  }
  if (int32_t rc = refresh_slots(o)) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return FBK_OK;
}

// The output of a one-shot materialising call, owned from its allocation until release() hands it to the caller.  Leaving
// the function any other way — a failed step, an exception out of a std::vector — drains the context's stream (kernels may
// still be writing the cells, host vectors may be the sources of queued copies) and frees the batch.  Declared under the
// context's lock and after set_device, so that the destructor runs under both.  A plan's output and a prepared query's are
// owned by the plan / query, not by a guard.
struct CellOutput {
  CellOutput() = default;
  CellOutput(const CellOutput&) = delete;
  CellOutput& operator=(const CellOutput&) = delete;
  ~CellOutput() {
    if (!o) return;
    (void)hipStreamSynchronize(ctx->stream);
    free_batch_storage(o);
  }
  // n_rows rows of cells, a run count per cell and, for n_counts != 0, that many zeroed cardinalities.  `what` names the
  // call in the message of a failed scratch allocation.
  int32_t alloc(fbk_ctx* c, uint64_t n_rows, uint64_t n_counts, const char* what) {
    ctx = c;
    if (int32_t rc = alloc_cell_batch(ctx, n_rows, &o)) return rc;
    hipError_t e = druns.alloc(ctx, std::max<uint64_t>(n_rows * fbk::kSlots, 1) * 4);
    if (e == hipSuccess && n_counts) e = dcnt.alloc(ctx, n_counts * 8);
    if (e == hipSuccess && n_counts) e = hipMemsetAsync(dcnt.p, 0, n_counts * 8, ctx->stream);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(e == hipErrorOutOfMemory ? FBK_E_NOMEM : FBK_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    return FBK_OK;
  }
  fbk_batch* batch() const { return o; }
  uint32_t* runs() { return druns.as<uint32_t>(); }
  u64* counts() { return dcnt.as<u64>(); }
  // finish_output; the first n_counts cardinalities go to out_counts (when that is not NULL)
  int32_t finish(uint32_t flags, uint64_t n_counts, uint64_t* out_counts, bool encoded_in_cells = false) {
    return finish_output(ctx, o, flags, runs(), counts(), n_counts, out_counts, encoded_in_cells);
  }
  // optimize() asked for: does the kernel apply it itself (option setop_direct_encode = 2; otherwise the separate re-encode
  // pass)?  The answer is the kernel's encode argument, and finish(n_counts, out_counts) goes by it.
  bool kernel_encodes(uint32_t flags) {
    enc = (flags & FBK_SETOP_OPTIMIZE) && ctx->opt.setop_direct_encode == 2;
    fin_flags = enc ? flags & ~uint32_t(FBK_SETOP_OPTIMIZE) : flags;
    return enc;
  }
  int32_t finish(uint64_t n_counts, uint64_t* out_counts) { return finish(fin_flags, n_counts, out_counts, enc); }
  fbk_batch* release() {
    fbk_batch* b = o;
    o = nullptr;
    return b;
  }

 private:
  fbk_ctx* ctx = nullptr;
  fbk_batch* o = nullptr;
  uint32_t fin_flags = 0;
  bool enc = false;
  DevBuf druns, dcnt;  // (freed after the destructor's drain)
};

}  // namespace
