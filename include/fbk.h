/*
 * fbk.h — C ABI of the MI355X roaring-bitmap execution kernel ("fbk" = FeatureBase
 * Kernel).  This is the drop-in boundary for ONE hot path of FeatureBase: the
 * Intersect / Union / Difference / Xor / Count / IntersectionCount loop that the
 * reference runs container-by-container on the CPU in Go.
 *
 * The reference has no FFI for this path (CGO_ENABLED=0, Makefile:34); the narrowest
 * Go choke points each entry point replaces are cited per function below as
 * <file>:<line> relative to the FeatureBase tree.  INTEGRATION.md shows the cgo stub a
 * maintainer would add on the Go side.
 *
 * Conventions
 *   - C linkage, plain pointers and sizes, no exceptions across the boundary: every entry point is a function-try-block
 *     (a host allocation that fails inside the library comes back as FBK_E_NOMEM, anything else a C++ library could throw
 *     as FBK_E_HIP with the message; tests/test_abi.py checks that no definition is left unwrapped).
 *   - Every function returns an int32 status: FBK_OK (0) or a negative FBK_E_* code;
 *     fbk_last_error_r(ctx, ...) returns the context's human readable message (see below).
 *     (roaring set-ops never return errors in Go — invariant breaks panic,
 *     roaring/roaring.go:976,3524 — so every error here is an argument/resource error.)
 *   - The caller owns every input buffer for the duration of the call only: the
 *     library copies/uploads before returning, which matches the lifetime rule of
 *     mmapped containers ("must not retain", roaring/filter.go:179-181, tx.go:66-72).
 *   - Handles (fbk_ctx, fbk_batch) are opaque; one fbk_ctx drives ONE GPU.  A process
 *     that owns several GPUs opens a group (fbk_group_open: one member context per device,
 *     shards partitioned over the members as executor.go:6579 `mapper` partitions shards
 *     over nodes, partial counts reduced inside the library); one process per GPU with
 *     torch.distributed / RCCL above the ABI is the other supported deployment.
 *   - Thread safety: calls on one context are serialised by an internal mutex (cgo pins
 *     one OS thread per call).  Concurrent callers that should overlap on the device
 *     (~NumCPU goroutines, executor.go:6723-6737) each use their own fbk_ctx_fork.
 *   - There is NO CPU fallback: if no gfx950 device is usable, fbk_open fails.
 *
 * Data model (modelled on roaring/containers_slice.go:5-10 — sorted keys + containers —
 * flattened to SoA descriptors over one payload arena):
 *   A *batch* is a set of *rows*.  A row is what fragment.row() returns
 *   (fragment.go:283-333): the <=16 containers of one (fragment,rowID) in one shard,
 *   ShardWidth = 2^20 columns = 16 containers of 2^16 bits (shardwidth/helper.go:14,
 *   fragment.go:47).  Container `key & 15` is the slot inside the row; the library never
 *   interprets the high key bits, it only carries them through to download.
 *   Payload encodings are byte-identical to what arrayWriteTo / bitmapWriteTo /
 *   runWriteTo emit (roaring/roaring.go:4068-4108) minus the 2-byte run-count prefix:
 *     array : len x uint16 ascending
 *     bitmap: 1024 x uint64 little endian, bit v at word v/64, bit v%64
 *     run   : len x {uint16 start, uint16 last}, inclusive, ascending, non-overlapping
 */
#ifndef FBK_H
#define FBK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBK_ABI_VERSION 6
/* ABI history.
 *   6 (round 6): + fbk_comm_unique_id / fbk_comm_init / fbk_comm_all_reduce_u64 / fbk_comm_fence / fbk_comm_close (the
 *      one-process-per-GPU exchange issued by the library itself).  fbk_batch_compact refuses a batch of another context;
 *      fbk_group_topn refuses members whose topn_semantics differ.  Later, entry points added at the same version:
 *      fbk_count_matrix_distinct; fbk_count_matrix_select / fbk_count_cube_select / fbk_count_matrix_sum_select / fbk_select_groups;
 *      fbk_extract_open / _span / _columns / _bsi / _rows / _free; fbk_bsi_sort;
 *      fbk_extract_open_columns; fbk_bsi_quantiles; fbk_bsi_percentile; fbk_bsi_distinct_rows;
 *      fbk_expr_count / fbk_expr_eval / fbk_query_expr; fbk_expr_bsi_agg / fbk_query_expr_bsi; fbk_expr_row_counts / fbk_expr_topk /
 *      fbk_expr_topn.
 *   5 (round 5): + fbk_topn_partials, options topn_semantics, matrix_shadow_arena_x.  CHANGED: fbk_topn / fbk_query_topn /
 *      fbk_group_topn with 0 < n < n_a return the reference's two-pass answer by default (topn_semantics = 1; = 0 restores
 *      round 4's exact top n of fbk_topn; round 4's per-member candidate rule of fbk_group_topn is gone — it was neither);
 *      count_range_reference_quirk defaults to 1 (the reference's number).
 *   4 (round 4): + fbk_query_bsi_range / _fold / _topn / _output, fbk_group_bsi_sum / _topn.  Also changed in that round
 *      (not said at the time): option pair_spw REMOVED (fbk_set_option fails, FBK_PAIR_SPW is ignored); pair_wpb accepts
 *      0 / 1 / 4 only; the default of matrix_shadow_max_mb went from 65536 to 16384; fbk_plan_setop(FBK_SETOP_OPTIMIZE)
 *      succeeds (when setop_direct_encode == 2) where it was an error.
 *
 * Where the DEFAULT deliberately differs from the reference, and the option that restores identity:
 *   (none since ABI 5.)  Before: CountRange on runs ending at `end` (count_range_reference_quirk = 1), TopN with n > 0
 *   (topn_semantics = 1).  What remains different cannot be restored by an option because the reference itself leaves it
 *   unspecified or depends on state off the path: the order of TopN pairs of EQUAL count (Go's unstable sort over map
 *   order; here row index ascending) and the rank cache's size / staleness (cache.go: at most CacheSize rows, refreshed
 *   lazily; here every row of the field is ranked, as after RecalculateCaches with CacheSize >= the field's rows). */

/* status codes */
#define FBK_OK 0
#define FBK_E_INVALID (-1)   /* bad argument / malformed container */
#define FBK_E_NODEVICE (-2)  /* no usable gfx950 device */
#define FBK_E_HIP (-3)       /* HIP runtime error (message has hipGetErrorString) */
#define FBK_E_NOMEM (-4)     /* host or device allocation failed */
#define FBK_E_CAPACITY (-5)  /* caller-provided output buffer too small */
#define FBK_E_NOTFOUND (-6)  /* cache miss (absent or stale entry) */

/* container type codes — identical to roaring/roaring.go:53-58 */
#define FBK_TYPE_NIL 0
#define FBK_TYPE_ARRAY 1
#define FBK_TYPE_BITMAP 2
#define FBK_TYPE_RUN 3

/* set operations: intersect (roaring.go:4753), union (:4980), xor (:6052),
 * difference a\b (:5692) */
#define FBK_OP_AND 0
#define FBK_OP_OR 1
#define FBK_OP_XOR 2
#define FBK_OP_ANDNOT 3

#define FBK_SLOTS_PER_ROW 16      /* containers per shard row, fragment.go:47 */
#define FBK_BITMAP_WORDS 1024     /* bitmapN, roaring.go:44 */
#define FBK_CONTAINER_BITS 65536

/* fbk_setop flags */
#define FBK_SETOP_KEEP_BITMAP 0u  /* every non-empty output container is a bitmap */
#define FBK_SETOP_OPTIMIZE 1u     /* re-encode outputs with Container.optimize() rules
                                     (roaring.go:3412-3461): run if runs<=2048 && runs<=n/2,
                                     else array if n<4096, else bitmap */

typedef struct fbk_ctx fbk_ctx;
typedef struct fbk_batch fbk_batch;

/* One container of a batch.  Replaces *roaring.Container (container_stash.go:46-53). */
typedef struct fbk_container_desc {
  uint64_t key;  /* roaring container key; slot = key & 15 */
  uint64_t off;  /* byte offset of the payload inside `payload` */
  uint32_t row;  /* batch-local row ordinal, 0 <= row < n_rows */
  uint32_t len;  /* array: #uint16; bitmap: 1024; run: #intervals */
  int32_t n;     /* cardinality (Container.N, container_stash.go:430); -1 = recount on device */
  uint8_t type;  /* FBK_TYPE_* */
  uint8_t pad[3];
} fbk_container_desc;

/* ---- lifetime ---------------------------------------------------------------- */

/* Number of visible HIP devices. */
int32_t fbk_device_count(int32_t* out_n);

/* Open a context on HIP device `device`.  Replaces nothing in Go; called at server
 * start (server/server.go Open). */
int32_t fbk_open(int32_t device, uint32_t flags, fbk_ctx** out_ctx);
int32_t fbk_close(fbk_ctx* ctx);

/* Message of the last failing call (never NULL).
 *   ctx == NULL : the calling THREAD's last failure (the only source for failures that have no
 *                 context yet: fbk_open, fbk_device_count, fbk_rbf_find_root).
 *   ctx != NULL : the CONTEXT's last failure, copied into a buffer owned by the calling thread (valid
 *                 until that thread's next call into the library).
 * fbk_last_error_r copies the context's message (and its status code) into a caller buffer — the
 * form a cgo binding must use: a goroutine can be rescheduled onto another OS thread between the
 * failing call and the call that fetches the message, so nothing thread-local is reliable there.
 * Semantics are sqlite3_errmsg's: with several callers failing concurrently on ONE context the
 * message is that of the most recent failure; callers that need their own message use their own
 * forked context (fbk_ctx_fork). */
const char* fbk_last_error(fbk_ctx* ctx);
int32_t fbk_last_error_r(fbk_ctx* ctx, char* buf, uint64_t cap, int32_t* out_code);

/* A second context on the same device for another calling thread: its own stream, lock, staging
 * area and memory pool, so that concurrent callers overlap on the device instead of serialising on
 * one context mutex — the analogue of the reference's pool of ~NumCPU shard workers
 * (executor.go:6723-6737).  Batches are read-only once uploaded and may be used through any context
 * of the same device; the fragment cache (fbk_cache_*) is shared with the root context.  A fork is
 * closed with fbk_close, before its root. */
int32_t fbk_ctx_fork(fbk_ctx* ctx, fbk_ctx** out_child);

/* Options (22; round 5 removed fifteen A/B switches together with the kernels and paths that had lost their comparison —
 * DESIGN.md section 4 lists them).  The environment variables FBK_<NAME> are read ONCE, by fbk_open; afterwards only these
 * calls change an option.
 *   semantics (DEFAULT 1 = the reference's result, 0 = the arithmetically exact one; see fbk_count_range, fbk_topn):
 *     count_range_reference_quirk, topn_semantics;
 *   memory: matrix_shadow (1: the count matrix over encoded rows reads run containers of more than matrix_shadow_run runs and
 *     arrays of more than matrix_shadow_array values through dense shadows built per batch on first use — up to matrix_shadow_max_mb of device
 *     memory per batch and matrix_shadow_arena_x times its own arena (0: no such rule), fbk_batch_memory reports what a batch
 *     got; 0: every container is decoded in every query), setop_compact (fbk_batch_compact applied to the outputs of one-shot
 *     calls with FBK_SETOP_OPTIMIZE), matrix_pass_kb (per-shard matrices are produced in passes of at most this size),
 *     upload_chunk_mb, upload_threads (the pinned staging buffers of the uploads and the host threads that fill them);
 *   measurement: time_kernels = 1 makes the query-level calls (count matrix, n-way fold, BSI range / sum / min / max) record
 *     HIP events on the context's stream right before and after their dominant kernel; fbk_get_option("last_kernel_ns")
 *     then returns that kernel's duration for the last such call;
 *   kernel selection, each a choice the library makes by itself (the default) that a test or a measurement can pin — BOTH
 *     sides are product paths, chosen by the shape of the call or of the rows: dense_spb and matrix_spb (container slots per
 *     block of the dense count / the count matrices), matrix_tickets (dense single-tile count matrix: 1 its blocks take their units
 *     from a ticket counter, long units first — the device's XCDs run at different paces; 0 by block id), matrix_fused (encoded rows: -1 by the matrix size, 1 the matrix-core
 *     kernel that decodes the rows in place, 0 the generic pair kernel), matrix_fp4 (dense count matrix on the FP4 matrix
 *     instruction: -1 for matrices of several tiles), topk_device_sort (-1 by the field size), pair_kernels (0 by the rows'
 *     payload: the round-2 kernels for tiny containers, the table + probe kernels otherwise), pair_wpb (their waves per
 *     block: 0 by the rows' payload), setop_direct_encode (pair set-ops with FBK_SETOP_OPTIMIZE: 2 Container.optimize() inside
 *     the kernel; 1 / 0 bitmap or small-array cells and a separate re-encode pass — the byte-for-byte cross-check of the
 *     in-kernel encoders, and what a plan's launch-only form refuses).
 * Every value of every kernel-selection option gives the same results (the tests run them against each other). */
int32_t fbk_set_option(fbk_ctx* ctx, const char* name, int64_t value);
int32_t fbk_get_option(fbk_ctx* ctx, const char* name, int64_t* out_value);

int32_t fbk_abi_version(void);

/* Use an externally owned hipStream_t (e.g. the caller's framework stream) for all
 * subsequent launches on this context; NULL restores the context's own stream. */
int32_t fbk_set_stream(fbk_ctx* ctx, void* hip_stream);

/* Block until everything enqueued on the context's stream has finished. */
int32_t fbk_synchronize(fbk_ctx* ctx);

/* ---- residency ----------------------------------------------------------------
 * fbk_batch_upload makes the rows a query touches device resident.  Replaces the
 * per-row materialisation fragment.row / rowFromStorage (fragment.go:283-333) ->
 * Tx.OffsetRange (rbf/tx.go:1586-1638).  `descs` may be in any order; (row, key&15)
 * must be unique.  Containers with n == 0 are legal and stored as nil (the reference
 * stores empty results as nil, roaring.go:751-752). */
int32_t fbk_batch_upload(fbk_ctx* ctx, const fbk_container_desc* descs, uint64_t n_desc,
                         uint32_t n_rows, const void* payload, uint64_t payload_len,
                         fbk_batch** out_batch);

/* Dense upload: n_rows rows of 16 bitmap containers each, `words` = n_rows*16*1024
 * uint64 (row-major).  Cardinalities are recounted on the device (the analogue of
 * bitmapRepair, roaring.go:4193-4206).  Keys are assigned row*16+slot.  `words` may also be a
 * DEVICE pointer on the context's device (rows a device-side decode produced, or a benchmark's
 * on-device generator): the copy is then device to device. */
int32_t fbk_batch_upload_dense(fbk_ctx* ctx, const uint64_t* words, uint32_t n_rows,
                               fbk_batch** out_batch);

int32_t fbk_batch_free(fbk_ctx* ctx, fbk_batch* batch);

/* Device memory a batch holds: its arena, its heavy-row shadows (option matrix_shadow; built on the first count matrix
 * over encoded rows that reads the batch) and the shadow state — 0 not looked at yet, 1 shadowed, 2 nothing heavy or over a
 * limit (matrix_shadow_max_mb of device memory; matrix_shadow_arena_x times the batch's own arena; a quarter of the free
 * device memory): the batch's containers are then decoded in every query. */
int32_t fbk_batch_memory(fbk_ctx* ctx, const fbk_batch* batch, uint64_t* out_arena_bytes, uint64_t* out_shadow_bytes,
                         int32_t* out_shadow_state);

/* Move the containers of a batch the caller owns into a right-sized arena.  Materialising calls with FBK_SETOP_OPTIMIZE apply
 * Container.optimize() inside their kernel, which writes the encoded bytes into the head of an 8 KiB cell per container
 * (arena = n_rows x 16 x 8 KiB); the one-shot calls (fbk_setop, fbk_fold_n / fbk_union_n, fbk_bsi_range*, fbk_flip,
 * fbk_shift) compact their output before returning it (option setop_compact = 1, the default: payload sizes, one scan, one
 * copy per container — nothing is decoded), so a caller that keeps results holds their encoded size.  Outputs of plans and
 * prepared queries (fbk_plan_output, fbk_query_output) are BORROWED and keep the 8 KiB stride — their next run rewrites
 * them in place — and this call refuses them; copy them out (download, or a one-shot call) to keep them.
 * *out_arena_bytes = the arena size afterwards (also what fbk_batch_memory reports). */
int32_t fbk_batch_compact(fbk_ctx* ctx, fbk_batch* batch, uint64_t* out_arena_bytes);

/* Sizes needed to download a batch. */
int32_t fbk_batch_info(fbk_ctx* ctx, const fbk_batch* batch, uint32_t* n_rows,
                       uint64_t* n_containers, uint64_t* payload_bytes);

/* Copy a batch back to the host in the same flattened layout (non-nil containers only,
 * sorted by (row, slot)).  The Go side rebuilds containers with
 * NewContainerArray/BitmapN/RunN (container_stash.go).  Replaces result Row
 * construction (row.go:561-610). */
int32_t fbk_batch_download(fbk_ctx* ctx, const fbk_batch* batch, fbk_container_desc* descs_out,
                           uint64_t descs_cap, void* payload_out, uint64_t payload_cap);

/* ---- serialised roaring (the reference's interchange format) ------------------------------
 * fbk_batch_upload_roaring makes the containers of ONE serialised bitmap device resident:
 * either the Pilosa format Bitmap.WriteTo emits (roaring.go:1730-1817: cookie 12348, 12-byte
 * {key u64, type u16, N-1 u16} headers, u32 offsets, payloads with a u16 count prefix on run
 * containers, :4054-4108) or the official RoaringBitmap format (cookies 12346 / 12347,
 * readOfficialHeader roaring.go:6948-7006, runs stored {start, length-1} and converted on
 * read, :2239-2247).  It replaces Bitmap.UnmarshalBinary / NewRoaringIterator
 * (roaring.go:1945-2262) + the per-container copy into fragment storage
 * (ImportRoaringBits, fragment.go:2038-2165): the blob crosses PCIe once and is unpacked by a
 * device kernel.  Batch row i holds the containers whose key >> 4 equals out_row_ids[i]
 * (ascending; for fragment storage that is the row ID, for a serialised Row the shard number);
 * slot = key & 15.  out_row_ids may be NULL; *out_n_rows is always set.
 * An ops log behind the containers of a Pilosa-format FILE image is replayed as
 * Bitmap.UnmarshalBinary does (unmarshal_binary.go:66-95; op layout and FNV-1a checksum
 * roaring.go:6325-6431): every op's checksum is verified on the host, consecutive add / remove /
 * addN / removeN ops collapse to the last op per position and are applied as one union and one
 * difference on the device, addRoaring / removeRoaring ops upload their nested image from the
 * same blob and fold it in; the containers that come out are Optimize()d.  The row list then
 * also names every row an op touches (such a row may end up empty).  A truncated or corrupt op
 * is FBK_E_INVALID (the reference's FileShouldBeTruncatedError), nothing is uploaded. */
int32_t fbk_batch_upload_roaring(fbk_ctx* ctx, const void* data, uint64_t len, fbk_batch** out_batch,
                                 uint64_t* out_row_ids, uint32_t row_cap, uint32_t* out_n_rows);

/* RBF, the reference's storage file (rbf/rbf.go): make the containers of ONE bitmap b-tree
 * (one fragment: index/field/view/shard, rbf.go rbfName) device resident straight from the file
 * image.  `file` is the database file (or mmap) from page 0; `root_pgno` the bitmap's root page
 * (fbk_rbf_find_root resolves a name through the root records, rbf.go:222-255).  The host walks
 * branch pages and reads cell headers (rbf.go:488-520, 616-626); array / RLE cell payloads and
 * the 8 KiB pages that BitmapPtr cells point to are moved into the arena by the device unpack
 * kernel after ONE H2D copy of the file image.  Replaces Tx.ContainerIterator / OffsetRange ->
 * cursor -> toContainer (rbf/tx.go:1333, 1586-1638, rbf/cursorx.go:230-266).  Row mapping as
 * fbk_batch_upload_roaring: batch row i holds keys with key >> 4 == out_row_ids[i]. */
int32_t fbk_rbf_find_root(const void* file, uint64_t len, const char* name, uint32_t* out_pgno);
int32_t fbk_batch_upload_rbf(fbk_ctx* ctx, const void* file, uint64_t len, uint32_t root_pgno, fbk_batch** out_batch,
                             uint64_t* out_row_ids, uint32_t row_cap, uint32_t* out_n_rows);

/* Serialise a batch in the Pilosa format (what Bitmap.WriteTo / writeToUnoptimized write,
 * roaring.go:1730-1817): non-empty containers in (row, slot) order, whose keys must be
 * strictly ascending.  Containers are written in their current encoding — WriteTo runs
 * Optimize() first, so produce the batch with FBK_SETOP_OPTIMIZE to get byte-identical
 * output.  fbk_batch_roaring_size reports the bytes needed. */
int32_t fbk_batch_roaring_size(fbk_ctx* ctx, const fbk_batch* batch, uint64_t* out_bytes);
int32_t fbk_batch_download_roaring(fbk_ctx* ctx, const fbk_batch* batch, void* out, uint64_t cap, uint64_t* out_len);

/* ---- device fragment cache ----------------------------------------------------------------
 * The reference re-materialises a row from storage on every use (fragment.row,
 * fragment.go:283-333; zero-copy views of mmapped pages valid inside one Tx,
 * rbf/cursorx.go:243-247).  On the GPU the steady state keeps a fragment's rows resident:
 * entries are keyed by the reference's fragment identity ("index/field/view/shard", the RBF
 * bitmap name) and carry a version the host bumps whenever the fragment is written (every
 * write path of fragment.go ends in one Tx commit), so a stale entry is a miss.
 *   put        hands a batch (and the row ids fbk_batch_upload_rbf/_roaring returned) to the
 *              cache, which now owns it; an existing entry under the key is replaced.
 *   get        FBK_OK + the batch pinned for the caller, or FBK_E_NOTFOUND (absent / other
 *              version; a stale entry is dropped).  The pointers stay valid until release.
 *   release    unpins; invalidated or evicted entries are freed at their last release.
 *   invalidate drops every entry whose key starts with key_prefix ("" = everything).
 *   configure  sets the byte budget (default 128 GiB of the 288 GB HBM); least recently used
 *              unpinned entries are evicted beyond it. */
int32_t fbk_cache_put(fbk_ctx* ctx, const char* key, uint64_t version, fbk_batch* batch, const uint64_t* row_ids,
                      uint32_t n_row_ids);
int32_t fbk_cache_get(fbk_ctx* ctx, const char* key, uint64_t version, const fbk_batch** out_batch,
                      const uint64_t** out_row_ids, uint32_t* out_n_row_ids);
int32_t fbk_cache_release(fbk_ctx* ctx, const fbk_batch* batch);
int32_t fbk_cache_invalidate(fbk_ctx* ctx, const char* key_prefix, uint32_t* out_dropped);
int32_t fbk_cache_configure(fbk_ctx* ctx, uint64_t cap_bytes);
int32_t fbk_cache_stats(fbk_ctx* ctx, uint64_t* entries, uint64_t* bytes, uint64_t* hits, uint64_t* misses,
                        uint64_t* evictions);

/* ---- counts -------------------------------------------------------------------- */

/* out[i] = Row.Count of rows[i]: sum of stored container N (roaring.go:542,
 * containers_slice.go:120-126, row.go:446). */
int32_t fbk_count(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n,
                  uint64_t* out_counts);

/* out[i] = number of bits of rows[i] in [start, end), positions relative to the row
 * (0 <= start <= end <= 2^20).  Replaces Bitmap.CountRange (roaring.go:573-615) ->
 * Container.countRange -> ArrayCountRange / BitmapCountRange / RunCountRange
 * (roaring.go:3074-3232), which fragment.go:237,396,444 use to count one row of a fragment.
 * The device counts bits; this equals the reference everywhere except on run containers that
 * hold a run whose last value == end-1+1 (`iv.Last == end`), where RunCountRange's
 * "subset of range" and "overlaps end" branches both fire and over-count (roaring.go:3216-3227)
 * — a case the reference's own callers (container-aligned ranges) never produce.
 * DEFAULT (option "count_range_reference_quirk" = 1): RunCountRange as written, over-count included — the
 * reference's number on the same inputs.  = 0 (fbk_set_option, or FBK_COUNT_RANGE_REFERENCE_QUIRK=0 in the
 * environment of fbk_open): the bit count.  Both modes are tested against the oracle (tests/test_gpu_parity.py). */
int32_t fbk_count_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n, uint64_t start,
                        uint64_t end, uint64_t* out_counts);

/* out[i] = |A.rows_a[i] ∩ B.rows_b[i]| without materialising.  Replaces
 * RowSegment.IntersectionCount (row.go:556) -> Bitmap.IntersectionCount
 * (roaring.go:711-733) -> intersectionCount (roaring.go:4477-4614), one call per
 * (query,node) instead of one per container.  a and b may be the same batch. */
int32_t fbk_intersection_count(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a,
                               const fbk_batch* b, const uint32_t* rows_b, uint64_t n_pairs,
                               uint64_t* out_counts);

/* ---- materialising set operations ---------------------------------------------- */

/* out row i = A.rows_a[i] <op> B.rows_b[i]; out_counts[i] (may be NULL) = its cardinality.
 * Replaces RowSegment.{Intersect,Union,Difference,Xor} (row.go:561-610) ->
 * Bitmap.{Intersect,Union,Difference,Xor} (roaring.go:736,1272,1564,1598).  The
 * cardinality is produced in the same pass, as the reference fuses it
 * (roaring.go:4971-4974).  Output keys are taken from operand A (or B where A's slot
 * is nil). */
int32_t fbk_setop(fbk_ctx* ctx, int32_t op, const fbk_batch* a, const uint32_t* rows_a,
                  const fbk_batch* b, const uint32_t* rows_b, uint64_t n_pairs, uint32_t flags,
                  fbk_batch** out_batch, uint64_t* out_counts);

/* ---- plans: launch-only hot path -------------------------------------------------
 * A plan is a prepared list of row pairs whose index arrays and result buffers are
 * device resident, so one step of the hot path is kernel launches only (no host
 * allocation, copy or synchronisation).  It is what ONE batch call per (query, node)
 * from mapperLocal (executor.go:6742-6790) becomes: the per-shard mapFn closure
 * (executor.go:5871) is the pair list, the reduceFn (executor.go:5880) is
 * fbk_plan_total.  `device_counts_or_null`, when given, is a caller-owned device buffer
 * of n_pairs uint64 (e.g. the tensor a collective library will all-reduce). */
typedef struct fbk_plan fbk_plan;

int32_t fbk_plan_create(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, const fbk_batch* b,
                        const uint32_t* rows_b, uint64_t n_pairs, void* device_counts_or_null,
                        fbk_plan** out_plan);
int32_t fbk_plan_free(fbk_ctx* ctx, fbk_plan* plan);

/* Enqueue counts[i] = |A.rows_a[i] ∩ B.rows_b[i]| (Bitmap.IntersectionCount,
 * roaring.go:711-733).  Asynchronous. */
int32_t fbk_plan_intersection_count(fbk_ctx* ctx, fbk_plan* plan);

/* fbk_plan_intersection_count + fbk_plan_total in ONE launch: the per-node sum is fused into
 * the counting kernel (its last block to finish adds up the per-pair counts), i.e. one step of
 * Count(Intersect(Row, Row)) over all local shards — mapFn and reduceFn of executeCount,
 * executor.go:5871-5880 — is a single kernel.  Asynchronous. */
int32_t fbk_plan_intersection_count_total(fbk_ctx* ctx, fbk_plan* plan, void* device_total_or_null);

/* The same counts, with the per-node reduce done by accumulation: every workgroup adds its count
 * to *device_accum (device memory, uint64), which the CALLER has zeroed — e.g. one slot of a
 * vector that is cleared once per N steps, or of an all-reduce bucket.  One launch and nothing
 * serial behind the last workgroup (fbk_plan_intersection_count_total pays ~3 us for its final
 * pass, fbk_plan_intersection_count + fbk_plan_total ~2 us for the second launch). */
int32_t fbk_plan_intersection_count_accumulate(fbk_ctx* ctx, fbk_plan* plan, void* device_accum);

/* Enqueue out row i = A.rows_a[i] <op> B.rows_b[i] and counts[i] = its cardinality
 * (Bitmap.Intersect/Union/Xor/Difference + Count, roaring.go:736,1272,1598,1564;
 * executeCount's mapFn, executor.go:5871-5876).  The output batch is owned by the plan
 * and overwritten by the next enqueue.  Asynchronous.  flags = FBK_SETOP_OPTIMIZE (round 4): the
 * kernel applies Container.optimize() itself and writes the encoded container into the head of each
 * result cell — still launch-only (option setop_direct_encode = 2, the default; with 0 / 1 the
 * re-encode is a separate pass that sizes its output on the host, which only fbk_setop can run). */
int32_t fbk_plan_setop(fbk_ctx* ctx, fbk_plan* plan, int32_t op, uint32_t flags);

/* Enqueue total = sum_i counts[i] (executeCount reduceFn, executor.go:5880) into the
 * plan's total cell or into a caller-owned device uint64.  Asynchronous. */
int32_t fbk_plan_total(fbk_ctx* ctx, fbk_plan* plan, void* device_total_or_null);

/* Synchronise and copy counts (n_pairs, may be NULL) and total (may be NULL) to the host. */
int32_t fbk_plan_read(fbk_ctx* ctx, fbk_plan* plan, uint64_t* out_counts, uint64_t* out_total);

/* Borrow / take ownership of the plan's set-op output batch. */
int32_t fbk_plan_output(fbk_ctx* ctx, fbk_plan* plan, fbk_batch** out_batch);
int32_t fbk_plan_detach_output(fbk_ctx* ctx, fbk_plan* plan, fbk_batch** out_batch);

/* ---- prepared queries: the launch-only form of the query-level calls -------------------------
 * fbk_plan_* above makes the PAIR operations launch-only.  A prepared query does the same for the
 * GroupBy / TopK count matrix (fbk_count_matrix), the n-way fold with its fused count
 * (fbk_fold_n_intersection_count / fbk_union_n_intersection_count) and BSI Sum / the one-pass
 * Sum(Range) (fbk_bsi_sum, fbk_bsi_range_sum): the row lists are validated and uploaded ONCE, the
 * result buffers live on the device, and every execution is memset + kernel(s) on the context's
 * stream — no allocation, no host<->device copy, no synchronisation.  It is what one (query, node)
 * call of mapperLocal (executor.go:6742) becomes when the same query shape runs again on resident
 * fragments, and it leaves the partial result where the multi-GPU reduce wants it (the cell of an
 * all-reduce).  The batches a query was prepared on must outlive it and must not be rewritten; calls on
 * one query are serialised by its context's mutex (run and read from different threads are safe, the
 * read returns the result of whichever run was enqueued last).
 *
 *   fbk_query_count_matrix              arguments as fbk_count_matrix; keep_per_shard != 0 keeps the
 *                                       per-shard matrices readable (fbk_query_read's out1)
 *   fbk_query_fold_intersection_count   arguments as fbk_fold_n_intersection_count
 *   fbk_query_bsi_sum                   op == 0: fbk_bsi_sum; op = FBK_BSI_*: fbk_bsi_range_sum in one
 *                                       pass (FBK_E_INVALID for the predicates only the two-pass form serves)
 *   fbk_query_run(q, device_out, flags) enqueue one execution.  device_out == NULL: the query's own
 *                                       result buffer; otherwise a caller-owned device buffer of the
 *                                       result's size (count matrix: n_a * n_b uint64; fold: n_groups
 *                                       uint64).  FBK_QUERY_ACCUMULATE adds to what the buffer holds
 *                                       instead of overwriting it (count-valued kinds only).
 *   fbk_query_result                    the query's own device result buffer and its size in bytes
 *   fbk_query_read(q, out0, out1)       synchronise; copy the last run's result to the host:
 *                                       count matrix: out0 = total [n_a * n_b] uint64, out1 = per-shard
 *                                       [n_shards][n_a * n_b] (or NULL); fold: out0 = counts [n_groups];
 *                                       BSI: out0 = int64 sums [n_shards], out1 = uint64 counts [n_shards].
 *
 * Queries with a ROW result keep the rows on the device too (round 4: the one-shot forms paid 40-80 us of
 * host work around a 130 us kernel for allocating the output batch, uploading the plane program and
 * downloading descriptors that nobody reads when the rows only feed the next operator):
 *   fbk_query_bsi_range                 Row(v op predicate), fragment.rangeOp (fragment.go:937-1303), arguments
 *                                       as fbk_bsi_range (8 KiB cells).  run = memset + k_bsi_range_slot;
 *                                       read: out0 = uint64 cardinalities [n_shards]
 *   fbk_query_fold                      the materialised n-way fold of any of the four operations (fbk_fold_n; flags =
 *                                       FBK_SETOP_OPTIMIZE: Container.optimize() in the kernel's epilogue).
 *                                       run = memset + ONE launch; read: out0 = uint64 cardinalities [n_groups]
 *   fbk_query_output(q, &batch)         the output batch of the last run, BORROWED: owned by the query, rewritten
 *                                       by its next run, freed with it.  A valid operand of any later call on the
 *                                       same context (the filter of fbk_bsi_sum / fbk_query_bsi_sum, a plan's row).
 *   fbk_query_topn                      fbk_topn with the per-shard counts, the totals AND the ordering (device
 *                                       radix sort, scratch sized at prepare) launch-only; read: out0 = uint32
 *                                       {number of results r, r row indexes} (capacity 1 + min(n, n_a), n = 0:
 *                                       1 + n_a), out1 = uint64 counts [r].  device_out must be NULL. */
typedef struct fbk_query fbk_query;
#define FBK_QUERY_ACCUMULATE 1u
int32_t fbk_query_count_matrix(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                               const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                               uint32_t n_shards, uint32_t keep_per_shard, fbk_query** out_query);
int32_t fbk_query_fold_intersection_count(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups,
                                          uint32_t k, const fbk_batch* filter, const uint32_t* rows_f, fbk_query** out_query);
int32_t fbk_query_bsi_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, uint32_t bit_depth,
                          int32_t op, int64_t predicate, const fbk_batch* filter, const uint32_t* rows_f, fbk_query** out_query);
int32_t fbk_query_bsi_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op,
                            uint32_t bit_depth, int64_t predicate, fbk_query** out_query);
int32_t fbk_query_fold(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups, uint32_t k,
                       uint32_t flags, fbk_query** out_query);
int32_t fbk_query_topn(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter,
                       const uint32_t* rows_f, uint32_t n_shards, uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold,
                       fbk_query** out_query);
int32_t fbk_query_output(fbk_ctx* ctx, fbk_query* query, fbk_batch** out_batch);
int32_t fbk_query_run(fbk_ctx* ctx, fbk_query* query, void* device_out, uint32_t flags);
int32_t fbk_query_result(fbk_ctx* ctx, fbk_query* query, void** out_device_ptr, uint64_t* out_bytes);
int32_t fbk_query_read(fbk_ctx* ctx, fbk_query* query, void* out0, void* out1);
int32_t fbk_query_free(fbk_ctx* ctx, fbk_query* query);

/* ---- n-way union ---------------------------------------------------------------------
 * rows holds n_groups groups of k row ordinals (group g = rows[g*k .. g*k+k)); out row g
 * is the union of the group's rows, out_counts[g] its cardinality.  Replaces
 * Row.Union(others...) (row.go:288) -> RowSegment.Union (:572) -> the n-way
 * Bitmap.unionInPlace (roaring.go:1410-1561) and the streaming BitmapRowsUnion used by
 * UnionRows (roaring/filter.go:294-366, fragment.go:2489): the accumulation happens in
 * registers, the union is written once. */
int32_t fbk_union_n(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups,
                    uint32_t k, uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts);

/* Fused Union-of-k-rows then IntersectionCount against a filter row, without ever
 * materialising the union: out_counts[g] = |(∪ group g) ∩ filter.rows_f[g]|
 * (filter == NULL: |∪ group g|).  executor.go:5382 executeUnionShard followed by
 * Row.intersectionCount (row.go:226). */
int32_t fbk_union_n_intersection_count(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows,
                                       uint64_t n_groups, uint32_t k, const fbk_batch* filter,
                                       const uint32_t* rows_f, uint64_t* out_counts);

/* ---- n-way fold -----------------------------------------------------------------------
 * Generalisation of fbk_union_n to the four set operations, folded left to right over the k
 * rows of each group exactly as the executor's per-shard functions fold a call's children:
 *   FBK_OP_AND     r0 & r1 & ... & r(k-1)    executeIntersectShard  executor.go:5357-5380
 *   FBK_OP_OR      r0 | r1 | ...             executeUnionShard      executor.go:5382-5404
 *   FBK_OP_XOR     r0 ^ r1 ^ ...             executeXorShard        executor.go:5513-5552
 *   FBK_OP_ANDNOT  r0 \ r1 \ ... \ r(k-1)     executeDifferenceShard executor.go:2950-2983
 * (Bitmap.IntersectInPlace / Difference with several others, roaring.go:855-925, 1564-1595.)
 * One launch, the intermediate rows never touch HBM.  AND / ANDNOT need k >= 1. */
int32_t fbk_fold_n(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows, uint64_t n_groups,
                   uint32_t k, uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts);

/* out_counts[g] = |fold(group g) ∩ filter.rows_f[g]| (filter == NULL: |fold(group g)|), never
 * materialised: Count(Intersect(...)) / Count(Union(...)) etc. in one pass
 * (executeCount -> executeBitmapCallShard, executor.go:5839-5892). */
int32_t fbk_fold_n_intersection_count(fbk_ctx* ctx, int32_t op, const fbk_batch* batch, const uint32_t* rows,
                                      uint64_t n_groups, uint32_t k, const fbk_batch* filter,
                                      const uint32_t* rows_f, uint64_t* out_counts);

/* ---- count matrix (GroupBy / TopN / TopK shape) --------------------------------------------
 * For every shard s, out[s][i][j] = |A.rows_a[s*n_a+i] ∩ B.rows_b[s*n_b+j] ∩ F.rows_f[s]|
 * (filter may be NULL).  out_total[i*n_b+j] is the sum over shards (mergeGroupCounts /
 * Pairs.Add arithmetic, executor.go:3728, 2852); out_per_shard (n_shards*n_a*n_b, may be
 * NULL) keeps the per-shard matrices.  Replaces groupByIterator.Next's
 * rows[last].intersectionCount(rows[last-1]) (executor.go:8893) and, with n_b == 1 and
 * B = the filter row, doTopK / fragment.top (executor.go:2705-2746, fragment.go:1317).
 * Limits: n_a, n_b <= 4096 for a matrix; with n_b == 1 (the TopK / TopN shape, served by a
 * dedicated rows-vs-filter kernel) n_a <= 2^22. */
int32_t fbk_count_matrix(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a,
                         const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter,
                         const uint32_t* rows_f, uint32_t n_shards, uint64_t* out_total,
                         uint64_t* out_per_shard);

/* ---- GroupBy over three fields ------------------------------------------------------------------
 * out_total[(p*n_a + i)*n_b + j] = Σ_s |P.rows_p[s*n_p+p] ∩ A.rows_a[s*n_a+i] ∩ B.rows_b[s*n_b+j] ∩ F.rows_f[s]|
 * for all groups at once: groupByIterator.Next's three levels (rows[0] ∩= filter, rows[1] ∩= rows[0], Count =
 * rows[2].intersectionCount(rows[1]): executor.go:8829-8835, 8861-8867, 8893), the per-shard counts summed as mergeGroupCounts
 * does (:3728).  A zero is a group the reference skips (:8913).  No intersection is materialised and the call synchronises once.
 *  - Row lists [n_shards][n_p], [n_shards][n_a], [n_shards][n_b], [n_shards].  filter == NULL: no filter.  p, a and b may be
 *    the same batch, and their row lists may be the same.
 *  - n_p, n_a, n_b <= 4096 and n_p * n_a * n_b <= 2^24 (a 128 MiB result); beyond that FBK_E_INVALID, and the message says
 *    to block the leading field.  NULL arguments and row indexes beyond a batch are FBK_E_INVALID, checked before any launch.
 *    Every error leaves the context usable.
 *  - n_shards == 0 writes a complete all-zero cube; n_p * n_a * n_b == 0 has nothing to write; both return FBK_OK.
 *  - Counts come from the rows' WORDS, never from stored cardinalities.  Every element of out_total is written.  The result is
 *    exact and does not depend on the grid, the chunking or the order of the adds (integer adds of per-shard counts < 2^21).
 *  - One matrix-core pass per shard over dense rows, the partial cube of every shard of a chunk kept in scratch and summed on the
 *    device; rows of batches that are not dense are densified first, a chunk of shards at a time:
 *    most = max(1, min(n_shards, 2^30 / per_shard)) with per_shard = 8 * n_p * n_a * n_b + 2^17 * (the rows densified per shard:
 *    n_p if P is not dense, n_a if A is not, n_b if B is not, 1 if the filter is not);
 *    chunk = ceil(n_shards / ceil(n_shards / most)), the shards dealt evenly over the fewest chunks.  Device scratch is bounded by
 *    that budget plus the result. */
int32_t fbk_count_cube(fbk_ctx* ctx, const fbk_batch* p, const uint32_t* rows_p, uint32_t n_p, const fbk_batch* a,
                       const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b,
                       const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, uint64_t* out_total);

/* ---- GroupBy with aggregate=Sum(field=v) ------------------------------------------------------
 * For every pair (i, j), summed over the shards given (X = A.rows_a[s*n_a+i] ∩ B.rows_b[s*n_b+j] ∩ F.rows_f[s] ∩ exists):
 *   out_counts[i*n_b+j] = Σ_s |X|
 *   out_sums[i*n_b+j]   = Σ_s Σ_k 2^k (|X ∩ ¬sign ∩ plane_k| − |X ∩ sign ∩ plane_k|), uint64 wrap-around as fbk_bsi_sum
 * i.e. fbk_bsi_sum over the filter A_i ∩ B_j ∩ F, summed over the shards, for all pairs at once: groupByIterator.Next's
 * executeSumCountShard per group (executor.go:8880-8913, 2155-2216).  The caller adds count * Base (executor.go:2206).
 * The BSI layout is fbk_bsi_sum's (base_rows[s] + 0 exists, + 1 sign, + 2 + k plane k); bits of the sign or a plane outside
 * exists contribute nothing.  b == NULL is the one-field GroupBy: n_b must be 1 and X = A_i ∩ F ∩ exists.  filter == NULL:
 * no filter.  bit_depth 0..64; n_a, n_b <= 4096.  Row lists [n_shards][n_a], [n_shards][n_b], [n_shards], [n_shards].
 * One matrix-core pass per shard over dense rows; rows of batches that are not dense are densified first, a chunk of shards
 * at a time: most = max(1, min(n_shards, 2^30 / per_shard)) with per_shard = ceil(bit_depth / 7) * 2^20 + 16 * n_a * n_b
 * + 2^17 * (the rows densified per shard: n_a if A is not dense, n_b if B is not, 1 if the filter is not, bit_depth + 2 if
 * the BSI batch is not); chunk = ceil(n_shards / ceil(n_shards / most)), the shards dealt evenly over the fewest chunks.
 * fbk_query_count_matrix_sum is the prepared form: fbk_query_run takes no device_out and no FBK_QUERY_ACCUMULATE;
 * fbk_query_read(q, out0, out1) gives the int64 sums [n_a*n_b] in out0 and the uint64 counts [n_a*n_b] in out1. */
int32_t fbk_count_matrix_sum(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                             const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                             const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                             int64_t* out_sums, uint64_t* out_counts);
int32_t fbk_query_count_matrix_sum(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                   const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                   const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                                   fbk_query** out_query);

/* ---- GroupBy with aggregate=Count(Distinct(field=v)) -------------------------------------------
 * For every pair (i, j), over ALL the shards given together (X_s = A.rows_a[s*n_a+i] ∩ B.rows_b[s*n_b+j] ∩ F.rows_f[s] ∩ exists):
 *   out_distinct[i*n_b+j] = |{ value(c) : c in X_s, any s }|, value = sign ? -magnitude : magnitude (int64 wrap-around, as
 *                           fbk_bsi_distinct: a set sign bit with magnitude 0 is the value 0); a union of value sets over the
 *                           shards, not a sum of per-shard counts
 *   out_counts[i*n_b+j]   = Σ_s |X_s| (may be NULL)
 * i.e. fbk_bsi_distinct's *out_n over the filter A_i ∩ B_j ∩ F, for all pairs at once: executor.go's Count(Distinct(Intersect(
 * group rows, filter))) per result group (:3338-3386).  Base is not needed (adding it is a bijection).  Sign and plane bits
 * outside exists are ignored.  Arguments as fbk_count_matrix_sum: b == NULL is the one-field form (n_b must be 1),
 * filter == NULL no filter, bit_depth 0..64, n_a, n_b <= 4096; fewer than 2^31 values of exists ∩ F per call; an exists row
 * whose stored cardinality is wrong gives FBK_E_INVALID.
 * Device scratch is bounded: the distinct values (fbk_bsi_distinct's buffers, 24 bytes per value of exists ∩ F), then a
 * presence tile of at most 2^27 bytes: with wb = ceil(n_b / 64), m64 = the number of distinct values rounded up to 64 and
 * row = 8 * wb * m64, one tile if n_a * row <= 2^27; else, if 64 * row <= 2^27, tiles of floor(2^27 / row) rounded down to a
 * multiple of 64 A rows; else tiles of min(n_a, 64) A rows x floor(2^27 / (8 * wb * min(n_a, 64))) rounded down to a multiple
 * of 64 values.  Every tile reads the operands once more.  Rows of batches that are not dense are densified a chunk of shards
 * at a time: most = max(1, min(n_shards, 2^30 / per_shard)) with per_shard = 2^17 * (n_a if A is not dense, n_b if B is not,
 * 1 if the filter is not, bit_depth + 2 if the BSI batch is not); chunk = ceil(n_shards / ceil(n_shards / most)); with more
 * than one chunk every tile densifies them again.  out_counts adds fbk_count_matrix_sum's count pass (its chunk arithmetic
 * at bit_depth 0). */
int32_t fbk_count_matrix_distinct(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                  const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                  const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                                  uint64_t* out_distinct, uint64_t* out_counts);

/* ---- GroupBy with Min / Max of an int field per group (SQL MIN(x), MAX(x) ... GROUP BY a, b) -----
 * For every pair (i, j), over ALL the shards given together (X_s = A.rows_a[s*n_a+i] ∩ B.rows_b[s*n_b+j] ∩ F.rows_f[s] ∩ exists,
 * X = the union of the X_s):
 *   out_min[i*n_b+j] / out_max[i*n_b+j]    the smallest / largest value over the columns of X
 *   out_min_counts / out_max_counts        the number of columns of X holding that value.  Pass both or neither as NULL; when
 *                                          NULL the pass that counts is not run.
 * The value of a column is fbk_extract_bsi's: sign ? -magnitude : magnitude.  A set sign over magnitude 0 is the value 0; sign and
 * plane bits outside exists are ignored.  Values are ORDERED as mathematical integers (up to 65 bits at depth 64) and WRITTEN as
 * int64 with wrap-around, exactly as fbk_bsi_min / fbk_bsi_max write theirs.  Base is not applied: the caller adds it.
 * An empty group gives out_min = INT64_MAX, out_max = INT64_MIN and counts 0: the identities of the fold, so a merge across nodes
 * is a plain min / max that adds the counts on equality.  For bit_depth <= 63 a non-empty group always has min <= max, so the
 * pair itself tells an empty group; at depth 64, where values wrap, ask for the counts.
 * Relation to the reference: the result is fragment.min / fragment.max (fragment.go:754-853) over the filter Intersect(group
 * rows, filter) per shard, folded over the shards by ValCount.Smaller / Larger (executor.go:8446-8548).  (The reference's SQL
 * planner refuses MIN / MAX under GROUP BY: sql3/planner/oppqlgroupby.go:188-195.)  Values are the same while no selected
 * magnitude reaches 2^63 (the reference's fold compares the wrapped int64).  Counts are the same whenever no column has the sign
 * bit over magnitude 0: the reference's importers never write that, and its per-shard scan counts such columns apart from the
 * +0 ones; here they are the value 0 like any other.
 * Arguments as fbk_count_matrix_sum: b == NULL is the one-field form (n_b must be 1), filter == NULL no filter, bit_depth 0..64,
 * n_a, n_b <= 4096, row lists [n_shards][n_a], [n_shards][n_b], [n_shards], [n_shards].  n_shards == 0 writes the empty-group
 * values.  Errors (NULL ctx / a / bsi / base_rows / out_min / out_max, exactly one count pointer NULL, unknown flags, a pinned
 * descent above its cap, row indexes beyond a batch) are FBK_E_INVALID before any launch.  One synchronisation per call.
 * flags picks the kernel path:
 *   FBK_MINMAX_DESCENT  lanes = groups: every group scans the bit planes MSB -> LSB on its own 64-column mask.  Work grows with
 *                       n_a * n_b whatever the rows hold; at most 1024 groups (FBK_E_INVALID above).
 *   FBK_MINMAX_SCATTER  lanes = columns: every column updates the groups it is in with 64-bit atomic min / max.  Work is the sum
 *                       over columns of |A rows holding it| * |B rows holding it|: best for mutex-like fields, poor for set
 *                       fields with many rows per column.  Device scratch is 48 bytes per group (768 MiB at 4096 x 4096), not
 *                       tiled.  With counts the operands are walked twice.
 *   FBK_MINMAX_AUTO     the descent iff n_a * n_b <= 64 (featurebase_amd/csrc/fbk_minmax_plan.h: kMinmaxDescentCells, fixed from a
 *                       measured sweep on mutex-like rows, where the descent was ahead up to 64 groups at depth 20 and up to 128 at
 *                       depth 8; a caller whose columns sit in many rows of a field may pin the descent, one with a field of
 *                       60 bits or more the scatter).
 * Rows of batches that are not dense are densified a chunk of shards at a time: most = max(1, min(n_shards, 2^30 / per_shard))
 * with per_shard = 2^17 * (n_a if A is not dense, n_b if B is not, 1 if the filter is not, bit_depth + 2 if the BSI batch is
 * not); chunk = ceil(n_shards / ceil(n_shards / most)); with more than one chunk the scatter path's counting walk densifies
 * them again.  The descent path's other scratch is at most 8 MiB of partials and 64 bytes per group. */
#define FBK_MINMAX_AUTO    0u  /* the library chooses the kernel path by the shape */
#define FBK_MINMAX_DESCENT 1u  /* pin the plane-descent path; FBK_E_INVALID when n_a * n_b exceeds its cap */
#define FBK_MINMAX_SCATTER 2u  /* pin the per-column scatter path */
int32_t fbk_count_matrix_minmax(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                                uint32_t flags, int64_t* out_min, int64_t* out_max, uint64_t* out_min_counts,
                                uint64_t* out_max_counts);

/* ---- GroupBy with a percentile of an int field per group (SQL PERCENTILE_DISC(x, p) ... GROUP BY a, b) -----
 * For every group g = i*n_b + j, over ALL the shards given together (X_s = A.rows_a[s*n_a+i] ∩ B.rows_b[s*n_b+j] ∩ F.rows_f[s] ∩
 * exists, X = the union of the X_s), with s_g[0 .. N_g) the values of the columns of X in ascending order:
 *   out_totals[g]           N_g, the number of columns of X; always written
 *   out_values[g*n_q + q]   s_g[k], k = max(1, ceil(N_g * q_num[q] / q_den[q])) - 1 in exact integer arithmetic: SQL's
 *                           PERCENTILE_DISC(num / den).  num = 0 is the minimum, num = den the maximum, 1/2 over N = 4 is s[1].
 *   out_counts[g*n_q + q]   the number of columns of X holding exactly that value
 * N_g == 0 gives value 0 and count 0 for every q.  Every element of the three arrays is written.
 * A column's value and the ORDER of the values are fbk_bsi_quantiles': sign ? -magnitude : magnitude with int64 wrap-around (at
 * depth 64 the order is the wrapped int64's, unlike fbk_count_matrix_minmax's), Base not added, sign and plane bits outside
 * exists ignored, a set sign over magnitude 0 the value 0, stored zeros take part.
 * Requests: 1 <= den <= 2^20, num <= den, n_q <= 16; they may repeat and come in any order.  n_q == 0: only out_totals is produced,
 * no plane is read, out_values / out_counts may be NULL.
 * Arguments a .. n_shards as fbk_count_matrix_minmax: b == NULL is the one-field form (n_b must be 1), filter == NULL no filter,
 * bit_depth 0..64, n_a, n_b <= 4096, row lists [n_shards][n_a], [n_shards][n_b], [n_shards], [n_shards]; at most 2^20 shards.
 * n_shards == 0 writes the empty-group values; n_a * n_b == 0 writes nothing.  Errors (NULL ctx / a / bsi / base_rows / out_totals;
 * NULL q_num / q_den / out_values / out_counts with n_q > 0; den == 0, den > 2^20, num > den; n_q > 16; n_a or n_b > 4096;
 * bit_depth > 64; b == NULL with n_b != 1; row indexes beyond a batch; unknown flags; a pinned path beyond its cap; histogram
 * scratch beyond its bound) are FBK_E_INVALID before any launch, and the context stays usable.
 * Method: ONE radix select on fbk_bsi_sort's key (bit_depth + 1 bits up to depth 62, 64 bits at 63 and 64), whole digits from the
 * top and the short digit last, whose histograms are kept per (group, request); passes = ceil(key bits / digit) = ceil((bit_depth + 1) / digit)
 * up to depth 63 and ceil(64 / digit) at 64.  Every pass reads each plane once whatever the number of groups; the ranks are
 * resolved on the device between the passes; one synchronisation per call.  The result does not depend on the grid, the chunking
 * or the order of the blocks: every count is a sum of integer adds.  flags picks the kernel path
 * (featurebase_amd/csrc/fbk_group_quantile_plan.h):
 *   FBK_GQUANT_GLOBAL  digit 8 bits; 64-bit histograms in device memory, one atomic add per (column, group, live request).  Scratch
 *                      = n_a * n_b * max(1, n_q) * 2^digit * 8 bytes, not tiled; above 2^30 bytes (2^19 (group, request) pairs)
 *                      the call is FBK_E_INVALID: block the leading field (fewer A rows per call).
 *   FBK_GQUANT_LDS     digit 8 bits; 32-bit histograms of ALL the (group, request) pairs in a block's 64 KiB of LDS, so at most
 *                      64 KiB / (4 * 2^digit) = 64 pairs n_a * n_b * max(1, n_q) (FBK_E_INVALID above); the blocks' partial
 *                      histograms (at most 2^26 bytes) are summed per bin, then the same scratch as above.
 *   FBK_GQUANT_AUTO    the LDS path iff n_a * n_b * max(1, n_q) <= 64 (kAutoLdsPairs, fixed from a measured sweep on mutex-like rows:
 *                      the LDS path was ahead wherever it applies; a single group through FBK_GQUANT_GLOBAL is 14 - 27 x slower).
 * Rows of batches that are not dense are densified a chunk of shards at a time by fbk_count_matrix_minmax's scatter rule: most =
 * max(1, min(n_shards, 2^30 / per_shard)) with per_shard = 2^17 * (n_a if A is not dense, n_b if B is not, 1 if the filter is not,
 * bit_depth + 2 if the BSI batch is not; 2 for it with n_q == 0); chunk = ceil(n_shards / ceil(n_shards / most)); with more than
 * one chunk every pass densifies them again.
 * NOT offered: a prepared fbk_query_* form; a fbk_group_* form (quantiles of shards on different devices do not merge: a group
 * must live on one device); the reference's bisection Percentile (fbk_bsi_percentile) replayed per group.  The reference has no
 * counterpart: its GroupBy takes Count, Sum and Count(Distinct) only. */
#define FBK_GQUANT_AUTO   0u /* the library chooses the kernel path by the shape */
#define FBK_GQUANT_LDS    1u /* pin the LDS-histogram path; FBK_E_INVALID when the (group, request) pairs exceed its cap */
#define FBK_GQUANT_GLOBAL 2u /* pin the device-memory histogram path */
int32_t fbk_count_matrix_quantiles(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                   const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                   const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                                   const uint32_t* q_num, const uint32_t* q_den, uint32_t n_q, uint32_t flags, int64_t* out_values,
                                   uint64_t* out_counts, uint64_t* out_totals);

/* ---- GroupBy(..., having=, sort=, offset=, limit=): only the selected groups leave the device -----
 * executeGroupBy's tail (executor.go:3176-3459: ApplyConditionToGroupCounts / satisfiesCondition :3787-3916, groupCountSorter and
 * getSorter :3096-3162, sort.Stable :3409, applyLimitAndOffsetToGroupByResult :3441-3459) applied to the totals of a GroupBy call
 * while they are still on the device.  Over cells 0 .. n-1 (the full call's output index: odometer order, last field fastest) with
 * counts[cell] (uint64) and, where the call has an aggregate, aggs[cell] (int64):
 *  - Groups: the cells with count > 0 (:8913) that pass `having`; *out_matched = their number, before offset / limit.
 *  - having_subject FBK_GROUPSEL_NONE: no condition.  _COUNT compares the count as uint64 (having_lo / having_hi are read as uint64),
 *    _AGG compares the aggregate as int64.  having_op: FBK_HAVING_EQ, _NEQ, _LT, _LTE, _GT, _GTE compare x with having_lo
 *    (having_hi is ignored); _BETWEEN lo <= x <= hi, _BTWN_LT_LTE lo < x <= hi, _BTWN_LTE_LT lo <= x < hi, _BTWN_LT_LT lo < x < hi;
 *    lo > hi selects nothing.  (The reference's "a negative literal in a count condition matches nothing" — Uint64Value fails,
 *    :3792-3795 — is the CALLER's rule: this struct cannot express a negative count bound.)
 *  - sort: n_sort = 0, 1 or 2 terms {subject FBK_GROUPSEL_COUNT | _AGG, desc 0 | 1}, compared in the order given; groups equal in
 *    every term keep ascending cell order (sort.Stable over the odometer order).  n_sort = 0: ascending cell order.  The same
 *    subject twice is FBK_E_INVALID (a repeated term never decides: drop it before the call).
 *  - offset, then limit, on that list: the records of ranks [offset, offset + limit).  limit = UINT64_MAX: none; offset + limit may
 *    exceed 2^64; offset >= *out_matched gives *out_n = 0.  (applyLimitAndOffsetToGroupByResult IGNORES such an offset, and a
 *    GroupBy with neither sort nor having applies its limit twice, :3302 and :3331: both are the caller's to reproduce —
 *    fbk::Executor::GroupBy does — and *out_matched is what tells it.)
 *  - Output: record k = {out_cells[k] (uint32), out_counts[k], out_aggs[k]}.  *out_n = the records of the result and *out_matched
 *    are always written, on FBK_OK and on FBK_E_CAPACITY; cap < *out_n -> FBK_E_CAPACITY, the arrays untouched (the fbk_bsi_sort
 *    convention).  cap > 0 with a NULL array is FBK_E_INVALID.
 *  - flags: FBK_GROUPSEL_DEVICE / FBK_GROUPSEL_HOST pin the path (tests, measurements); both is FBK_E_INVALID; neither: the library
 *    downloads the totals and selects on the host when n <= 2^16 cells (measured: the device stage costs about 45 us of launches
 *    without a sort and about 200 us with one, which the transfer of 2^16 cells and the host's pass still undercut or match;
 *    docs/history/DESIGN_groupby_select_measurements.md), on the device above.  Both paths give identical output.
 *  - An unknown flag, op, subject or desc, n_sort > 2, a sort term or a having on _AGG where the call has no aggregate: FBK_E_INVALID,
 *    checked with the GroupBy call's own argument checks before any launch.  Every error leaves the context usable.
 *  - Device path: one ordered compaction pass over the cells (wave ballot ranks, block counts, a scan, an emit pass) gives the
 *    matched cells in ascending order; without a sort only the ranks [offset, offset + limit) are written.  With a sort and
 *    K = offset + limit < matched, an MSB-first radix select (8 bits per pass over the order-preserving 64-bit keys of the terms,
 *    digits chosen on the device) finds the key of rank K, a second ordered pass keeps the keys below it and the first ties in cell
 *    order, and only those K are sorted (stable radix sort, secondary term first).  Without an effective limit all matched groups
 *    are sorted.  Device scratch beside the totals themselves (8 n bytes, 16 n with an aggregate), with U = ceil(n / 512),
 *    K = min(offset + limit, matched), W = the cells that are sorted (K if K < matched, else matched) and n_out the records:
 *      16 (U + 1) + the scan's temporary storage (~U) + 20 n_out, and with a sort 4 * matched + 20 W + the radix sort's
 *      temporary storage (~12 W) + (K < matched: 4 K + 2^10 + 32) bytes: never a (key, key, index) record per cell.
 *
 * fbk_count_matrix_select: fbk_count_matrix's arguments (no per-shard output) — the one- and two-field GroupBy on counts
 *   (n_b == 1 with B = the filter row is the one-field form); cell = i * n_b + j.  Counts only.
 * fbk_count_cube_select: fbk_count_cube's arguments; cell = (p * n_a + i) * n_b + j.  Counts only.
 * fbk_count_matrix_sum_select: fbk_count_matrix_sum's arguments; the aggregate is the sum (Base NOT added), the count is the sum's
 *   count (over exists).
 * fbk_select_groups: the stage alone over host arrays counts[n], aggs[n] (aggs may be NULL: counts only), n <= 2^24: for
 *   fbk_count_matrix_distinct results and results merged from several blocked calls.
 * n_shards == 0 or zero cells: *out_n = *out_matched = 0, FBK_OK. */
#define FBK_GROUPSEL_DEVICE 1u
#define FBK_GROUPSEL_HOST 2u
#define FBK_GROUPSEL_NONE 0u
#define FBK_GROUPSEL_COUNT 1u
#define FBK_GROUPSEL_AGG 2u
#define FBK_HAVING_EQ 1u
#define FBK_HAVING_NEQ 2u
#define FBK_HAVING_LT 3u
#define FBK_HAVING_LTE 4u
#define FBK_HAVING_GT 5u
#define FBK_HAVING_GTE 6u
#define FBK_HAVING_BETWEEN 7u
#define FBK_HAVING_BTWN_LT_LTE 8u
#define FBK_HAVING_BTWN_LTE_LT 9u
#define FBK_HAVING_BTWN_LT_LT 10u
typedef struct fbk_groupby_term {
  uint32_t subject; /* FBK_GROUPSEL_COUNT | FBK_GROUPSEL_AGG */
  uint32_t desc;    /* 0 ascending, 1 descending */
} fbk_groupby_term;
typedef struct fbk_groupby_select {
  uint32_t flags;
  uint32_t n_sort;
  fbk_groupby_term sort[2];
  uint32_t having_subject; /* FBK_GROUPSEL_NONE | _COUNT | _AGG */
  uint32_t having_op;      /* FBK_HAVING_* */
  int64_t having_lo, having_hi;
  uint64_t offset, limit;
} fbk_groupby_select; /* 64 bytes */
int32_t fbk_count_matrix_select(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                uint32_t n_shards, const fbk_groupby_select* sel, uint32_t* out_cells, uint64_t* out_counts,
                                uint64_t cap, uint64_t* out_n, uint64_t* out_matched);
int32_t fbk_count_cube_select(fbk_ctx* ctx, const fbk_batch* p, const uint32_t* rows_p, uint32_t n_p, const fbk_batch* a,
                              const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b, const uint32_t* rows_b, uint32_t n_b,
                              const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, const fbk_groupby_select* sel,
                              uint32_t* out_cells, uint64_t* out_counts, uint64_t cap, uint64_t* out_n, uint64_t* out_matched);
int32_t fbk_count_matrix_sum_select(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* b,
                                    const uint32_t* rows_b, uint32_t n_b, const fbk_batch* filter, const uint32_t* rows_f,
                                    const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, uint32_t n_shards,
                                    const fbk_groupby_select* sel, uint32_t* out_cells, uint64_t* out_counts, int64_t* out_aggs,
                                    uint64_t cap, uint64_t* out_n, uint64_t* out_matched);
int32_t fbk_select_groups(fbk_ctx* ctx, const uint64_t* counts, const int64_t* aggs, uint64_t n, const fbk_groupby_select* sel,
                          uint32_t* out_cells, uint64_t* out_counts, int64_t* out_aggs, uint64_t cap, uint64_t* out_n,
                          uint64_t* out_matched);

/* ---- Extract(filter, Rows(f1), Rows(f2), ...): the records of a column filter -------------------
 * executeExtract (executor.go:4711-5046), usually under executeLimitCall's Extract(Limit(filter, limit=, offset=), ...)
 * (:1027-1100).  A handle fixes the selected columns once, then one call per field rotates that field's bits into per-column
 * results on the device (64 x 64 in-register transposes; a column's output slot is its rank, computed from popcounts).
 *
 * fbk_extract_open: the selected columns are the set bits of filter.rows_f[s], s = 0 .. n_shards-1, in the order given
 * (shard_ids strictly ascending and < 2^44), column = shard_ids[s] * 2^20 + position; of these the ranks [offset, offset + limit)
 * (limit = UINT64_MAX: no limit; offset + limit may exceed 2^64) — offset, then limit, on the ascending column list.  *out_n = n,
 * their number.
 *  - Selection is computed from the filter's WORDS, never from stored cardinalities: a batch whose stored cardinality is wrong
 *    cannot misplace output.
 *  - n must be below 2^31, otherwise FBK_E_INVALID (the message says to use a limit).  n == 0 (empty filter, limit == 0,
 *    offset >= the filter's count, n_shards == 0) is a valid handle whose calls write nothing but out_offsets[0] = 0 and
 *    *out_n_items = 0.
 *  - The call synchronises once (it returns n).  It records the span of shards [first, first + count) that hold a selected column
 *    (fbk_extract_span); the per-field calls never densify or read a shard outside that span, and inside it skip every 1024-column
 *    unit and every 64-column word without a selected column: Extract(Limit(All(), limit=1000)) over a thousand shards costs a
 *    few words per row, not the field.
 *  - Resident in the handle until fbk_extract_free: per shard OF THE SPAN 2^17 bytes (the filter's words with the selected
 *    columns only — a dense copy, whatever the filter's encoding) + 2^12 bytes (the rank of every 1024-column unit's first
 *    column), and 8 bytes per shard of the call.  The handle does not read the filter batch after open, but it belongs to the
 *    query that owns that batch: keep the filter batch alive until the handle is freed, and free every handle before fbk_close.
 *  - The handle belongs to the context that opened it (another context: FBK_E_INVALID) and every call takes that context's lock
 *    and stream; its resident state is its own, not the context's scratch: several handles may be alive and used alternately.
 *  - Filter, BSI and A batches may be dense or encoded.  Rows of a batch that is not dense are densified a chunk at a time into at
 *    most 2^28 bytes of scratch: with R the rows densified per shard (filter: 1; fbk_extract_bsi: bit_depth + 2;
 *    fbk_extract_rows: n_a) and per_shard = 2^17 * R: if per_shard <= 2^28, most = max(1, min(shards, 2^28 / per_shard)) and
 *    chunk = ceil(shards / ceil(shards / most)) shards per launch with all their rows; else one shard per launch in blocks of
 *    2^28 / 2^17 = 2048 rows.  `shards` is n_shards for fbk_extract_open (both of its passes) and the span's count for the
 *    per-field calls.  Results do not depend on the chunking or on the grid size.
 *
 * fbk_extract_columns: out_columns[k], k < n: the selected columns, ascending.
 * fbk_extract_bsi (int field, layout of fbk_bsi_sum, base_rows [n_shards] as given to open, bit_depth 0..64):
 *   out_present[k] = 1 and out_values[k] = sign ? -magnitude : magnitude (Base NOT added, int64 wrap-around, a set sign bit over
 *   magnitude 0 is 0 — as fbk_bsi_distinct) when column k is in exists; else 0 and 0.  Sign and plane bits outside exists are
 *   ignored (executor.go:5007, :5016 intersect with exists).  Every element of both arrays is written.
 * fbk_extract_rows (set / mutex / bool field, rows_a = [n_shards][n_a] as fbk_count_matrix's, n_a <= 4096): CSR over the n columns:
 *   the items of column k = out_items[out_offsets[k] .. out_offsets[k+1]) = the indices i (0 .. n_a-1, ascending) with the column
 *   in A.rows_a[s*n_a+i].  *out_n_items is always set; cap too small -> FBK_E_CAPACITY, out_offsets [n+1] still complete,
 *   out_items untouched (the fbk_bsi_distinct convention).  Fields of more than 4096 rows take one call per block of rows.
 * fbk_extract_free: NULL handle is a no-op. */
typedef struct fbk_extract fbk_extract;
int32_t fbk_extract_open(fbk_ctx* ctx, const fbk_batch* filter, const uint32_t* rows_f, const uint64_t* shard_ids, uint32_t n_shards,
                         uint64_t offset, uint64_t limit, fbk_extract** out, uint64_t* out_n);
int32_t fbk_extract_span(fbk_ctx* ctx, const fbk_extract* h, uint32_t* out_first, uint32_t* out_count);
int32_t fbk_extract_columns(fbk_ctx* ctx, fbk_extract* h, uint64_t* out_columns);
int32_t fbk_extract_bsi(fbk_ctx* ctx, fbk_extract* h, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth,
                        int64_t* out_values, uint8_t* out_present);
int32_t fbk_extract_rows(fbk_ctx* ctx, fbk_extract* h, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, uint64_t* out_offsets,
                         uint32_t* out_items, uint64_t cap, uint64_t* out_n_items);
int32_t fbk_extract_free(fbk_ctx* ctx, fbk_extract* h);

/* fbk_extract_open_columns: a handle that selects exactly columns[0 .. n) (any order, n < 2^31) instead of a filter's bits: the
 * winners of fbk_bsi_sort for Extract(Sort(...), Rows(f), ...) (executor.go:4686-4700, :4762-4769), or the list of
 * Extract(ConstRow(columns=[...]), ...) (:5604-5694).  shard_ids as fbk_extract_open; a column whose shard (column >> 20) is not in
 * shard_ids, or one listed twice, is FBK_E_INVALID.  out_rank[k] (n entries) = the slot of columns[k] in the handle's ASCENDING
 * column order: the per-field calls answer in that order, so record k of the caller's list is slot out_rank[k] of their outputs.
 * Span (the shards between the smallest and the largest listed column), residency and every per-field call are those of a handle
 * from fbk_extract_open; base_rows / rows_a of the per-field calls are [n_shards] / [n_shards][n_a] over the shard_ids given here.
 * The bits are ORed into the handle's words on the device (distinct bits: the result does not depend on the order). */
int32_t fbk_extract_open_columns(fbk_ctx* ctx, const uint64_t* columns, uint64_t n, const uint64_t* shard_ids, uint32_t n_shards,
                                 fbk_extract** out, uint32_t* out_rank);

/* ---- Sort(filter, field=, sort-desc=, limit=, offset=) by an int field ---------------------------
 * executeSort / executeSortShard / SortedRow.Merge (executor.go:9321-9385, :9387-9538, :9574-9608, fragment.go:2878-2969): the
 * columns of exists ∩ filter ordered by the field's value, then offset, then limit.  The reference sorts every shard and merges
 * whole shard results before it cuts; this call SELECTS: K = min(offset + limit, total) candidates are found by a radix select
 * over the bit planes (ceil((bit_depth + 1) / 11) passes, 64-bit keys for bit_depth 63 and 64), only they are sorted, and only
 * the records of ranks [offset, K) leave the device.
 *  - Field layout as fbk_bsi_sum (base_rows[s] + 0 exists, + 1 sign, + 2 + i plane i; bit_depth 0..64); shard_ids as
 *    fbk_extract_open (strictly ascending, < 2^44, column = shard id * 2^20 + position; at most 2^20 shards per call).
 *    filter == NULL: every column of exists.  Dense and encoded batches both work; what is not dense is densified a chunk of
 *    shards at a time by fbk_extract_*'s rule with R = (field encoded ? bit_depth + 2 : 0) + (filter encoded ? 1 : 0).
 *  - out_values[k] is exactly fbk_extract_bsi's value of out_columns[k]: sign ? -magnitude : magnitude, int64 wrap-around (bit_depth
 *    64: magnitudes >= 2^63 order as the negative numbers they wrap to), Base NOT added.  Sign and plane bits outside exists are
 *    ignored.
 *  - KEPT REFERENCE QUIRK (default): a column whose magnitude is 0 does NOT take part, with or without its sign bit:
 *    flattenRowValues (fragment.go:2943-2969) builds its column -> value map from the set PLANE bits only, so a stored 0 never
 *    reaches RowKVs.  FBK_SORT_KEEP_ZERO keeps those columns with value 0: what ORDER BY of a SQL caller means.
 *  - Order: value ascending, FBK_SORT_DESC descending.  Columns of EQUAL value come in ascending column id, in both directions and
 *    across shards.  The reference leaves this unspecified (Go map iteration order under a stable sort, and SortedRow.Merge takes
 *    the OTHER shard's record first on a tie): fixed here, as TopN's ties were.
 *  - offset, then limit, on that global order (executor.go:9367-9383).  limit == UINT64_MAX: no limit.  offset past the end or
 *    limit == 0: *out_n = 0 (the reference panics or slices past len there; not copied).
 *  - *out_n = the records of the result, always set; cap < *out_n -> FBK_E_CAPACITY, out_columns / out_values untouched (the
 *    fbk_bsi_distinct convention).  *out_total (may be NULL) = the columns that take part, before offset / limit.
 *  - K must be below 2^31, else FBK_E_INVALID (the message says to use a limit).  The TOTAL is not capped.  Device scratch, with
 *    n_less <= K the columns below the K-th value and n = *out_n:
 *      2^14 + 2^23 (histograms) + 2^15 * n_shards + chunk (<= 2^28, 0 if both batches are dense) + 16 K + 16 n_less + radix sort temporary (~16 n_less)
 *      + 16 n + 4 * (row lists) bytes: no key or value per filtered column.
 *  - The result does not depend on grid size, chunking or the order in which blocks run: histogram counts are sums of per-block
 *    counts (integer addition commutes), every candidate's slot is its rank from popcount prefixes, the device sort is stable.
 *  - Bool, mutex and keyed fields are not sorted here (the reference's bool comparison, fragment.go:2890-2894, is not an order). */
#define FBK_SORT_DESC 1u
#define FBK_SORT_KEEP_ZERO 2u
int32_t fbk_bsi_sort(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter,
                     const uint32_t* rows_f, const uint64_t* shard_ids, uint32_t n_shards, uint32_t flags, uint64_t offset,
                     uint64_t limit, uint64_t* out_columns, int64_t* out_values, uint64_t cap, uint64_t* out_n, uint64_t* out_total);

/* ---- Quantiles and Percentile(field=, nth=, filter=) of an int field ------------------------------
 * Both calls are ONE radix select over the bit planes (fbk_bsi_sort's walk and key: ceil((bit_depth + 1) / 11) passes, 64-bit keys
 * for bit_depth 63 and 64) that follows SEVERAL ranks at once: pass 0 gives N, the ranks are resolved against it, every later pass
 * counts the next digit under each live prefix.  No column id leaves the device, so there is no shard_ids argument.
 *  - Field layout, filter == NULL, dense or encoded batches and the chunking rule are fbk_bsi_sort's (R = (field encoded ?
 *    bit_depth + 2 : 0) + (filter encoded ? 1 : 0)); bit_depth 0..64; at most 2^20 shards per call.
 *  - The value of a column is fbk_extract_bsi's: sign ? -magnitude : magnitude, int64 wrap-around, Base NOT added; sign and plane
 *    bits outside exists are ignored.
 *  - EVERY column of exists ∩ filter takes part, stored zeros included: N is the reference's
 *    Count(Intersect(filter, Row(field != null))) (executor.go:1390-1398).  This is NOT Sort's flattenRowValues quirk (fbk_bsi_sort
 *    drops magnitude 0 by default); it equals fbk_bsi_sort with FBK_SORT_KEEP_ZERO.
 *  - *out_total = N, always set.  n_shards == 0 or N == 0: FBK_OK, every out_counts[i] = 0 (and out_values[i] = 0).
 *  - Device scratch: 2^17 (histograms) + 2^26 (the blocks' partial histograms: at most 1024 blocks of 8 x 2048 counts) + chunk
 *    (<= 2^28, 0 if both batches are dense) + 4 * (row lists) bytes.  One launch counts under at most 8 prefixes (64 KiB of LDS); a
 *    pass with more live prefixes takes ceil(prefixes / 8) walks over the planes.  The host reads prefixes * 2048 counts per pass.
 *  - The result does not depend on grid size, chunking or the order in which blocks run: every count is a sum of per-block counts.
 *
 * fbk_bsi_quantiles: with s[0 .. N) the ascending values, ranks[i] = k asks for s[k], FBK_RANK_FROM_TOP | k for s[N-1-k].
 *   out_values[i] = that value, out_counts[i] = the participating columns holding exactly it.  k >= N: (0, 0) — "no such rank", not
 *   an error.  Ranks may repeat and come in any order; n_ranks <= 1024, else FBK_E_INVALID.  n_ranks == 0: the count alone, one
 *   walk over exists and filter (no plane is read).  PERCENTILE_DISC, box plots, equi-depth histograms; no reference counterpart.
 *
 * fbk_bsi_percentile: executePercentile (executor.go:1310-1601) for each nth[i] (n_nth <= 256; outside [0, 100] or NaN:
 *   FBK_E_INVALID), on value + base.  With L = uint64((double(N) * nth) / 100.0) and G = uint64((double(N) * (100 - nth)) / 100.0)
 *   (:1408-1409): G != 0 and L == 0 -> the minimum, G == 0 -> the maximum, out_counts[i] = the columns holding it (what
 *   ValCount.Smaller / Larger accumulate, :8446, :8526); else the reference's bisection between minimum and maximum, out_counts[i]
 *   = 1.  The bisection is REPLAYED, not searched: "leftCount > desiredLess" holds exactly when s[L] < guess and "rightCount >
 *   desiredGreater" exactly when s[N-1-G] > guess, so the ranks 0, N-1, L and N-1-G of one select fix every step — including the
 *   reference's quirks (it may answer a value no column holds, and it answers the last guess when the bounds cross).  N == 0:
 *   out_counts[i] = 0 (the median of nothing is NULL, :1399-1402).  minimum + base or maximum + base outside int64: FBK_E_INVALID.
 *   Int, and timestamp-as-integer, fields only: the decimal branch (:1466-1490) does its arithmetic in pql.Decimal and stays with
 *   the caller. */
#define FBK_RANK_FROM_TOP (1ull << 63)
int32_t fbk_bsi_quantiles(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter,
                          const uint32_t* rows_f, uint32_t n_shards, const uint64_t* ranks, uint32_t n_ranks, int64_t* out_values,
                          uint64_t* out_counts, uint64_t* out_total);
int32_t fbk_bsi_percentile(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, const fbk_batch* filter,
                           const uint32_t* rows_f, uint32_t n_shards, int64_t base, const double* nth, uint32_t n_nth,
                           int64_t* out_values, uint64_t* out_counts, uint64_t* out_total);

/* ---- BSI (bit-sliced integers) ----------------------------------------------------------------
 * A BSI fragment of shard s occupies bit_depth+2 consecutive rows of `batch` starting at
 * base_rows[s]: +0 exists, +1 sign, +2+i magnitude bit i (fragment.go:62-65). */
#define FBK_BSI_EQ 1
#define FBK_BSI_NEQ 2
#define FBK_BSI_LT 3
#define FBK_BSI_LTE 4
#define FBK_BSI_GT 5
#define FBK_BSI_GTE 6

/* Per shard: out_counts[s] = |exists ∩ filter|, out_sums[s] = Σ_i 2^i (|pos ∩ bit_i| − |neg ∩ bit_i|)
 * with uint64 wrap-around exactly as BitmapBSICountFilter (roaring/filter.go:1097-1218,
 * fragment.sum fragment.go:724-750).  filter == NULL means "no filter"; a filter row with no
 * container in a slot contributes nothing for that slot.  The caller adds count*Base
 * (executor.go:2205). */
int32_t fbk_bsi_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_sums,
                    uint64_t* out_counts);

/* ---- SQL VAR(x) and CORR(x, y): the raw moments of two int fields in one pass -------------------
 * Over all the shards given, E_s = exists_x ∩ exists_y ∩ F.rows_f[s] (filter == NULL: no filter; the reference skips a row when
 * either value is nil, sql3/planner/expressionagg.go:978-981):
 *   n = Σ_s |E_s|,  sum_x = Σ x,  sum_y = Σ y,  sum_xx = Σ x²,  sum_yy = Σ y²,  sum_xy = Σ x·y   over the columns of every E_s,
 * what aggregateVar (:1110-1195) and aggregateCorr (:949-1047) fold row by row into float accumulators.  Here every sum is an
 * integer modulo 2^128 (two's complement, as fbk_bsi_sum wraps modulo 2^64): exact whenever the true value fits an int128, which
 * always holds when depth_x + depth_y + ceil(log2 n) <= 127, and independent of the grid, the chunking and the order.
 *  - The field layout is fbk_bsi_sum's (base_rows[s] + 0 exists, + 1 sign, + 2 + k plane k), the value of a column
 *    fbk_extract_bsi's: sign ? -magnitude : magnitude; a set sign over magnitude 0 is 0; sign and plane bits outside exists are
 *    ignored.  Bit depths 0..64 each.  At most 2^28 shards per call.
 *  - y == NULL is the one-field form (VAR): depth_y must be 0, E_s = exists_x ∩ F, and sum_y, sum_yy, sum_xy are written as 0.
 *    x and y may be the same batch and the same field: then sum_xy == sum_xx == sum_yy.
 *  - Base is NOT applied: VAR and CORR do not depend on it.  A caller that wants the moments of x + bx and y + by shifts them:
 *      Σ(x+bx) = Σx + n·bx                         Σ(x+bx)² = Σx² + 2·bx·Σx + n·bx²
 *      Σ(y+by) = Σy + n·by  (Σ(y+by)² alike)       Σ(x+bx)(y+by) = Σxy + by·Σx + bx·Σy + n·bx·by
 *    A decimal field of scale s stores value · 10^s: VAR scales by 10^(-2s), CORR not at all.
 *  - NULL ctx, x, base_rows_x or out, a depth above 64, more than 2^28 shards and row indexes beyond a batch give FBK_E_INVALID
 *    before any launch; every error leaves the context usable.
 *    n_shards == 0 writes an all-zero struct and returns FBK_OK.  One synchronisation per call.
 *  - One matrix-core pass over dense rows, every plane read once; rows of batches that are not dense are densified first, a
 *    chunk of shards at a time: most = max(1, min(n_shards, 2^30 / (2^17 * R))) with R = the rows densified per shard:
 *    depth_x + 2 if x is not dense, depth_y + 2 if y is not, 1 if the filter is not; chunk = ceil(n_shards / ceil(n_shards /
 *    most)), the shards dealt evenly over the fewest chunks (R == 0: one chunk). */
typedef struct fbk_i128 {
  uint64_t lo;
  int64_t hi; /* two's complement: hi * 2^64 + lo */
} fbk_i128;
typedef struct fbk_moments {
  uint64_t n;
  uint64_t reserved;
  fbk_i128 sum_x, sum_y, sum_xx, sum_yy, sum_xy;
} fbk_moments; /* 96 bytes */
int32_t fbk_bsi_moments(fbk_ctx* ctx, const fbk_batch* x, const uint32_t* base_rows_x, uint32_t depth_x, const fbk_batch* y,
                        const uint32_t* base_rows_y, uint32_t depth_y, const fbk_batch* filter, const uint32_t* rows_f,
                        uint32_t n_shards, fbk_moments* out);

/* ---- SQL WHERE x < y: the Row of a comparison between two int fields ------------------------------
 * out row s = the columns of shard s with value_x op value_y, a device Row that every later operator (Count, GroupBy, Sort,
 * Extract, Sum, TopK, the call trees of fbk_expr_*) takes as it takes any filter.  The reference has no fast path for this
 * predicate: generatePQLCallFromBinaryExpr (sql3/planner/expressionpql.go:267-520) needs a literal on the right-hand side
 * (planExprToValue(expr.rhs) fails on a column reference), pushdownFiltersToFilterableRelations (sql3/planner/planoptimizer.go:
 * 393-411) then leaves the filter unpushed, and PlanOpFilter (sql3/planner/opfilter.go:107) evaluates
 * binOpPlanExpression.Evaluate (sql3/planner/expression.go:322-) row by row on the host over an Extract of every record.  Here
 * the answer is a function of the bit planes alone: the BSI Range scan with the constant's bit replaced by the other field's
 * plane, every plane read once (k_bsi_compare_slot).
 *  - The field layout is fbk_bsi_sum's (base_rows[s] + 0 exists, + 1 sign, + 2 + i plane i).  Bit depths 0..64 each; they may
 *    differ.  x and y may be different batches, the same batch, or the same field; dense and encoded batches both work, and
 *    containers are read in their encoded form.
 *  - Participating columns: E_s = exists_x ∩ exists_y ∩ F.rows_f[s] (filter == NULL: no filter).  A column outside E_s is never
 *    in the result, for FBK_BSI_NEQ too: the reference's evaluator yields NULL when either side is NULL (expression.go:348 and
 *    the like) and the filter drops the row.
 *  - The value of a column is (sign ? -magnitude : magnitude) + base as an EXACT integer: bit-sliced arithmetic has no width
 *    limit, so depth 64 and bases at the int64 extremes compare correctly, with no int64 wrap-around.  This is the one place
 *    where the value is not fbk_extract_bsi's, which wraps magnitudes >= 2^63.  A set sign over magnitude 0 is 0; sign and plane
 *    bits outside exists are ignored.
 *  - op is one of FBK_BSI_EQ .. FBK_BSI_GTE, evaluated as value_x op value_y.
 *  - Output as fbk_bsi_range's: the container keys of out row s are s * 16 + slot; out_counts[s] (may be NULL) is the row's
 *    cardinality; flags & FBK_SETOP_OPTIMIZE re-encodes and compacts the result as it does there.
 *  - Count-only form (SELECT COUNT(*) ... WHERE x < y): out_batch == NULL with out_counts != NULL writes the counts only; no
 *    output arena is allocated and no cell is written.  Both NULL is FBK_E_INVALID.
 *  - FBK_COMPARE_PATH_OFFSET pins the general (two's-complement) kernel instance even when base_x == base_y, where the
 *    sign-magnitude instance runs by default; the result is the same bit for bit.
 *  - NULL ctx, x, y or base rows, a filter without rows_f, a depth above 64, an unknown op, unknown flags, 2^27 shards or more
 *    and row indexes beyond a batch give FBK_E_INVALID before any launch; every error leaves the context usable.
 *    n_shards == 0 is FBK_OK with an empty batch, as fbk_bsi_range gives.  One synchronisation per call (FBK_SETOP_OPTIMIZE adds
 *    those of the re-encode).
 *  - Out of this call's scope: decimal fields of different scale and timestamps of different unit.  The caller brings them to
 *    one scale first; only the constant offset base_x - base_y is applied here. */
#define FBK_COMPARE_PATH_OFFSET 0x100u /* pin the general (two's-complement) instance even when base_x == base_y */
int32_t fbk_bsi_compare(fbk_ctx* ctx, const fbk_batch* x, const uint32_t* base_rows_x, uint32_t depth_x, int64_t base_x,
                        const fbk_batch* y, const uint32_t* base_rows_y, uint32_t depth_y, int64_t base_y, int32_t op,
                        const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, uint32_t flags,
                        fbk_batch** out_batch, uint64_t* out_counts);

/* Per shard: (out_vals[s], out_counts[s]) = fragment.min / fragment.max (fragment.go:754-853):
 * the smallest / largest stored value among the columns of exists ∩ filter and the number of
 * columns holding it; (0, 0) when there is no such column.  Sign-magnitude planes, MSB -> LSB
 * scan (minUnsigned :781, maxUnsigned :832).  The caller adds Base (field.go MinForShard /
 * MaxForShard) and folds shards with ValCount.Smaller / Larger (executor.go:8446, 8526). */
int32_t fbk_bsi_min(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_vals,
                    uint64_t* out_counts);
int32_t fbk_bsi_max(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                    uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_vals,
                    uint64_t* out_counts);

/* Distinct values of a BSI field among the columns of exists ∩ filter over all the shards given:
 * executeDistinctShardBSI (executor.go:2034-2153) — which gathers every column's value from the
 * bit planes — followed by the SignedRow.Union reduce over shards (executor.go:1190-1196).
 * out_values receives the sorted distinct stored values (sign applied, Base NOT added: the
 * caller adds bsiGroup.Base and splits into SignedRow{Neg, Pos}); *out_n their number, also when
 * FBK_E_CAPACITY reports that `cap` was too small.  The planes are transposed on the device
 * (64 x 64 bit-matrix transpose in registers), sorted and de-duplicated there. */
int32_t fbk_bsi_distinct(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                         uint32_t bit_depth, const fbk_batch* filter, const uint32_t* rows_f, int64_t* out_values,
                         uint64_t cap, uint64_t* out_n);

/* Distinct(filter, field=f) of an int field as a ROW, the form the reference computes: executeDistinctShardBSI (executor.go:2034-2153)
 * returns SignedRow{Neg, Pos}, two rows whose COLUMNS are the values with bsiGroup.Base added, executeDistinct unites them over the
 * shards (:1190-1196), executeBitmapCallShard accepts Distinct as a child (:1809) and handlePreCalls (:362-449) hands r.Pos of a
 * Distinct on another index to the outer query as a Precomputed row — a foreign-key join.  fbk_bsi_distinct is the list form (SELECT
 * DISTINCT: 24 bytes of scratch per column, a sort, the values on the host); here no value leaves the device and nothing is sorted:
 * setting a bit is de-duplication.
 *  - Field layout, filter == NULL, dense or encoded batches and the chunking rule are fbk_bsi_sort's (R = (field encoded ?
 *    bit_depth + 2 : 0) + (filter encoded ? 1 : 0)); at most 2^20 input shards; no shard_ids argument: column ids play no part.
 *    bit_depth 0..63; 64: FBK_E_INVALID (fbk_bsi_distinct takes such a field).
 *  - The stored value of a column is fbk_extract_bsi's (sign ? -magnitude : magnitude; sign and plane bits outside exists are
 *    ignored; stored zeros take part); v = stored + base.  v >= 0 sets position uint64(v) of Pos, v < 0 position uint64(-v) of Neg
 *    (:2123-2130).  Every participating column of every input shard sets its bit in the same result: the union over shards.
 *    minimum + base or maximum + base outside int64: FBK_E_INVALID (as fbk_bsi_percentile).
 *  - *out_batch: rows [0, n_pos) are the shards (position >> 20) of Pos that hold a bit, ascending; rows [n_pos, n_pos + n_neg)
 *    those of Neg, ascending; row n_pos + n_neg is an EMPTY row without containers, for the caller to name where the result does
 *    not reach a shard.  out_shard_ids[r] = the row's shard; container keys are shard * 16 + slot; out_counts[r] (may be NULL) =
 *    the row's cardinality, recounted from the words.  flags: 0 (bitmap containers) or FBK_SETOP_OPTIMIZE (re-encoded and compacted
 *    as by every materialising call).  The batch is the caller's (fbk_batch_free) and a valid operand of every later call.
 *  - *out_n_pos / *out_n_neg are always set.  cap < n_pos + n_neg: FBK_E_CAPACITY, *out_batch = NULL, out_shard_ids / out_counts
 *    untouched (the fbk_bsi_distinct convention), decided before the output arena is allocated or a bit is scattered.  n_shards == 0,
 *    an empty filter or nothing in exists: FBK_OK, n_pos = n_neg = 0, the batch holds the one empty row.
 *  - The positions of one sign must lie within 2^23 consecutive shards, else FBK_E_INVALID (a field of small numbers with a few
 *    huge outliers is not a join key; fbk_bsi_distinct returns it as a list).  The window is [0, (2^bit_depth + |base|) >> 20] where
 *    that is within 2^23, else it comes from fbk_bsi_min / _max's kernel over exists ∩ filter (with values of both signs, whose
 *    windows would start at 0, one more walk finds each sign's smallest position if starting at 0 is too wide).
 *  - The output arena is (n_pos + n_neg + 1) * 2^17 bytes; if it cannot be allocated: FBK_E_NOMEM, the context stays usable.
 *    Scratch beyond it does not grow with the columns: the densify chunk (<= 2^28), two presence bitmaps (one bit per shard of the
 *    window and sign, <= 2^20 bytes each), their word prefixes, 12 bytes per output cell (run counts, cardinalities), row lists.
 *  - Two walks over the planes (presence of shards; scatter of bits, which reads a word before it ORs into it and issues no atomic
 *    for a bit already set).  OR commutes: the result does not depend on grid size, chunking or the order in which blocks run. */
int32_t fbk_bsi_distinct_rows(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, int64_t base,
                              const fbk_batch* filter, const uint32_t* rows_f, uint32_t n_shards, uint32_t flags, fbk_batch** out_batch,
                              uint64_t* out_shard_ids, uint64_t cap, uint32_t* out_n_pos, uint32_t* out_n_neg, uint64_t* out_counts);

/* TopK / TopN: totals[i] = sum over the shards of |A[shard][i] ∩ F[shard]| (of the stored row
 * cardinalities when filter == NULL), ordered on the device by count descending and row index
 * ascending inside one count, rows with a zero count dropped, at most k results (k = 0: all) —
 * executeTopK / doTopK (executor.go:2705-2774) with the order of BSIData.PivotDescending
 * (bsi.go:18-62); executeTopN / fragment.top (fragment.go:1317-1437) count the same intersections
 * (their rank-cache thresholds are approximations the device does not need).  rows_a is
 * [n_shards][n_a] (row i of every shard = the same field row), rows_f [n_shards].
 * out_index[j] = i, out_count[j] = totals[i]; *out_n = number of results, also when
 * FBK_E_CAPACITY reports that `cap` was too small.  Fields of more than 4096 rows are ordered by
 * a device radix sort and only the k winners cross the bus, not n_a counts (n_a <= 2^22). */
int32_t fbk_topk(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter,
                 const uint32_t* rows_f, uint32_t n_shards, uint32_t k, uint32_t* out_index, uint64_t* out_count, uint32_t cap,
                 uint32_t* out_n);

/* TopN (executeTopN, executor.go:2779-2864; per shard fragment.top, fragment.go:1317-1437).  Per shard s and row i,
 * cnt = the row's stored cardinality and count = |row ∩ F_s| (count = cnt without a filter = the `Src` row).  The row
 * QUALIFIES in that shard iff cnt != 0, count != 0 and
 *   tanimoto_threshold > 0 and a filter is given:
 *       src*T/100 < cnt < src*100/T   and   ceil(count*100 / (cnt + src - count)) > T     (:1334-1391;
 *       src = |F_s|, T = tanimoto_threshold, a percentage; evaluated in integer arithmetic, which equals
 *       the reference's float64 comparisons for every count a shard can hold)
 *   otherwise:  cnt >= min_threshold and count >= min_threshold                              (:1357, :1394;
 *       the caller passes what executeTopNShard passes: 0 there becomes defaultMinThreshold = 1, the same rule)
 * and totals[i] = the sum of count over the shards where row i qualifies (Pairs.Add, cache.go:463).
 *
 * n = 0 or n >= n_a: every row with a total is returned, ordered count descending / row index ascending.
 * 0 < n < n_a, option topn_semantics = 1 (DEFAULT): the reference's two passes.  Pass 1: per SHARD, fragment.top with
 *   N = n walks the rows in rank order (cnt descending; equal cnt: row index ascending) — the first n qualifying rows,
 *   and with a filter every later row whose cnt passes the cnt-level test and whose count reaches the smallest count of
 *   those n (the heap only grows, :1404-1425) — and the ids of all shards are merged, untrimmed (executeTopNShards
 *   :2829-2864).  Pass 2: the totals of exactly those candidates (:2812-2818), ordered, trimmed to n (:2823-2825).  A row
 *   outside every shard's own list is not returned even if its total would rank: that IS the reference's answer
 *   (TestExecutor_Execute_TopN_fill_small, tests/golden/executor_topn_vectors.json).  One kernel (k_topn_candidates,
 *   one block per shard, histogram selection — no sort) next to the counting the call does anyway.
 * 0 < n < n_a, topn_semantics = 0: the exact top n of totals.
 * The rank cache itself (cache.go: at most CacheSize rows per fragment, refreshed lazily) is not modelled: every row given
 * in rows_a is ranked.  fbk_topk (executeTopK, an exact operator in the reference too) is fbk_topn with both thresholds 0
 * and no candidate pass. */
int32_t fbk_topn(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter,
                 const uint32_t* rows_f, uint32_t n_shards, uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold,
                 uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n);

/* One member's share of a TopN for the one-process-per-GPU deployment (featurebase_amd/dist.py topn_reduce): totals[i] as
 * fbk_topn computes them over THIS context's shards and candidates[i] != 0 iff some shard here lists row i in pass 1
 * (without a candidate pass — n = 0, n >= n_a, topn_semantics = 0 — every row with a total).  The ranks all-reduce
 * [totals | candidates] (2 n_a words, ONE collective), drop the rows no rank flagged, order and trim: the same answer
 * as fbk_topn over all shards, however they are dealt.  n_shards = 0: zeros.  Both outputs hold n_a uint64. */
int32_t fbk_topn_partials(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter,
                          const uint32_t* rows_f, uint32_t n_shards, uint32_t n, uint64_t min_threshold, uint64_t tanimoto_threshold,
                          uint64_t* out_totals, uint64_t* out_candidates);

/* The TopK counts in the form executeTopKShard hands to its reducer: BSI planes over the ROW IDS
 * (bsiBuilder.Insert(rowID, count), bsi.go:251-284; merged across shards with AddBSI = fbk_bsi_add,
 * read back with PivotDescending, bsi.go:18-62).  totals[i] as in fbk_topk; out row p (p <
 * *out_depth = bits of the largest total) holds bit i iff bit p of totals[i] is set; row ids are the
 * indices i (n_a <= 2^20), container keys p * 16 + slot. */
int32_t fbk_topk_bsi(fbk_ctx* ctx, const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, const fbk_batch* filter,
                     const uint32_t* rows_f, uint32_t n_shards, uint32_t flags, fbk_batch** out_batch, uint32_t* out_depth);

/* out row i = rows[i] with the bits of the row-relative positions [start, end] (inclusive, 0 <= start
 * <= end < 2^20) negated: Bitmap.Flip (roaring/roaring.go:2769-2799); the container-level flip of the
 * reference's combination table (flipArray / flipBitmap / flipRun, roaring.go:6259-6274) is the
 * range of one slot.  No PQL call reaches Flip (Not is Difference(existence, row), executor.go:5554);
 * it completes the container algebra.  out_counts[i] = cardinality of out row i. */
int32_t fbk_flip(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, uint64_t n_rows, uint64_t start, uint64_t end,
                 uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts);

/* Shift: out row i = rows[i] with every column moved up by one — Row.Shift (row.go:374-396) /
 * RowSegment.Shift (:613-626) / Bitmap.Shift(1) (roaring/roaring.go:1629-1662; shiftArray,
 * shiftBitmap, shiftRun :6184-6257), which executeShiftShard (executor.go:5818-5836) applies n
 * times.  The reference lets the bit that leaves a shard's last column fall into a container
 * keyed one past the segment, which Row.Columns() reports as the first column of the next shard;
 * here that bit is handed over explicitly: carry_rows[i] (or NULL) names the row of the
 * PREVIOUS shard whose column ShardWidth-1 becomes column 0 of out row i.  Either index may be
 * FBK_NO_ROW: rows[i] absent (a shard that exists only to receive the carried bit), no
 * predecessor.  out_counts[i] = cardinality of out row i (rows left empty are nil containers). */
#define FBK_NO_ROW 0xFFFFFFFFu
int32_t fbk_shift(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, const uint32_t* carry_rows, uint64_t n_rows,
                  uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts);

/* Unsigned BSI addition z = x + y, plane by plane (ripple carry): roaring.Add
 * (roaring/add.go:12-849), which AddBSI (bsi.go:83-175) uses to merge per-shard TopK counts.
 * Group g of x is the depth_x rows rows_x[g*depth_x + i] (plane i = bit i, no exists / sign
 * planes), likewise y; out row g*(D+1) + i is plane i of the sum, D = max(depth_x, depth_y),
 * plane D holding the final carry.  Output container keys are out_row * 16 + slot (the fragment-storage
 * form rowID << 4 | slot with the output row ordinal as row id). */
int32_t fbk_bsi_add(fbk_ctx* ctx, const fbk_batch* x, const uint32_t* rows_x, uint32_t depth_x, const fbk_batch* y,
                    const uint32_t* rows_y, uint32_t depth_y, uint64_t n_groups, uint32_t flags, fbk_batch** out_batch);

/* out row s = columns of shard s whose value satisfies `op predicate` (fragment.rangeOp,
 * fragment.go:937-1208); the container keys of the result are s * 16 + slot. */
int32_t fbk_bsi_range(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                      int32_t op, uint32_t bit_depth, int64_t predicate, uint32_t flags, fbk_batch** out_batch,
                      uint64_t* out_counts);

/* Sum(Row(v op predicate), field = v) — the values of the columns that satisfy a range predicate on the SAME BSI
 * field, summed: executeSumCountShard (executor.go:2155) with the filter that executeRowBSIGroupShard (:5249) builds
 * from fragment.rangeOp.  The reference computes the range as a Row and then runs fragment.sum with that Row as the
 * filter (fragment.go:724-750): every bit plane is read twice.  Here one pass: a column that the MSB -> LSB scan
 * matches at plane i has the predicate's bits above i, so its high part is a constant per plane and its low planes
 * are still to come (k_bsi_range_sum_slot).  `filter` (optional, rows_f[s] per shard) restricts the
 * columns first, as Sum(Intersect(Row(v op k), <filter>), field = v).  out_sums[s] / out_counts[s] equal fbk_bsi_sum
 * with filter = fbk_bsi_range(op, predicate) (∩ filter) bit for bit; the reference's special forms (predicate 0,
 * saturated predicates, EQ / NEQ) run as exactly those two calls. */
int32_t fbk_bsi_range_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards, int32_t op,
                          uint32_t bit_depth, int64_t predicate, const fbk_batch* filter, const uint32_t* rows_f,
                          int64_t* out_sums, uint64_t* out_counts);

/* The per-plane schedule fbk_bsi_range_sum runs for (op, bit_depth, predicate) — host arithmetic only, no device:
 * out_actions[i] (64 entries) = what happens at plane i (0 sums only, 1 remaining &= plane, 2 remaining &= ~plane,
 * 3 matched |= remaining & plane, 4 matched |= remaining & ~plane), out_vhi[i] (64) = value of a column matched at
 * plane i above and at that plane, *out_scan_positive = the scanned sign class, *out_take_other = the other class
 * belongs to the result as a whole.  Returns 1 (not an error) when this predicate takes the two-pass path.  For
 * tests and for callers that want to know which path a query will take. */
int32_t fbk_bsi_range_sum_plan(int32_t op, uint32_t bit_depth, int64_t predicate, uint8_t* out_actions, uint64_t* out_vhi,
                               uint32_t* out_scan_positive, uint32_t* out_take_other);

/* Sum(Row(lo <= v <= hi), field = v): fbk_bsi_range_sum's two-sided form (fragment.rangeBetween + fragment.sum on the same
 * field; `filter` as there).  One pass over the planes for batches in the dense layout (fbk_batch_upload_dense) and
 * lo < hi within the field's range: two scan lanes — the positives up to hi and the negatives up to |lo|, or, for bounds of
 * one sign, the columns sharing the bounds' common prefix split at the highest differing bit into ">= lower" and
 * "<= upper" (k_bsi_between_sum_half); otherwise fbk_bsi_range_between + fbk_bsi_sum.  Totals equal those
 * two calls bit for bit.  fbk_bsi_between_sum_plan: the schedule (host arithmetic only; returns 1 for the two-pass path):
 * out_actions[2][64], out_vhi[2][64], out_split[64], out_vfin[2], out_flags[5] = {lane 0 positive, lane 1 positive,
 * lane 1 starts as its class, lane 0 whole class, lane 1 whole class}. */
int32_t fbk_bsi_range_between_sum(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows, uint32_t n_shards,
                                  uint32_t bit_depth, int64_t lo, int64_t hi, const fbk_batch* filter, const uint32_t* rows_f,
                                  int64_t* out_sums, uint64_t* out_counts);
int32_t fbk_bsi_between_sum_plan(uint32_t bit_depth, int64_t lo, int64_t hi, uint8_t* out_actions, uint64_t* out_vhi,
                                 uint8_t* out_split, uint64_t* out_vfin, uint32_t* out_flags);

/* lo <= value <= hi (fragment.rangeBetween, fragment.go:1213-1303). */
int32_t fbk_bsi_range_between(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* base_rows,
                              uint32_t n_shards, uint32_t bit_depth, int64_t lo, int64_t hi, uint32_t flags,
                              fbk_batch** out_batch, uint64_t* out_counts);

/* ---- a whole bitmap call tree in one launch ------------------------------------------------------
 * The filter of a query — Intersect(Union(Row(a=1), Row(a=2)), Not(Row(b=3)), Row(x > 5)), the tree that
 * executeBitmapCallShard (executor.go:1782) evaluates by recursion — as a list of LEAVES and a POSTFIX PROGRAM over them.
 * For each shard s the program is evaluated over that shard's row of every leaf, one wavefront per (shard, slot): the
 * intermediate values stay on chip, every leaf container is read once in its encoded form, the result is counted or written
 * once (k_expr_slot).
 *   leaf     kind FBK_EXPR_ROW: rows[s] = ordinal of the shard's row in `batch` (op, bit_depth, lo, hi unused);
 *            FBK_EXPR_BSI: rows[s] = base row of the shard's BSI fragment, the leaf is Row(v op lo) (fbk_bsi_range's row);
 *            FBK_EXPR_BETWEEN: Row(lo <= v <= hi) (fbk_bsi_range_between's row).  Leaves may come from different batches,
 *            a leaf may be pushed any number of times, an empty row is a leaf like any other.
 *   program  word = opcode << 24 | leaf index.  FBK_EXPR_PUSH pushes the leaf; FBK_EXPR_AND / _OR / _XOR / _ANDNOT pop b, pop
 *            a and push a op b (ANDNOT: a \ b).  Not(x) is written PUSH exists, <x>, ANDNOT (executeNotShard); Shift crosses
 *            containers and stays a call of its own (fbk_shift), its result enters as a ROW leaf.
 *   limits   FBK_EXPR_MAX_LEAVES leaves, FBK_EXPR_MAX_PROG words, FBK_EXPR_MAX_DEPTH values on the stack at once.  Anything
 *            beyond a limit, a stack underflow, more or fewer than one value left at the end, a leaf index >= n_leaves, an
 *            unknown opcode or leaf kind, bit_depth > 64, a NULL batch or n_prog == 0 is FBK_E_INVALID before anything is
 *            launched.  n_shards == 0 is FBK_OK with an empty result (fbk_expr_count, fbk_expr_eval); fbk_query_expr refuses it
 *            with FBK_E_INVALID, as fbk_query_fold and fbk_query_bsi_range refuse a query over nothing.
 *   fbk_expr_count   out_counts[s] = the cardinality of the result in shard s
 *   fbk_expr_eval    the result as row s of a new batch (the caller frees it); flags as fbk_fold_n: 0 = bitmap cells,
 *                    FBK_SETOP_OPTIMIZE = Container.optimize() applied and the arena compacted.  out_counts may be NULL.
 *                    Keys: row s carries the high key bits of the first pushed leaf's row, as a fold carries its first row's;
 *                    a program that starts with a BSI leaf has the default keys (s * 16 + slot), as fbk_bsi_range has.
 *   fbk_query_expr   the prepared form (contract of fbk_query_fold / fbk_query_bsi_range): row lists, leaf table and program
 *                    uploaded once, run = memset + ONE launch, read: out0 = uint64 cardinalities [n_shards];
 *                    fbk_query_output lends the row batch.  flags | FBK_EXPR_COUNT_ONLY: no row batch (fbk_query_output
 *                    fails), and only then fbk_query_run accepts device_out and FBK_QUERY_ACCUMULATE. */
#define FBK_EXPR_ROW 0u
#define FBK_EXPR_BSI 1u
#define FBK_EXPR_BETWEEN 2u
#define FBK_EXPR_PUSH 0u
#define FBK_EXPR_AND 1u
#define FBK_EXPR_OR 2u
#define FBK_EXPR_XOR 3u
#define FBK_EXPR_ANDNOT 4u
#define FBK_EXPR_MAX_LEAVES 256u
#define FBK_EXPR_MAX_PROG 1024u
#define FBK_EXPR_MAX_DEPTH 8u
#define FBK_EXPR_COUNT_ONLY 2u
typedef struct fbk_expr_leaf {
  const fbk_batch* batch;
  const uint32_t* rows; /* [n_shards] */
  uint32_t kind;        /* FBK_EXPR_ROW / _BSI / _BETWEEN */
  int32_t op;           /* FBK_BSI_* for FBK_EXPR_BSI */
  uint32_t bit_depth;
  uint32_t pad;
  int64_t lo, hi;       /* FBK_EXPR_BSI: lo is the predicate */
} fbk_expr_leaf;
int32_t fbk_expr_count(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                       uint32_t n_shards, uint64_t* out_counts);
int32_t fbk_expr_eval(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                      uint32_t n_shards, uint32_t flags, fbk_batch** out_batch, uint64_t* out_counts);
int32_t fbk_query_expr(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                       uint32_t n_shards, uint32_t flags, fbk_query** out_query);

/* Sum / Min / Max of an int field over a call tree, in the tree's own launch: SELECT SUM(x) ... WHERE <tree>.  The reference
 * evaluates the filter (executeSum / executeMin / executeMax, executor.go -> executeBitmapCallShard) and hands the Row to
 * fragment.sum / min / max (fragment.go:724-853); fbk_expr_eval followed by fbk_bsi_sum / _min / _max does the same with the
 * row written out and read back.  Here the filter stays in the wavefront's registers and the field's planes stream past it
 * (k_expr_agg_slot).  leaves / prog / n_shards and every tree error: as fbk_expr_count.  batch / base_rows /
 * bit_depth: the BSI field as fbk_bsi_sum takes it (it may be a leaf's own batch).  agg: FBK_AGG_SUM, _MIN or _MAX.
 *   out_vals[s], out_counts[s]   bit for bit what fbk_bsi_sum / fbk_bsi_min / fbk_bsi_max return for shard s with the tree's row
 *                    as their filter: Base not added, Sum wraps in uint64, (0, 0) where nothing qualifies.
 *   FBK_E_INVALID before anything is launched: a tree error, agg > 2, bit_depth > 64, a NULL batch, NULL base_rows or outputs
 *                    with n_shards > 0, base_rows[s] + bit_depth + 2 > the batch's rows, n_shards > 2^26.  n_shards == 0 is
 *                    FBK_OK; fbk_query_expr_bsi refuses it, as fbk_query_expr does.
 *   fbk_query_expr_bsi   the prepared form (contract of fbk_query_bsi_sum): everything uploaded once, run = memset + ONE launch,
 *                    read: out0 = int64 values [n_shards], out1 = uint64 counts [n_shards]; a leaf batch or the field batch
 *                    compacted since is picked up by the next run.  FBK_AGG_SUM leaves {psum, nsum, count} per shard (24 bytes,
 *                    uint64, all three additive with wrap-around): fbk_query_run accepts device_out, and FBK_QUERY_ACCUMULATE adds
 *                    a run to what the buffer holds.  _MIN / _MAX leave per-slot records only fbk_query_read folds: device_out
 *                    must be NULL and FBK_QUERY_ACCUMULATE is FBK_E_INVALID. */
#define FBK_AGG_SUM 0u
#define FBK_AGG_MIN 1u
#define FBK_AGG_MAX 2u
int32_t fbk_expr_bsi_agg(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                         uint32_t n_shards, uint32_t agg, const fbk_batch* batch, const uint32_t* base_rows, uint32_t bit_depth,
                         int64_t* out_vals, uint64_t* out_counts);
int32_t fbk_query_expr_bsi(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                           uint32_t n_shards, uint32_t agg, const fbk_batch* batch, const uint32_t* base_rows, uint32_t bit_depth,
                           fbk_query** out_query);

/* The counting operators over a call tree, in the tree's own launch: SELECT f, COUNT(*) ... WHERE <tree> GROUP BY f [ORDER BY
 * count DESC LIMIT k] — TopK(f, filter=<tree>), TopN(f, <tree>, n=), GroupBy(Rows(f), filter=<tree>).  The reference evaluates
 * the filter per shard (executeTopK / executeTopN -> executeBitmapCallShard) and counts every row of the field against it (doTopK,
 * executor.go:2705-2746; fragment.top, fragment.go:1317-1437); fbk_expr_eval followed by fbk_topk / fbk_topn / fbk_count_matrix
 * does the same with the filter row written out as 8 KiB cells and read back per block.  Here every block of the counting kernel
 * computes the filter container itself from the lowered tree and keeps it in LDS (k_expr_rows_vs_filter): one
 * upload for the tree, one for the field's rows, no output batch, one synchronisation.
 *   leaves / prog / n_shards and every tree error and limit: as fbk_expr_count (n_shards <= 2^26).
 *   a / rows_a / n_a   the field as fbk_topk takes it: rows_a[s * n_a + i] = row i of the field in shard s, n_a <= 2^22.
 *   fbk_expr_row_counts   out_total [n_a], out_per_shard [n_shards * n_a] or NULL, out_filter_counts [n_shards] or NULL: bit for
 *                    bit out_total / out_per_shard of fbk_count_matrix(a, rows_a, n_a, F, rows_f, 1, ...) with F the batch
 *                    fbk_expr_eval gives for the tree, and the counts of fbk_expr_count.  With out_per_shard all shards are one
 *                    pass (n_shards * n_a * 8 bytes on the device); a rank of a cluster reduces these with its peers' itself.
 *   fbk_expr_topk / fbk_expr_topn   bit for bit fbk_topk / fbk_topn with that F as the filter: ordering, zero counts dropped, k /
 *                    n = 0 for all, min_threshold, tanimoto_threshold (<= 100), option topn_semantics and its candidate pass, the
 *                    device sort past 4096 rows (option topk_device_sort), FBK_E_CAPACITY with *out_n = what is needed.
 *   FBK_E_INVALID before anything is launched, the context stays usable: a tree error, NULL a, NULL rows_a with n_a and n_shards
 *                    > 0, a row index past the batch, n_a > 2^22, n_shards > 2^26, a NULL output that is not optional.
 *   n_shards == 0    FBK_OK: zero totals (fbk_expr_row_counts), *out_n = 0.  n_a == 0: FBK_OK, nothing written but *out_n = 0.
 * Not offered: a prepared fbk_query_* form; fbk_topn_partials / fbk_group_topn over a tree (out_per_shard and out_total are what a
 * rank needs to reduce counts itself); k_expr_slot on the block-wide evaluator. */
int32_t fbk_expr_row_counts(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                            const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards, uint64_t* out_total,
                            uint64_t* out_per_shard, uint64_t* out_filter_counts);
int32_t fbk_expr_topk(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                      const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards, uint32_t k, uint32_t* out_index,
                      uint64_t* out_count, uint32_t cap, uint32_t* out_n);
int32_t fbk_expr_topn(fbk_ctx* ctx, const fbk_expr_leaf* leaves, uint32_t n_leaves, const uint32_t* prog, uint32_t n_prog,
                      const fbk_batch* a, const uint32_t* rows_a, uint32_t n_a, uint32_t n_shards, uint32_t n, uint64_t min_threshold,
                      uint64_t tanimoto_threshold, uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n);


/* fragment.rows(start, filters...) (fragment.go:2465-2486; executeRowsShard, executor.go:4077-4182): which of
 * the rows rows[0 .. n_rows) — the fragment's rows from `start` on, in ascending row-id order, one device row each
 * — hold anything, hold `column`, and fall under `limit`.  The reference streams the fragment's containers in key
 * order through the filter protocol of roaring/filter.go (BitmapRowFilter :371-469 over BitmapColumnFilter :226-249
 * and BitmapRowLimitFilter :471-509, ApplyFilterToIterator :1062-1085: skip-ahead by YesKey / NoKey so that a column
 * filter opens one container per row); here every row is examined at once (16 lanes read a row's 16 descriptors,
 * one lane probes the column's container) and the survivors are compacted in order.
 *   column  FBK_NO_COLUMN, or a column of the shard (0 .. 2^20 - 1): the row must contain it
 *   limit   0 = none (a PQL `limit=0` is NewBitmapRowLimitFilter(0), which ends the scan at once: the caller returns no
 *           rows without calling); else the reference's composition [column filter, limit filter]: the limit filter spends one
 *           of its rows on every row in which the scan looks at a container, matching or not.  Without a column
 *           that is every non-empty row (result: the first `limit` non-empty rows).  With a column the scan leaves a
 *           row r in which it saw the column's slot c (or a later one) by skipping to key (r + 1, c), so a row whose
 *           containers all lie below slot c is not counted when it directly follows (id + 1) such a row — the result
 *           is "the rows among the first `limit` COUNTED rows that contain the column".
 *   row_ids the fragment row ids of rows[0 .. n_rows), strictly ascending; required when a column AND a limit are
 *           given (the rule above needs to know which rows follow each other directly), otherwise may be NULL
 *   out_idx[cap]  positions (into rows[]) of the matching rows, ascending; *out_n = how many (FBK_E_CAPACITY when
 *           cap is too small: *out_n says how many there are). */
#define FBK_NO_COLUMN (~0ull)
int32_t fbk_rows(fbk_ctx* ctx, const fbk_batch* batch, const uint32_t* rows, const uint64_t* row_ids, uint64_t n_rows, uint64_t column,
                 uint64_t limit, uint32_t* out_idx, uint64_t cap, uint64_t* out_n);

/* ---- several GPUs in one process ---------------------------------------------------------------
 * The reference maps per-shard functions on the node that owns each shard and folds count-valued
 * results with an associative reduceFn in the same process (mapReduce / mapperLocal,
 * executor.go:6449-6533, 6742-6790; executeCount's reduceFn :5880; mergeGroupCounts :3728).  A
 * group is that for the GPUs of one node: one context per device (member m), shard s on member
 * s mod G, every member's work enqueued on its own stream so that the devices run concurrently, and
 * the partial counts reduced by one of
 *   FBK_REDUCE_HOST  G device->pinned-host copies of the partials and an add on the host
 *   FBK_REDUCE_PEER  one kernel on member 0 loading the other devices' partials over xGMI (peer access)
 *   FBK_REDUCE_RCCL  ncclAllReduce over single-process communicators (ncclCommInitAll); librccl is
 *                    dlopen'ed on first use, so libfbk.so itself links only the HIP runtime.
 * Bitmap-valued results are not exchanged (they stay per shard, executor.go:1767).  Data is made
 * resident and plans are created through the member contexts (fbk_group_member) with the ordinary
 * calls.  The same device ordinal may appear several times (members share the device): that is how
 * the G > 1 path is exercised on a one-GPU box; FBK_REDUCE_RCCL refuses such a group. */
typedef struct fbk_group fbk_group;
#define FBK_REDUCE_HOST 0
#define FBK_REDUCE_PEER 1
#define FBK_REDUCE_RCCL 2
int32_t fbk_group_open(const int32_t* devices, uint32_t n_devices, uint32_t flags, fbk_group** out_group);
int32_t fbk_group_close(fbk_group* group);
int32_t fbk_group_size(const fbk_group* group, uint32_t* out_n);
int32_t fbk_group_member(fbk_group* group, uint32_t i, fbk_ctx** out_ctx); /* borrowed: closed by fbk_group_close */
int32_t fbk_group_set_reduce(fbk_group* group, int32_t mode);

/* One step of Count(Intersect(Row, Row)) over the shards of all members: plans[m] (created on
 * member m over the shards it owns; NULL = none) runs as one launch per device with the per-device
 * sum fused, all devices concurrently; *out_total = sum over the members (executor.go:5871-5880). */
int32_t fbk_group_plan_intersection_count_total(fbk_group* group, fbk_plan* const* plans, uint64_t* out_total);

/* The count matrix of fbk_count_matrix over the shards of all members: per_member[m] are member m's
 * arguments (n_shards == 0: the member has no shard of this query), out_total[i * n_b + j] the sum
 * over every shard of every member (mergeGroupCounts across nodes, executor.go:3728). */
typedef struct fbk_matrix_args {
  const fbk_batch* a;
  const uint32_t* rows_a; /* [n_shards][n_a] */
  const fbk_batch* b;
  const uint32_t* rows_b; /* [n_shards][n_b] */
  const fbk_batch* filter; /* may be NULL */
  const uint32_t* rows_f; /* [n_shards] */
  uint32_t n_shards;
  uint32_t pad;
} fbk_matrix_args;
int32_t fbk_group_count_matrix(fbk_group* group, const fbk_matrix_args* per_member, uint32_t n_a, uint32_t n_b,
                               uint64_t* out_total);

/* Sum(field = v) over the shards of all members (executeSumCountShard, executor.go:2155, reduced by ValCount.Add
 * :8438): per_member[m] are member m's arguments of fbk_bsi_sum (n_shards == 0: none of its shards), each member
 * folds its shards on its device into {psum, nsum, count} and the three words are reduced over the members.
 * *out_sum = int64(psum) - int64(nsum) with uint64 wrap-around (roaring/filter.go:1103-1108) = the sum of
 * fbk_bsi_sum's out_sums over every shard of every member; *out_count likewise.  The caller adds count * Base. */
typedef struct fbk_bsi_args {
  const fbk_batch* batch;
  const uint32_t* base_rows; /* [n_shards] */
  const fbk_batch* filter;   /* may be NULL */
  const uint32_t* rows_f;    /* [n_shards] */
  uint32_t n_shards;
  uint32_t pad;
} fbk_bsi_args;
int32_t fbk_group_bsi_sum(fbk_group* group, const fbk_bsi_args* per_member, uint32_t bit_depth, int64_t* out_sum,
                          uint64_t* out_count);

/* TopN over the shards of all members: fbk_topn's answer over the union of the members' shards (the same two passes
 * under topn_semantics = 1, exact under 0), independent of how the shards are dealt — in the reference a node returns its
 * shards' merged pairs UNTRIMMED (executeTopNShards :2829-2864), the truncation to n happens per shard inside fragment.top.
 * Every member counts its shards and flags its shards' candidates; ONE reduce of [totals | candidate flags] (2 n_a words;
 * n_a without a candidate pass) over the members, then order and trim on the host.  per_member[m] are member m's
 * arguments of fbk_topn; outputs as fbk_topn.  The first member's topn_semantics decides for the group. */
typedef struct fbk_topn_args {
  const fbk_batch* a;
  const uint32_t* rows_a;  /* [n_shards][n_a] */
  const fbk_batch* filter; /* may be NULL */
  const uint32_t* rows_f;  /* [n_shards] */
  uint32_t n_shards;
  uint32_t pad;
} fbk_topn_args;
int32_t fbk_group_topn(fbk_group* group, const fbk_topn_args* per_member, uint32_t n_a, uint32_t n, uint64_t min_threshold,
                       uint64_t tanimoto_threshold, uint32_t* out_index, uint64_t* out_count, uint32_t cap, uint32_t* out_n);

/* The reduce alone, for count-valued partials the caller produced with the member contexts (BSI
 * sums, TopK counts, fold counts): device_partials[m] = `words` uint64 on member m's device (NULL =
 * zeros), produced on member m's stream. */
int32_t fbk_group_reduce_u64(fbk_group* group, void* const* device_partials, uint64_t words, uint64_t* out_total);

/* ---- one process per GPU: the exchange step issued by the library -------------------------------
 * The deployment of executor.go:6449-6533 on one node is one process per GPU, each with a context over the shards it
 * owns; the only exchange is the sum of count-valued partials (reduceFn).  Issued through PyTorch that all-reduce costs
 * the launching thread ~28 us per call (profiles/r06_collective_host_cost.json) — more than half of a 41 us headline step.
 * These calls put it on the library's side: a communicator per context over RCCL (dlopen'ed, as for fbk_group), created
 * from a unique id that rank 0 draws and the host code hands to the other ranks by whatever channel it has (the Go shim:
 * its cluster RPC; bench.py / featurebase_amd.dist: torch.distributed.broadcast_object_list).
 *   fbk_comm_unique_id      rank 0: 128 bytes (ncclGetUniqueId)
 *   fbk_comm_init           every rank: ncclCommInitRank on the context's device; collective (blocks until all ranks arrive)
 *   fbk_comm_all_reduce_u64 in place sum of n_words uint64 at device_words over the ranks, ASYNCHRONOUS: ordered after what
 *                           the context's stream holds at the call, run on the communicator's own stream, so the kernels
 *                           of the following queries overlap it.  The words must not be touched until a fence.
 *   fbk_comm_fence          the context's stream waits for every all-reduce enqueued so far (one event: no host wait)
 *   fbk_comm_close          destroys the communicator (fbk_close does it too) */
#define FBK_COMM_ID_BYTES 128
int32_t fbk_comm_unique_id(uint8_t* out_id /* FBK_COMM_ID_BYTES */);
int32_t fbk_comm_init(fbk_ctx* ctx, const uint8_t* id /* FBK_COMM_ID_BYTES */, int32_t n_ranks, int32_t rank);
int32_t fbk_comm_all_reduce_u64(fbk_ctx* ctx, void* device_words, uint64_t n_words);
int32_t fbk_comm_fence(fbk_ctx* ctx);
int32_t fbk_comm_close(fbk_ctx* ctx);

/* Message (and status code) of the last failing fbk_group_* call on THIS group, copied into a caller
 * buffer: the form a cgo binding must use (see fbk_last_error_r).  Group-level failures — argument
 * checks, "plan was not created on member m", peer / RCCL set-up, buffer growth — have no member
 * context to be recorded on; failures inside a member's enqueue are recorded on the group AND on that
 * member.  While a group call runs it holds every member's context lock (in member order) until the
 * member streams are synchronised, and a call that fails half-way drains the members it had enqueued. */
int32_t fbk_group_last_error_r(fbk_group* group, char* buf, uint64_t cap, int32_t* out_code);

#ifdef __cplusplus
}
#endif
#endif /* FBK_H */
