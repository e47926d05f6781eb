// fbk_group_field.inc — the host frame of the GroupBy aggregates over an int field (fbk_count_matrix_sum, _distinct, _minmax,
// _quantiles): the call's twelve operand arguments as one struct, and its four dense operands (A rows, B rows, the filter row, the
// BSI fragment) walked a chunk of shards at a time.  Included by fbk.hip after fbk_dense_operands.inc.

namespace {

struct GroupFieldArgs {  // filled at the ABI entry; checked by msum_args_ok (fbk_matrix_sum_api.inc)
  const fbk_batch* a;
  const uint32_t* rows_a;
  uint32_t n_a;
  const fbk_batch* b;  // nullptr: the one-field form (n_b == 1)
  const uint32_t* rows_b;
  uint32_t n_b;
  const fbk_batch* filter;  // nullptr: no filter
  const uint32_t* rows_f;
  const fbk_batch* bsi;
  const uint32_t* base_rows;
  uint32_t bit_depth, n_shards;
  uint64_t width() const { return uint64_t(n_a) * n_b; }
};

struct GroupFieldViews {  // what the kernels take for one chunk
  DenseView A, B, F, S;
};

struct GroupFieldOperands {
  DenseOperands ops;
  int A = 0, B = 0, F = 0, S = 0;  // the operands' numbers in ops
  uint32_t n_a = 0, n_b = 0, depth = 0, n_shards = 0;

  // depth: the planes the kernels read (the fragment's exists and sign rows come with them).  The chunk is the caller's rule over
  // ops.densified_rows(), so it is taken between add() and upload().
  void add(const GroupFieldArgs& g, uint32_t depth_read) {
    n_a = g.n_a, n_b = g.n_b, depth = depth_read, n_shards = g.n_shards;
    A = ops.add(g.a, g.rows_a, g.n_a), B = ops.add(g.b, g.rows_b, g.n_b), F = ops.add(g.filter, g.rows_f, 1);
    S = ops.add(g.bsi, g.base_rows, depth_read + 2, true);
  }
  int32_t upload(fbk_ctx* ctx, uint32_t chunk) { return ops.upload(ctx, n_shards, chunk); }

  GroupFieldViews views(uint32_t s0) const { return {ops.view(A, s0), ops.view(B, s0), ops.view(F, s0), ops.view(S, s0)}; }

  // fn(views, s0, ns) for every chunk [s0, s0 + ns) of the shards, densified in one launch (DenseOperands::for_each_chunk)
  template <class Fn>
  void for_each_chunk(fbk_ctx* ctx, bool first_walk, Fn fn) {
    ops.for_each_chunk(ctx, first_walk, DenseOperands::Densify::together, [&](uint32_t s0, uint32_t ns) { fn(views(s0), s0, ns); });
  }

  // blocks of a group_column_walk launch (fbk_group_walk.hip.h) over ns shards: four units of kGroupWalkWords words a block
  static uint32_t walk_grid(uint32_t ns) {
    const uint64_t units = uint64_t(ns) * (fbk::kGroupRowWords / fbk::kGroupWalkWords);
    return uint32_t(std::min<uint64_t>((units + 3) / 4, fbk::kGroupWalkBlocks));
  }

  // a kernel whose parameters are FBK_GROUP_PARAMS and then its own tail, over the ns shards of a chunk's views
  template <class Kernel, class... Tail>
  void launch(Kernel kernel, dim3 grid, size_t lds, fbk_ctx* ctx, const GroupFieldViews& v, uint32_t ns, Tail... tail) const {
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, ctx->stream, v.A.arena, v.A.rows, n_a, v.B.arena, v.B.rows, n_b, v.F.arena, v.F.rows, v.S.arena, v.S.rows, depth,
                       ns, tail...);
  }
};

}  // namespace
