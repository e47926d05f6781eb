"""fbk_expr_row_counts / fbk_expr_topk / fbk_expr_topn on the GPU: the counting operators over every generated call tree of
tests/expr_gen.py, in the tree's own launch, against the numpy model of tests/expr_rows_gen.py AND against the pair of calls they
replace on the same context (fbk_expr_eval, then fbk_count_matrix with that row as the single B row / fbk_topk / fbk_topn with it as
the filter): exactly equal.  Then the named cases of the issue.  The worlds are 1-3 shards, the field 1 to 200 rows of a pool of 40;
FBK_FUZZ_ITERS=<n> runs more iterations, FBK_TEST_SEED re-rolls them."""
import ctypes as C

import numpy as np
import pytest

import datagen as D
import expr_gen as G
import expr_rows_gen as RG
import test_gpu_expr as TE
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu

PUSH0 = np.asarray([G.PUSH << 24], dtype=np.uint32)


class Env(TE.Env):
    """test_gpu_expr.Env plus the pool of the field's rows, batch "F" """

    def __init__(self, ctx, w):
        super().__init__(ctx, w)
        self.batches["F"] = ctx.upload([D.to_fbk_row(r) for r in w.pool])

    def shards(self):
        return np.arange(self.w.n_shards, dtype=np.uint32)


def row_counts(env, leaves, prog, rows):
    tot, per, fc = env.ctx.expr_row_counts(leaves, prog, env.batches["F"], rows, per_shard=True, filter_counts=True)
    return tot.tolist(), per.tolist(), fc.tolist()


def pair_counts(env, leaves, prog, rows):
    """what the fused call replaces: the tree's row, then count_matrix with that row as its single B row"""
    ctx = env.ctx
    filt, fc = ctx.expr_eval(leaves, prog)
    tot, per = ctx.count_matrix(env.batches["F"], rows, filt, env.shards().reshape(-1, 1), per_shard=True)
    filt.free()
    return np.asarray(tot).reshape(-1).tolist(), np.asarray(per).reshape(rows.shape).tolist(), fc.tolist()


def check_counts(env, tree, n_as, what):
    w = env.w
    leaves, prog = env.program(tree)
    for n_a in n_as:
        rows = w.field(n_a)
        tot, per, fc = w.model_counts(tree, rows)
        exp = (tot.tolist(), per.tolist(), fc.tolist())
        assert row_counts(env, leaves, prog, rows) == exp, (what, n_a)
        assert pair_counts(env, leaves, prog, rows) == exp, (what, n_a)
        assert env.ctx.expr_row_counts(leaves, prog, env.batches["F"], rows).tolist() == exp[0], (what, n_a)  # totals alone: passes by option


@pytest.fixture(scope="module")
def B(oracle):
    from oracle import pybsi

    pybsi._lib()
    return pybsi


@pytest.mark.parametrize("it", range(G.ITERS))
def test_generated_trees_times_five_field_sizes(gpu_ctx, B, it):
    w = RG.World(it)
    env = Env(gpu_ctx, w)
    try:
        check_counts(env, w.tree(), RG.N_AS, f"FBK_TEST_SEED={hex(D.SEED)} it={it}")
    finally:
        env.free()


@pytest.fixture(scope="module")
def env(gpu_ctx, B):
    e = Env(gpu_ctx, RG.World(4))  # two shards, bit depth 5
    yield e
    e.free()


_checker = {}


def lowered_reads(tree, tmp_path):
    if "exe" not in _checker:  # (built once: the stand-alone planner check of tests/test_expr_cpu.py)
        _checker["exe"] = G.build_checker(str(tmp_path / "expr_plan_check_san"))
    checker = _checker["exe"]
    line = G.run_checker(checker, [G.postfix(tree)], str(tmp_path / "corpus.txt"))[0]
    assert line[0] == "OK"
    return RG.operand_reads([int(x) for x in line[5:]])


def test_block_shapes_the_cases_rely_on(gpu_ctx, B, tmp_path):
    """n_a = 200 under a 3-leaf tree: 4 blocks per (shard, slot), the last with 8 rows; n_a = 65 under a 64-plane predicate: the
    tree is too long to evaluate twice, one block whose 64-row loop runs twice (the Python restatement of the rule; the library's
    own is checked against it in test_expr_rows_cpu.py)"""
    for it in (0, 1, 2):  # 1, 2 and 3 shards
        w = RG.World(it)
        e = Env(gpu_ctx, w)
        try:
            three = ("and", ("or", w.a[1], w.a[2]), w.exists)
            assert lowered_reads(three, tmp_path) == 3 and RG.chunks_of(200, w.n_shards, 3) == (4, 8)
            check_counts(e, three, (200,), f"three leaves, {w.n_shards} shards")
        finally:
            e.free()
    w = RG.World(3)  # bit depth 64, one shard
    assert w.depth == 64
    e = Env(gpu_ctx, w)
    try:
        wide = ("and", G.Leaf(G.BETWEEN, "V", w.base, 0, 64, -5, 1 << 40), w.exists)
        Lw = lowered_reads(wide, tmp_path)
        assert Lw > 65 and RG.rows_per_block(65, w.n_shards, Lw) == 128 and RG.chunks_of(65, w.n_shards, Lw) == (1, 65)
        assert RG.chunks_of(65, w.n_shards, 3) == (2, 1)  # (a short tree splits the same field)
        check_counts(e, wide, (65,), "64 planes")
    finally:
        e.free()


def topk_pair(env, leaves, prog, rows, k):
    filt, _ = env.ctx.expr_eval(leaves, prog)
    idx, cnt = env.ctx.topk(env.batches["F"], rows, k, filt, env.shards())
    filt.free()
    return idx.tolist(), cnt.tolist()


def topn_pair(env, leaves, prog, rows, n, mt, tt):
    filt, _ = env.ctx.expr_eval(leaves, prog)
    idx, cnt = env.ctx.topn(env.batches["F"], rows, n, filt, env.shards(), mt, tt)
    filt.free()
    return idx.tolist(), cnt.tolist()


@pytest.mark.parametrize("it", [0, 1, 2, 4, 5])
def test_topk_and_topn_equal_the_pair(gpu_ctx, B, it):
    w = RG.World(it)
    e = Env(gpu_ctx, w)
    ctx = gpu_ctx
    try:
        trees = [w.tree(), ("or", w.a[0], w.a[1], w.exists), ("and", ("or", w.a[1], w.a[2]), w.exists)]
        for ti, tree in enumerate(trees):
            leaves, prog = e.program(tree)
            for n_a in (5, 65, 200):
                rows = w.field(n_a)
                totals = w.model_counts(tree, rows)[0]
                for sort in (0, 1):
                    ctx.set_option("topk_device_sort", sort)
                    for k in (0, 1, 5, n_a):
                        got = ctx.expr_topk(leaves, prog, e.batches["F"], rows, k)
                        got = (got[0].tolist(), got[1].tolist())
                        assert got == RG.top_of(totals, k), (it, ti, n_a, sort, k)
                        assert got == topk_pair(e, leaves, prog, rows, k), (it, ti, n_a, sort, k)
                    for sem in (0, 1):
                        ctx.set_option("topn_semantics", sem)
                        for n in (0, 3):
                            for mt in (0, 2):
                                for tt in (0, 30):
                                    got = ctx.expr_topn(leaves, prog, e.batches["F"], rows, n, mt, tt)
                                    assert (got[0].tolist(), got[1].tolist()) == topn_pair(e, leaves, prog, rows, n, mt, tt), (it, ti, n_a, sort, sem, n, mt, tt)
    finally:
        ctx.set_option("topk_device_sort", -1)
        ctx.set_option("topn_semantics", 1)
        e.free()


def test_several_passes_over_the_shards(gpu_ctx, B):
    """option matrix_pass_kb = 1: one shard per pass — the tree's leaves are indexed by the call's shard, the field's rows and the
    counts by the pass's"""
    w = RG.World(2)  # three shards
    assert w.n_shards == 3
    e = Env(gpu_ctx, w)
    try:
        tree = ("or", ("and", w.a[1], w.exists), w.a[2])
        leaves, prog = e.program(tree)
        rows = w.field(200)
        tot, per, fc = w.model_counts(tree, rows)
        gpu_ctx.set_option("matrix_pass_kb", 1)
        got = gpu_ctx.expr_row_counts(leaves, prog, e.batches["F"], rows, filter_counts=True)
        assert (got[0].tolist(), got[1].tolist()) == (tot.tolist(), fc.tolist())
        for n, mt, tt in ((0, 0, 0), (3, 2, 30)):
            a = gpu_ctx.expr_topn(leaves, prog, e.batches["F"], rows, n, mt, tt)
            assert (a[0].tolist(), a[1].tolist()) == topn_pair(e, leaves, prog, rows, n, mt, tt), (n, mt, tt)
    finally:
        gpu_ctx.set_option("matrix_pass_kb", 1 << 20)
        e.free()


def test_result_empty_in_one_shard(env):
    """a tree whose result is empty in shard 1 only: no counts from it, src = 0"""
    w = env.w
    only0 = G.Leaf(G.ROW, "B", [w.exists.rows[0], w.empty.rows[1]])
    tree = ("and", ("or", w.a[0], w.exists), only0)
    leaves, prog = env.program(tree)
    rows = w.field(65)
    tot, per, fc = w.model_counts(tree, rows)
    assert fc[0] > 0 and fc[1] == 0 and not per[1].any() and per[0].any()
    check_counts(env, tree, (65,), "empty in shard 1")
    got = env.ctx.expr_topn(leaves, prog, env.batches["F"], rows, 0, 0, 30)
    assert (got[0].tolist(), got[1].tolist()) == topn_pair(env, leaves, prog, rows, 0, 0, 30)


def test_existence_row_with_full_slots(gpu_ctx, B):
    """a tree equal to a row of 16 full containers: every block takes the f_full path (the stored counts answer)"""
    w = RG.World(4)
    rid = [s * G.RB for s in range(w.n_shards)]
    for s in range(w.n_shards):
        w.rows["B"][rid[s]] = {rid[s] * 16 + slot: D.oracle_container(w.rng, "run_full") for slot in range(16)}
    e = Env(gpu_ctx, w)
    try:
        for tree in (w.exists, ("or", w.exists, w.a[0]), ("not", w.exists, w.empty)):
            assert (G.popcount(w.model(tree)) == 1 << 20).all()
            check_counts(e, tree, (1, 65, 200), "full slots")
    finally:
        e.free()


def test_single_push_of_a_row_leaf_equals_topk_with_that_row(env):
    w, ctx = env.w, env.ctx
    rows = w.field(200)
    for lf in (w.a[0], w.a[3], w.exists, w.empty):
        got = ctx.expr_topk([env.leaf(lf)], PUSH0, env.batches["F"], rows, 5)
        exp = ctx.topk(env.batches["F"], rows, 5, env.batches[lf.batch], np.asarray(lf.rows, np.uint32))
        assert (got[0].tolist(), got[1].tolist()) == (exp[0].tolist(), exp[1].tolist()) == RG.top_of(w.model_counts(lf, rows)[0], 5), repr(lf)
        check_counts(env, lf, (65,), repr(lf))


def test_tree_that_fills_every_saved_slot(env):
    """the complete tree of NEQ predicates of test_gpu_expr_agg (FBK_EXPR_MAX_DEPTH values saved at once: 64 KiB of dynamic LDS on
    top of the block's own 20 KiB)"""
    w = env.w
    level = [G.Leaf(G.BSI, "V", w.base, 2, w.depth, (i % 5) - 2, 0) for i in range(1 << (G.MAX_DEPTH - 1))]
    ops = ["or", "xor", "and", "andnot"]
    d = 0
    while len(level) > 1:
        level = [(ops[(d + i) % 4], level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
        d += 1
    assert G.stack_depth(G.postfix(level[0])[1]) == G.MAX_DEPTH
    check_counts(env, level[0], (65,), "every saved slot")
    tree = ("xor", level[0], w.exists)  # (that tree alone may well be empty: a row on top of it)
    assert all(w.model_counts(tree, w.field(1))[2])
    check_counts(env, tree, (65, 200), "every saved slot, then a row")


def test_between_and_bit_depths_0_and_64(gpu_ctx, B):
    for it, depth in ((0, 0), (3, 64), (4, 5)):
        w = RG.World(it)
        assert w.depth == depth
        e = Env(gpu_ctx, w)
        try:
            lim = (1 << min(depth, 63)) - 1
            for lf in (G.Leaf(G.BETWEEN, "V", w.base, 0, depth, -lim, lim), G.Leaf(G.BETWEEN, "V", w.base, 0, depth, 0, lim // 2),
                       G.Leaf(G.BSI, "V", w.base, 6, depth, 0, 0), G.Leaf(G.BSI, "V", w.base, 2, depth, 1, 0)):
                check_counts(e, ("or", lf, w.a[1]), (65,), f"depth {depth} {lf!r}")
                check_counts(e, lf, (5,), f"depth {depth} {lf!r} alone")
        finally:
            e.free()


def test_array_leaf_of_over_4096_values(gpu_ctx, B):
    w = RG.World(0)
    big = w.rows["A"][0][0]  # shard 0, row 0, slot 0: array_dense_runs
    assert big.typ == 1 and big.n > 4096
    e = Env(gpu_ctx, w)
    try:
        for tree in (w.a[0], ("and", w.exists, w.a[0]), ("xor", w.a[0], w.a[1])):
            check_counts(e, tree, (1, 200), "array of over 4096 values")
    finally:
        e.free()


def last_error(ctx):
    buf, code = C.create_string_buffer(1024), C.c_int32()
    L.check(ctx.lib.fbk_last_error_r(ctx.h, buf, 1024, C.byref(code)))
    return code.value, buf.value.decode()


def test_malformed_arguments(env):
    w, ctx, lib = env.w, env.ctx, env.ctx.lib
    n, n_a = w.n_shards, 65
    F = env.batches["F"]
    rows = w.field(n_a)
    good_leaves, good_prog = env.program(("and", w.a[0], w.exists))
    want = row_counts(env, good_leaves, good_prog, rows)
    want_top = RG.top_of(np.asarray(want[0]), 0)
    arr, nl, pr, _ = ctx._expr_args(good_leaves, good_prog, None)
    tot, per, fc = np.zeros(n_a, np.uint64), np.zeros(n * n_a, np.uint64), np.zeros(n, np.uint64)
    idx, cnt, got = np.zeros(n_a, np.uint32), np.zeros(n_a, np.uint64), C.c_uint32()
    past = rows.copy()
    past[-1, -1] = F.n_rows
    many_rows, many_shards = (1 << 22) + 1, (1 << 26) + 1

    def counts(a=F.h, ra=rows.ctypes.data, na=n_a, n_shards=n, leaves=arr, n_leaves=nl, prog=pr, ot=tot.ctypes.data, **_):
        return lib.fbk_expr_row_counts(ctx.h, leaves, n_leaves, prog.ctypes.data, prog.size, a, ra, na, n_shards, ot, per.ctypes.data, fc.ctypes.data)

    def topk(a=F.h, ra=rows.ctypes.data, na=n_a, n_shards=n, leaves=arr, n_leaves=nl, prog=pr, cap=n_a, oi=idx.ctypes.data, on=C.byref(got), **_):
        return lib.fbk_expr_topk(ctx.h, leaves, n_leaves, prog.ctypes.data, prog.size, a, ra, na, n_shards, 0, oi, cnt.ctypes.data, cap, on)

    def topn(a=F.h, ra=rows.ctypes.data, na=n_a, n_shards=n, leaves=arr, n_leaves=nl, prog=pr, cap=n_a, oi=idx.ctypes.data, on=C.byref(got), tt=0, **_):
        return lib.fbk_expr_topn(ctx.h, leaves, n_leaves, prog.ctypes.data, prog.size, a, ra, na, n_shards, 0, 0, tt, oi, cnt.ctypes.data, cap, on)

    def still_good(tag):
        assert row_counts(env, good_leaves, good_prog, rows) == want, tag
        t = ctx.expr_topk(good_leaves, good_prog, F, rows)
        assert (t[0].tolist(), t[1].tolist()) == want_top, tag

    bad = [("NULL a", dict(a=None)), ("NULL rows_a", dict(ra=None)), ("row past the batch", dict(ra=past.ctypes.data)), ("n_a", dict(na=many_rows)),
           ("shards", dict(n_shards=many_shards))]
    for tag, leaves, prog in G.malformed(w):  # every tree error, as fbk_expr_count reports it
        ls = ctx._expr_args([env.leaf(lf) for lf in leaves], np.asarray(prog, dtype=np.uint32), n)
        bad.append((tag, dict(leaves=ls[0], n_leaves=ls[1], prog=ls[2])))
    for tag, kw in bad:
        for call in (counts, topk, topn):
            assert call(**kw) == L.FBK_E_INVALID, (tag, call.__name__)
            code, msg = last_error(ctx)
            assert code == L.FBK_E_INVALID and msg, (tag, call.__name__)
        still_good(tag)
    for call, kw in ((counts, dict(ot=None)), (topk, dict(on=None)), (topn, dict(on=None)), (topk, dict(oi=None)), (topn, dict(tt=101))):
        assert call(**kw) == L.FBK_E_INVALID and last_error(ctx)[1], (call.__name__, kw)
    # buffers too small: FBK_E_CAPACITY, *out_n = what is needed
    assert len(want_top[0]) > 2
    for call in (topk, topn):
        got.value = 0
        assert call(cap=2) == L.FBK_E_CAPACITY, call.__name__
        assert got.value == len(want_top[0]) and last_error(ctx)[0] == L.FBK_E_CAPACITY
        still_good("capacity")
    # no shards: FBK_OK (the tree is still checked), zero totals / no results; no rows: FBK_OK, nothing written
    tot[:] = 7
    assert counts(n_shards=0, ra=None) == L.FBK_OK and not tot.any()
    got.value = 9
    assert topk(n_shards=0, ra=None) == L.FBK_OK and got.value == 0
    assert counts(n_shards=0, prog=np.asarray([G.AND << 24], dtype=np.uint32)) == L.FBK_E_INVALID
    tot[:] = 7
    assert counts(na=0, ra=None, ot=None) == L.FBK_OK and counts(na=0) == L.FBK_OK and (tot == 7).all()
    got.value = 9
    assert topn(na=0, ra=None, cap=0, oi=None) == L.FBK_OK and got.value == 0
    still_good("the end")


def test_leaf_batch_compacted_between_two_calls(gpu_ctx, B):
    w = RG.World(4)
    e = Env(gpu_ctx, w)  # its own batches: two of them are compacted below
    try:
        tree = ("and", ("or", w.a[1], w.a[2], w.exists), ("not", w.exists, w.a[3]))
        leaves, prog = e.program(tree)
        rows = w.field(200)
        tot, per, fc = w.model_counts(tree, rows)
        exp = (tot.tolist(), per.tolist(), fc.tolist())
        assert any(exp[0]) and row_counts(e, leaves, prog, rows) == exp
        e.batches["A"].compact()
        e.batches["F"].compact()
        assert row_counts(e, leaves, prog, rows) == exp
        t = gpu_ctx.expr_topk(leaves, prog, e.batches["F"], rows, 5)
        assert (t[0].tolist(), t[1].tolist()) == RG.top_of(tot, 5)
    finally:
        e.free()
