"""fbk_expr_bsi_agg / fbk_query_expr_bsi on the GPU: Sum, Min and Max of an int field over every generated call tree of
tests/expr_gen.py, in the tree's own launch, against the numpy model of tests/expr_agg_gen.py AND against the two calls they replace
on the same context (fbk_expr_eval, then fbk_bsi_sum / fbk_bsi_min / fbk_bsi_max with that row as the filter): values and counts
exactly equal per shard.  Then the named cases of the issue.  The worlds are 1-3 shards; FBK_FUZZ_ITERS=<n> runs more iterations,
FBK_TEST_SEED re-rolls them."""
import ctypes as C

import numpy as np
import pytest

import datagen as D
import expr_agg_gen as A
import expr_gen as G
import test_gpu_expr as TE
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu

PUSH0 = np.asarray([G.PUSH << 24], dtype=np.uint32)


class Env(TE.Env):
    """test_gpu_expr.Env plus the second fragment, batch "W" """

    def __init__(self, ctx, w):
        super().__init__(ctx, w)
        rows = []
        for fr in w.fields["W"].frags:
            for r, bm in enumerate(fr.rows):
                rows.append({r * 16 + k: D.to_fbk(c) for k, c in bm.items() if c.n} if bm is not None else {})
        self.batches["W"] = ctx.upload(rows)

    def field(self, name):
        f = self.w.fields[name]
        return self.batches[name], np.asarray(f.base, dtype=np.uint32), f.depth


def two_calls(env, agg, leaves, prog, name):
    """what the fused call replaces: the tree's row, then the aggregate with that row as its filter"""
    ctx = env.ctx
    batch, base, depth = env.field(name)
    filt, _ = ctx.expr_eval(leaves, prog)
    fn = {A.SUM: ctx.bsi_sum, A.MIN: ctx.bsi_min, A.MAX: ctx.bsi_max}[agg]
    vals, counts = fn(batch, base, depth, filt, np.arange(env.w.n_shards, dtype=np.uint32))
    filt.free()
    return vals.tolist(), counts.tolist()


def check_tree(env, tree, name, what):
    ctx, w = env.ctx, env.w
    leaves, prog = env.program(tree)
    batch, base, depth = env.field(name)
    for agg in A.AGGS:
        exp = w.model_agg(agg, tree, name)
        vals, counts = ctx.expr_bsi_agg(agg, leaves, prog, batch, base, depth)
        assert (vals.tolist(), counts.tolist()) == exp, (what, agg)
        assert two_calls(env, agg, leaves, prog, name) == exp, (what, agg)
        q = ctx.query_expr_bsi(agg, leaves, prog, batch, base, depth)
        q.run()
        v, c = q.read()
        q.free()
        assert (v.tolist(), c.tolist()) == exp, (what, agg)


@pytest.fixture(scope="module")
def B(oracle):
    from oracle import pybsi

    pybsi._lib()
    return pybsi


@pytest.mark.parametrize("it", range(G.ITERS))
def test_generated_trees_times_three_aggregates(gpu_ctx, B, it):
    w = A.World(it)
    env = Env(gpu_ctx, w)
    try:
        check_tree(env, w.tree(), w.agg_field, f"FBK_TEST_SEED={hex(D.SEED)} it={it} field={w.agg_field}")
    finally:
        env.free()


@pytest.fixture(scope="module")
def env(gpu_ctx, B):
    e = Env(gpu_ctx, A.World(4))  # two shards; V of bit depth 5, W of bit depth 12
    yield e
    e.free()


def test_single_push_of_a_row_leaf_equals_the_filtered_aggregates(env):
    w, ctx = env.w, env.ctx
    for lf in (w.a[0], w.exists, w.empty):
        for name in ("W", "V"):
            batch, base, depth = env.field(name)
            for agg, fn in ((A.SUM, ctx.bsi_sum), (A.MIN, ctx.bsi_min), (A.MAX, ctx.bsi_max)):
                vals, counts = ctx.expr_bsi_agg(agg, [env.leaf(lf)], PUSH0, batch, base, depth)
                ev, ec = fn(batch, base, depth, env.batches[lf.batch], lf.rows)
                assert (vals.tolist(), counts.tolist()) == (ev.tolist(), ec.tolist()) == w.model_agg(agg, lf, name), (repr(lf), name, agg)


def test_sum_over_a_predicate_of_the_same_field_equals_range_sum(env):
    w, ctx = env.w, env.ctx
    batch, base, depth = env.field("V")
    some = sorted(w.values[0].values())
    for op in G.BSI_OPS:
        for pred in (some[len(some) // 2], -3, 0):
            lf = G.Leaf(G.BSI, "V", w.base, op, depth, pred, 0)
            vals, counts = ctx.expr_bsi_sum([env.leaf(lf)], PUSH0, batch, base, depth)
            ev, ec = ctx.bsi_range_sum(batch, base, op, depth, pred)
            assert (vals.tolist(), counts.tolist()) == (ev.tolist(), ec.tolist()) == w.model_agg(A.SUM, lf, "V"), (op, pred)


def test_depth_0_and_depth_64(gpu_ctx, B):
    for it, depth in ((5, 0), (2, 64)):  # W's depth is DEPTHS[(it + 1) % 6]
        w = A.World(it)
        assert w.wdepth == depth
        e = Env(gpu_ctx, w)
        try:
            tree = ("or", w.exists, w.a[0])
            check_tree(e, tree, "W", f"depth {depth}")
            leaves, prog = e.program(tree)
            batch, base, _ = e.field("W")
            inside = G.popcount(w.model(tree) & w.exists_words("W")).tolist()
            sums, counts = gpu_ctx.expr_bsi_sum(leaves, prog, batch, base, depth)
            assert counts.tolist() == inside and all(inside)
            if depth == 0:  # nothing but the existence of a value: Sum 0 over |filter ∩ exists| columns, Min and Max (0, count)
                assert sums.tolist() == [0] * w.n_shards
                for fn in (gpu_ctx.expr_bsi_min, gpu_ctx.expr_bsi_max):
                    v, c = fn(leaves, prog, batch, base, 0)
                    assert (v.tolist(), c.tolist()) == ([0] * w.n_shards, inside)
            else:  # tens of thousands of 63-bit magnitudes in shard 0's full slot, all negative: nsum wraps uint64 (check_tree compared it)
                cols, mag, neg = w.fields["W"].data[0]
                bits = np.unpackbits(w.model(tree)[0].reshape(-1).view(np.uint8), bitorder="little")[cols].astype(bool)
                assert sum(int(x) for x in mag[bits & neg]) >= 1 << 64
        finally:
            e.free()


def test_tree_that_fills_every_saved_slot_then_the_aggregate(env):
    """the complete tree of NEQ predicates of test_gpu_expr (FBK_EXPR_MAX_DEPTH values saved at once): the aggregate's plane loads
    decode through the scratch below that stack"""
    w = env.w
    level = [G.Leaf(G.BSI, "V", w.base, 2, w.depth, (i % 5) - 2, 0) for i in range(1 << (G.MAX_DEPTH - 1))]
    ops = ["or", "xor", "and", "andnot"]
    d = 0
    while len(level) > 1:
        level = [(ops[(d + i) % 4], level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
        d += 1
    assert G.stack_depth(G.postfix(level[0])[1]) == G.MAX_DEPTH
    check_tree(env, level[0], "W", "every saved slot, W")
    for name in ("W", "V"):  # (that tree alone may well be empty: a row on top of it, applied to the accumulator directly)
        tree = ("xor", level[0], w.exists)
        assert G.stack_depth(G.postfix(tree)[1]) == G.MAX_DEPTH and all(w.model_agg(A.SUM, tree, name)[1])
        check_tree(env, tree, name, "every saved slot, then a row, " + name)


def last_error(ctx):
    buf, code = C.create_string_buffer(1024), C.c_int32()
    L.check(ctx.lib.fbk_last_error_r(ctx.h, buf, 1024, C.byref(code)))
    return code.value, buf.value.decode()


def test_malformed_arguments(env):
    w, ctx, lib = env.w, env.ctx, env.ctx.lib
    n = w.n_shards
    batch, base, depth = env.field("W")
    good_leaves, good_prog = env.program(("and", w.a[0], w.exists))
    want = [x.tolist() for x in ctx.expr_bsi_sum(good_leaves, good_prog, batch, base, depth)]
    arr, nl, pr, _ = ctx._expr_args(good_leaves, good_prog, None)
    vals, counts = np.zeros(n, np.int64), np.zeros(n, np.uint64)
    past = np.asarray([batch.n_rows - depth - 1] * n, dtype=np.uint32)  # base + bit_depth + 2 = the batch's rows + 1
    many = (1 << 26) + 1
    h = C.c_void_p()

    def one_shot(n_shards=n, agg=A.SUM, b=batch.h, br=base.ctypes.data, d=depth, ov=vals.ctypes.data, oc=counts.ctypes.data, leaves=arr, n_leaves=nl, prog=pr):
        return lib.fbk_expr_bsi_agg(ctx.h, leaves, n_leaves, prog.ctypes.data, prog.size, n_shards, agg, b, br, d, ov, oc)

    def prepared(n_shards=n, agg=A.SUM, b=batch.h, br=base.ctypes.data, d=depth, leaves=arr, n_leaves=nl, prog=pr, **_):
        return lib.fbk_query_expr_bsi(ctx.h, leaves, n_leaves, prog.ctypes.data, prog.size, n_shards, agg, b, br, d, C.byref(h))

    bad = [("agg", dict(agg=3)), ("agg", dict(agg=0xFFFFFFFF)), ("bit_depth", dict(d=65)), ("batch", dict(b=None)), ("base_rows", dict(br=None)),
           ("fragment past the batch", dict(br=past.ctypes.data)), ("shards", dict(n_shards=many))]
    for tag, leaves, prog in G.malformed(w):  # every tree error, as fbk_expr_count reports it
        ls = ctx._expr_args([env.leaf(lf) for lf in leaves], np.asarray(prog, dtype=np.uint32), n)
        bad.append((tag, dict(leaves=ls[0], n_leaves=ls[1], prog=ls[2])))
    for tag, kw in bad:
        for call in (one_shot, prepared):
            assert call(**kw) == L.FBK_E_INVALID, (tag, call.__name__)
            code, msg = last_error(ctx)
            assert code == L.FBK_E_INVALID and msg, (tag, call.__name__)
        assert not h.value
        assert [x.tolist() for x in ctx.expr_bsi_sum(good_leaves, good_prog, batch, base, depth)] == want, tag  # the context is still usable
    for kw in (dict(ov=None), dict(oc=None)):  # (the prepared form has no outputs)
        assert one_shot(**kw) == L.FBK_E_INVALID and last_error(ctx)[1]
    # no shards: FBK_OK for the one-shot call (the tree is still checked), refused by the prepared form
    assert one_shot(n_shards=0, br=None, ov=None, oc=None) == L.FBK_OK
    assert one_shot(n_shards=0, prog=np.asarray([G.AND << 24], dtype=np.uint32)) == L.FBK_E_INVALID
    assert prepared(n_shards=0) == L.FBK_E_INVALID and last_error(ctx)[1] and not h.value
    assert [x.tolist() for x in ctx.expr_bsi_sum(good_leaves, good_prog, batch, base, depth)] == want


def test_prepared_form(gpu_ctx, B):
    import torch

    w = A.World(4)
    env = Env(gpu_ctx, w)  # its own batches: two of them are compacted below
    ctx = gpu_ctx
    try:
        tree = ("and", ("or", w.a[1], w.a[2], w.exists), ("not", w.exists, w.a[3]), w.preds[2])
        if not any(w.model_agg(A.SUM, tree, "W")[1]):
            tree = ("or", w.a[0], w.exists)
        leaves, prog = env.program(tree)
        batch, base, depth = env.field("W")
        exp = {agg: w.model_agg(agg, tree, "W") for agg in A.AGGS}
        assert any(exp[A.SUM][1])
        qs = {agg: ctx.query_expr_bsi(agg, leaves, prog, batch, base, depth) for agg in A.AGGS}
        for agg, q in qs.items():
            with pytest.raises(L.FbkError):
                q.read()  # before the first run
            for _ in range(2):  # two runs, equal results
                q.run()
                v, c = q.read()
                assert (v.tolist(), c.tolist()) == exp[agg], agg
        # a leaf batch and the field batch move: the next run reads them where they are now
        env.batches["A"].compact()
        batch.compact()
        for agg, q in qs.items():
            q.run()
            v, c = q.read()
            assert (v.tolist(), c.tolist()) == exp[agg], agg
        # Sum: {psum, nsum, count} per shard in a caller's buffer, a second run accumulated on top doubles all three
        cell = torch.zeros(3 * w.n_shards, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        qs[A.SUM].run(cell.data_ptr())
        v, c = qs[A.SUM].read()
        assert (v.tolist(), c.tolist()) == exp[A.SUM]
        qs[A.SUM].run(cell.data_ptr(), accumulate=True)
        v, c = qs[A.SUM].read()
        assert v.tolist() == [A.to_int64(2 * x) for x in exp[A.SUM][0]] and c.tolist() == [2 * x for x in exp[A.SUM][1]]
        raw = cell.cpu().numpy().view(np.uint64).reshape(-1, 3)
        assert raw[:, 2].tolist() == [2 * x for x in exp[A.SUM][1]]
        qs[A.SUM].run()  # back to its own buffer, overwritten
        v, c = qs[A.SUM].read()
        assert (v.tolist(), c.tolist()) == exp[A.SUM]
        # Min / Max: per-slot records, neither redirected nor accumulated
        for agg in (A.MIN, A.MAX):
            for bad in (lambda: qs[agg].run(cell.data_ptr()), lambda: qs[agg].run(accumulate=True), lambda: qs[agg].run(qs[agg].result_ptr()[0])):
                with pytest.raises(L.FbkError) as e:
                    bad()
                assert e.value.code == L.FBK_E_INVALID
            qs[agg].run()
            v, c = qs[agg].read()
            assert (v.tolist(), c.tolist()) == exp[agg]
        for q in qs.values():
            q.free()
    finally:
        env.free()
