"""fbk_expr_* on the GPU: every generated call tree of tests/expr_gen.py through expr_count, expr_eval (with and without
FBK_SETOP_OPTIMIZE) and query_expr, against the numpy model AND against the chain of existing calls it replaces on the same
context (fbk_setop / fbk_fold_n / fbk_bsi_range / fbk_bsi_range_between, node by node): counts equal, downloaded bit content equal,
with optimize() the container encodings equal to those the chain's last call produced.  Then the named cases of the issue.  The
worlds are 1-3 shards; FBK_FUZZ_ITERS=<n> runs more iterations, FBK_TEST_SEED re-rolls them."""
import numpy as np
import pytest

import datagen as D
import expr_gen as G
from featurebase_amd import lib as L
from featurebase_amd import roaring as R

pytestmark = pytest.mark.gpu

OPC = {"and": L.OP_AND, "or": L.OP_OR, "xor": L.OP_XOR, "andnot": L.OP_ANDNOT, "not": L.OP_ANDNOT}


class Env:
    """a World resident on the device: batches "A", "B" (set rows) and "V" (the BSI fragments)"""

    def __init__(self, ctx, w):
        self.ctx, self.w = ctx, w
        self.batches = {name: ctx.upload([D.to_fbk_row(r) for r in w.rows[name]]) for name in ("A", "B")}
        rows = []
        for fr in w.frags:
            for r, bm in enumerate(fr.rows):
                rows.append({r * 16 + k: D.to_fbk(c) for k, c in bm.items() if c.n} if bm is not None else {})
        self.batches["V"] = ctx.upload(rows)
        self._leaves = {}

    def leaf(self, lf):
        if id(lf) not in self._leaves:
            self._leaves[id(lf)] = R.ExprLeaf(self.batches[lf.batch] if lf.has_batch else None, lf.rows, lf.kind, lf.op, lf.bit_depth, lf.lo, lf.hi)
        return self._leaves[id(lf)]

    def program(self, tree):
        leaves, prog = G.postfix(tree)
        return [self.leaf(lf) for lf in leaves], np.asarray(prog, dtype=np.uint32)

    def free(self):
        for b in self.batches.values():
            b.free()

    # -- the chain of existing calls ----------------------------------------------------------------------------------
    def chain(self, tree, flags=0):
        """(batch, rows, counts or None, owned): the tree node by node; `flags` go to the LAST call only"""
        ctx, n = self.ctx, self.w.n_shards
        if isinstance(tree, G.Leaf):
            if tree.kind == G.ROW:
                return self.batches[tree.batch], np.asarray(tree.rows, np.uint32), None, False
            if tree.kind == G.BSI:
                b, cnt = ctx.bsi_range(self.batches["V"], tree.rows, tree.op, tree.bit_depth, tree.lo, flags)
            else:
                b, cnt = ctx.bsi_range_between(self.batches["V"], tree.rows, tree.bit_depth, tree.lo, tree.hi, flags)
            return b, np.arange(n, dtype=np.uint32), cnt, True
        kids = tree[1:]
        if len(kids) >= 2 and all(isinstance(k, G.Leaf) and k.kind == G.ROW and k.batch == kids[0].batch for k in kids):
            groups = np.asarray([[k.rows[s] for k in kids] for s in range(n)], dtype=np.uint32)  # one level of plain rows: fbk_fold_n
            b, cnt = ctx.fold_n(OPC[tree[0]], self.batches[kids[0].batch], groups, flags)
            return b, np.arange(n, dtype=np.uint32), cnt, True
        acc = self.chain(kids[0], flags if len(kids) == 1 else 0)
        for i, k in enumerate(kids[1:]):
            rhs = self.chain(k)
            b, cnt = ctx.setop(OPC[tree[0]], acc[0], acc[1], rhs[0], rhs[1], flags if i == len(kids) - 2 else 0)
            for old in (acc, rhs):
                if old[3]:
                    old[0].free()
            acc = (b, np.arange(n, dtype=np.uint32), cnt, True)
        return acc

    def chain_result(self, tree, flags=0):
        """(rows downloaded, counts) of the chain; a tree that is one ROW leaf goes through a one-row fold (a copy)"""
        b, rows, cnt, owned = self.chain(tree, flags)
        if not owned:
            b, cnt = self.ctx.fold_n(L.OP_OR, b, rows.reshape(-1, 1), flags)
            rows = np.arange(self.w.n_shards, dtype=np.uint32)
        res = b.download()
        b.free()
        return [res[int(r)] for r in rows], np.asarray(cnt, dtype=np.uint64)


def words(rows):
    return np.stack([G.words_of_row(r) for r in rows])


def encodings(rows):
    return [{k & 15: (c.typ, c.n, np.asarray(c.data).tobytes()) for k, c in r.items() if c.n} for r in rows]


def check_tree(env, tree, what):
    ctx, w = env.ctx, env.w
    leaves, prog = env.program(tree)
    exp = w.model(tree)
    exp_cnt = G.popcount(exp)
    assert ctx.expr_count(leaves, prog).tolist() == exp_cnt.tolist(), what
    chain_rows, chain_cnt = env.chain_result(tree)
    assert chain_cnt.tolist() == exp_cnt.tolist(), what
    assert (words(chain_rows) == exp).all(), what
    out, cnt = ctx.expr_eval(leaves, prog)
    res = out.download()
    out.free()
    assert cnt.tolist() == exp_cnt.tolist(), what
    assert (words(res) == exp).all(), what
    assert all(c.typ == L.TYPE_BITMAP for r in res for c in r.values()), what  # flags 0: bitmap cells
    out, cnt = ctx.expr_eval(leaves, prog, L.SETOP_OPTIMIZE)
    res = out.download()
    out.free()
    chain_opt, _ = env.chain_result(tree, L.SETOP_OPTIMIZE)
    assert cnt.tolist() == exp_cnt.tolist(), what
    assert (words(res) == exp).all(), what
    assert encodings(res) == encodings(chain_opt), what
    for flags in (0, L.SETOP_OPTIMIZE):
        q = ctx.query_expr(leaves, prog, flags)
        q.run()
        assert q.read().tolist() == exp_cnt.tolist(), what
        got = q.output().download()
        assert (words(got) == exp).all(), what
        if flags:
            assert encodings(got) == encodings(chain_opt), what
        q.free()


@pytest.fixture(scope="module")
def B(oracle):
    from oracle import pybsi

    pybsi._lib()
    return pybsi


@pytest.mark.parametrize("it", range(G.ITERS))
def test_generated_trees(gpu_ctx, B, it):
    w = G.World(it)
    env = Env(gpu_ctx, w)
    try:
        check_tree(env, w.tree(), f"FBK_TEST_SEED={hex(D.SEED)} it={it}")
    finally:
        env.free()


@pytest.fixture(scope="module")
def env(gpu_ctx, B):
    e = Env(gpu_ctx, G.World(1))  # two shards, bit depth 1
    yield e
    e.free()


def test_single_push_is_a_copy(env):
    for lf in (env.w.a[0], env.w.empty, env.w.preds[0]):
        check_tree(env, lf, repr(lf))


def test_results_empty_everywhere_and_all_empty_leaves(env):
    w = env.w
    check_tree(env, ("and", w.a[0], w.empty), "x AND empty")
    check_tree(env, ("andnot", w.a[1], w.a[1]), "x ANDNOT x")
    check_tree(env, ("or", w.empty, ("xor", w.empty, w.empty)), "every leaf the empty row")
    # a shard whose every leaf is the empty row, next to a shard with content
    mixed = G.Leaf(G.ROW, "B", [w.empty.rows[0], w.b[1].rows[1]])
    mixed2 = G.Leaf(G.ROW, "B", [w.empty.rows[0], w.b[2].rows[1]])
    check_tree(env, ("or", mixed, mixed2), "one shard all empty")


def test_leaves_from_three_batches_and_repeated_leaves(env):
    w = env.w
    x = w.a[0]
    check_tree(env, ("and", ("or", x, w.b[1]), ("not", w.exists, w.a[3]), w.preds[0]), "three batches")
    check_tree(env, ("xor", x, x), "x XOR x")
    check_tree(env, ("and", x, x), "x AND x")
    leaves, prog = env.program(("xor", x, x))
    assert env.ctx.expr_count(leaves, prog).tolist() == [0] * w.n_shards
    leaves, prog = env.program(("and", x, x))
    assert env.ctx.expr_count(leaves, prog).tolist() == G.popcount(w.leaf_words(x)).tolist()


def test_compile_expr_helper(env):
    """the nested-tuple helper of the package gives the program the tests' own postfix gives"""
    w = env.w
    a, b, c, e, p = (env.leaf(x) for x in (w.a[1], w.a[2], w.a[3], w.exists, w.preds[1]))
    tree = ("and", ("or", a, b), ("not", e, c), p)
    leaves, prog = R.compile_expr(tree)
    mirror = ("and", ("or", w.a[1], w.a[2]), ("not", w.exists, w.a[3]), w.preds[1])
    assert prog.tolist() == G.postfix(mirror)[1] and len(leaves) == 5
    assert env.ctx.expr_count(leaves, prog).tolist() == G.popcount(w.model(mirror)).tolist()


def test_output_keys_are_those_the_existing_calls_give(env):
    """FULL container keys, not only the slot: a tree that starts with a row carries that row's high key bits as fbk_fold_n
    carries its first row's; a tree that starts with a predicate has the default keys of fbk_bsi_range."""
    w, ctx = env.w, env.ctx

    def keys(batch):
        rows = batch.download()
        batch.free()
        return [sorted(r) for r in rows]

    rows3 = [w.a[3], w.a[1], w.a[2]]  # the first leaf is row 3 of every shard: high bits (s * RA + 3) << 4
    leaves, prog = env.program(("or", *rows3))
    groups = np.asarray([[lf.rows[s] for lf in rows3] for s in range(w.n_shards)], dtype=np.uint32)
    got = keys(ctx.expr_eval(leaves, prog, L.SETOP_OPTIMIZE)[0])
    assert got == keys(ctx.fold_n(L.OP_OR, env.batches["A"], groups, L.SETOP_OPTIMIZE)[0])
    assert all(k >> 4 == w.a[3].rows[s] for s in range(w.n_shards) for k in got[s]) and any(got)
    q = ctx.query_expr(leaves, prog, L.SETOP_OPTIMIZE)
    q.run()
    assert [sorted(r) for r in q.output().download()] == got
    q.free()
    p = w.preds[0]
    leaves, prog = env.program(("and", p, w.exists))
    chain = p.kind == G.BSI and ctx.bsi_range(env.batches["V"], p.rows, p.op, p.bit_depth, p.lo)[0] or ctx.bsi_range_between(env.batches["V"], p.rows, p.bit_depth, p.lo, p.hi)[0]
    exp = w.model(("and", p, w.exists))
    got = keys(ctx.expr_eval(leaves, prog)[0])
    want = keys(chain)  # (the predicate alone: same default keys wherever both have a container)
    for s in range(w.n_shards):
        assert got[s] == [s * 16 + slot for slot in range(16) if exp[s, slot].any()]
        assert set(got[s]) <= set(want[s])


def test_union_of_64_rows_equals_union_n(env):
    w, ctx = env.w, env.ctx
    pool = w.a + w.b
    picks = [pool[i % len(pool)] for i in range(64)]
    a_only = [w.a[i % G.RA] for i in range(64)]
    check_tree(env, ("or", *picks), "64-way union over two batches")
    leaves, prog = env.program(("or", *a_only))
    out, cnt = ctx.expr_eval(leaves, prog, L.SETOP_OPTIMIZE)
    groups = np.asarray([[lf.rows[s] for lf in a_only] for s in range(w.n_shards)], dtype=np.uint32)
    ref, ref_cnt = ctx.union_n(env.batches["A"], groups, L.SETOP_OPTIMIZE)
    got, exp = out.download(), ref.download()
    out.free()
    ref.free()
    assert cnt.tolist() == ref_cnt.tolist()
    assert {k: (c.typ, c.n, c.data.tobytes()) for r in got for k, c in r.items()} == {k: (c.typ, c.n, c.data.tobytes()) for r in exp for k, c in r.items()}


def test_depth_limit_and_every_saved_value(env):
    """A program exactly at FBK_EXPR_MAX_DEPTH runs; so does the tree that needs the most saved values the limit admits (a complete
    tree of NEQ predicates: every leaf's own scan saves one more, FBK_EXPR_MAX_DEPTH in all); one value more is FBK_E_INVALID."""
    w, ctx = env.w, env.ctx
    t = w.a[0]
    for i in range(G.MAX_DEPTH - 1):
        t = (["and", "or", "xor", "andnot"][i % 4], w.a[(i + 1) % G.RA], t)
    assert G.stack_depth(G.postfix(t)[1]) == G.MAX_DEPTH
    check_tree(env, t, "at the depth limit")
    level = [G.Leaf(G.BSI, "V", w.base, 2, w.depth, (i % 5) - 2, 0) for i in range(1 << (G.MAX_DEPTH - 1))]
    ops = ["or", "xor", "and", "andnot"]
    d = 0
    while len(level) > 1:
        level = [(ops[(d + i) % 4], level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
        d += 1
    leaves, prog = env.program(level[0])
    assert G.stack_depth(prog.tolist()) == G.MAX_DEPTH
    exp = w.model(level[0])
    assert ctx.expr_count(leaves, prog).tolist() == G.popcount(exp).tolist()
    out, _ = ctx.expr_eval(leaves, prog)
    res = out.download()
    out.free()
    assert (words(res) == exp).all()
    leaves, prog = env.program(w.a[0])
    deep = np.asarray([(G.PUSH << 24)] * (G.MAX_DEPTH + 1) + [G.OR << 24] * G.MAX_DEPTH, dtype=np.uint32)
    with pytest.raises(L.FbkError) as e:
        ctx.expr_count(leaves, deep)
    assert e.value.code == L.FBK_E_INVALID and "FBK_EXPR_MAX_DEPTH" in str(e.value)
    assert ctx.expr_count(leaves, prog).tolist() == G.popcount(w.leaf_words(w.a[0])).tolist()  # the context is still usable


def test_malformed_programs_through_the_abi(env):
    w, ctx = env.w, env.ctx
    good_leaves, good_prog = env.program(("and", w.a[0], w.a[1]))
    want = ctx.expr_count(good_leaves, good_prog).tolist()
    limit_names = {"max_depth": "FBK_EXPR_MAX_DEPTH", "max_prog": "FBK_EXPR_MAX_PROG", "max_leaves": "FBK_EXPR_MAX_LEAVES"}
    for tag, leaves, prog in G.malformed(w):
        ls, pr = [env.leaf(lf) for lf in leaves], np.asarray(prog, dtype=np.uint32)
        calls = [lambda: ctx.expr_count(ls, pr, n_shards=w.n_shards), lambda: ctx.expr_eval(ls, pr, 0, n_shards=w.n_shards),
                 lambda: ctx.query_expr(ls, pr, 0, n_shards=w.n_shards), lambda: ctx.query_expr(ls, pr, 0, count_only=True, n_shards=w.n_shards)]
        for call in calls:
            with pytest.raises(L.FbkError) as e:
                call()
            assert e.value.code == L.FBK_E_INVALID, tag
            if tag in limit_names:
                assert limit_names[tag] in str(e.value), (tag, str(e.value))
        assert ctx.expr_count(good_leaves, good_prog).tolist() == want, tag  # nothing was launched, nothing is broken
    # rows past the batch, fragments past the batch
    with pytest.raises(L.FbkError):
        ctx.expr_count([R.row_leaf(env.batches["A"], [10 ** 6] * w.n_shards)], [G.PUSH << 24])
    with pytest.raises(L.FbkError):
        ctx.expr_count([R.bsi_leaf(env.batches["V"], [w.base[-1] + 1] * w.n_shards, L.BSI_GT, w.depth, 0)], [G.PUSH << 24])
    with pytest.raises(L.FbkError):
        ctx.expr_eval(good_leaves, good_prog, 4)  # unknown flags
    # no shards: FBK_OK with an empty result; the prepared form refuses a query over nothing, as its neighbours do
    for count_only in (False, True):
        with pytest.raises(L.FbkError) as e:
            ctx.query_expr(good_leaves, good_prog, 0, count_only=count_only, n_shards=0)
        assert e.value.code == L.FBK_E_INVALID
    assert ctx.expr_count(good_leaves, good_prog, n_shards=0).size == 0
    out, cnt = ctx.expr_eval(good_leaves, good_prog, n_shards=0)
    assert out.n_rows == 0 and cnt.size == 0
    out.free()


def test_prepared_form(env, B):
    w, ctx = env.w, env.ctx
    tree = ("and", ("or", w.a[1], w.a[2]), ("not", w.exists, w.a[3]), w.preds[2])
    leaves, prog = env.program(tree)
    exp = w.model(tree)
    exp_cnt = G.popcount(exp).tolist()
    q = ctx.query_expr(leaves, prog, L.SETOP_OPTIMIZE)
    with pytest.raises(L.FbkError):
        q.output()  # before the first run
    q.run()
    first = (q.read().tolist(), encodings(q.output().download()))
    q.run()
    assert (q.read().tolist(), encodings(q.output().download())) == first and first[0] == exp_cnt
    # the borrowed output is a valid filter of fbk_bsi_sum
    sums, counts = ctx.bsi_sum(env.batches["V"], w.base, w.depth, q.output(), np.arange(w.n_shards, dtype=np.uint32))
    for s in range(w.n_shards):
        bits = np.unpackbits(exp[s].reshape(-1).view(np.uint8), bitorder="little")
        inside = [v for c, v in w.values[s].items() if bits[c]]
        assert (int(sums[s]), int(counts[s])) == (sum(inside), len(inside)), s
    for bad in (lambda: q.run(accumulate=True), lambda: q.run(device_ptr=q.result_ptr()[0])):
        with pytest.raises(L.FbkError):
            bad()
    q.free()
    # count only: no row output; accumulating a second run doubles the counts
    qc = ctx.query_expr(leaves, prog, count_only=True)
    qc.run()
    assert qc.read().tolist() == exp_cnt
    with pytest.raises(L.FbkError):
        qc.output()
    qc.run(accumulate=True)
    assert qc.read().tolist() == [2 * c for c in exp_cnt]
    qc.run()
    assert qc.read().tolist() == exp_cnt
    qc.free()
