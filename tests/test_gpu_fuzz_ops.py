"""Structural fuzz of the calls that read their operands through the shared dense-operand walk (DenseOperands): fbk_bsi_sort and
fbk_extract_open_columns, fbk_extract_open / _span / _columns / _bsi / _rows, fbk_bsi_quantiles / _percentile, fbk_count_matrix_sum and
its prepared form, fbk_count_matrix_distinct, fbk_bsi_distinct_rows and fbk_bsi_distinct, fbk_count_matrix_minmax under every path
pin with and without counts, fbk_bsi_moments and fbk_count_cube.  The per-operator tests are thorough on
values and regular on structure; this file is the other way round.  tests/fuzz_ops_gen.py makes the cases (a pool of rows of every
container archetype uploaded twice, encoded and dense; arbitrary row lists into it; every operand draws its batch) and the
expectations (the numpy references); tests/test_fuzz_ops_cpu.py checks both without a GPU.  Everything is integer and bit-exact.

test_short_last_chunk_*: one deterministic call per walk whose shards do not divide evenly over the densify chunks (the ordinary case
in production: 33 shards at 31 per chunk are dealt 17 + 16), with a dense operand among the encoded ones, so that everything that
depends on a chunk's first shard differs between the first chunk and the last.

FBK_FUZZ_ITERS=<n> runs more iterations, FBK_TEST_SEED re-rolls them (scripts/fuzz_parity.sh)."""
import numpy as np
import pytest

import distinct_rows_ref as DR
import extract_ref as X
import fuzz_ops_gen as G
import minmax_ref as MM
import pct_ref as P
import sort_ref as SR
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu
ITERS = G.ITERS


class Uploaded:
    """the pool of a case on the device, encoded and dense; of(name) = the batch the operand draws"""

    def __init__(self, ctx, case):
        self.case = case
        self.enc = ctx.upload(case.pool.fbk_rows())
        self.dense = ctx.upload_dense(case.W)

    def of(self, name):
        return self.enc if self.case.enc[name] else self.dense

    def free(self):
        self.enc.free()
        self.dense.free()


def filter_args(up, c):
    return (up.of("filter"), c.rows_f) if c.rows_f is not None else (None, None)


def check_optimized(O, res):
    """FBK_SETOP_OPTIMIZE: every container has the encoding Container.optimize() picks for its content"""
    for row in res:
        for c in row.values():
            oc = O.optimize(O.OContainer.bitmap(c.words()))
            assert c.n and c.typ == oc.typ and c.n == oc.n
            assert np.array_equal(np.asarray(c.data).reshape(-1), np.asarray(oc.data()).reshape(-1))


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_sort_and_open_columns(gpu_ctx, oracle, it):
    c = G.Case("sort", it)
    rng = c.rng
    up = Uploaded(gpu_ctx, c)
    try:
        bS, (bF, rf) = up.of("bsi"), filter_args(up, c)
        for desc in (False, True):
            for keep_zero in (False, True):
                total = c.sort_expected(desc, keep_zero, 0, 0)[2]
                offset, limit = c.pick_cut(total, False), c.pick_cut(total, True)
                cap = int(rng.integers(0, 8)) if rng.random() < 0.3 else None  # too small: the capacity protocol, then the retry
                what = (c, "desc", desc, "keep_zero", keep_zero, "offset", offset, "limit", limit, "cap", cap)
                cols, vals, tot = gpu_ctx.bsi_sort(bS, c.base_rows, c.depth, c.shard_ids, bF, rf, desc, keep_zero, offset, limit, cap)
                ec, ev, et = c.sort_expected(desc, keep_zero, offset, limit)
                assert tot == et, what
                assert np.array_equal(cols, ec), what
                assert np.array_equal(vals, ev), what
        # the winners, in the sort's order, as the selection of an Extract
        desc, keep_zero = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
        offset, limit = int(rng.integers(0, 50)), int(rng.integers(1, 3000))
        what = (c, "winners", desc, keep_zero, offset, limit)
        cols, vals, _ = gpu_ctx.bsi_sort(bS, c.base_rows, c.depth, c.shard_ids, bF, rf, desc, keep_zero, offset, limit)
        ec, ev, _ = c.sort_expected(desc, keep_zero, offset, limit)
        assert np.array_equal(cols, ec) and np.array_equal(vals, ev), what
        h, rank = gpu_ctx.extract_columns(cols, c.shard_ids)
        with h:
            asc = np.sort(cols)
            assert np.array_equal(asc[rank], cols) and np.array_equal(h.columns(), asc), what
            hv, hp = h.bsi(bS, c.base_rows, c.depth)
            assert hp.all() and np.array_equal(hv[rank], vals), what
            sh, pos = c.locate(asc)
            offs, items = h.rows(up.of("a"), c.rows_a)
            eo, ei = X.rows_expected(c.A, sh, pos)
            assert np.array_equal(offs, eo) and np.array_equal(items, ei), what
    finally:
        up.free()


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_extract(gpu_ctx, it):
    c = G.Case("extract", it)
    rng = c.rng
    up = Uploaded(gpu_ctx, c)
    handles = []
    try:
        bF = up.of("filter")
        total = c.total
        cuts = [(c.pick_cut(total, False), int(rng.integers(1, 5000))), (0, None if total <= 20000 else 20000),
                (int(rng.integers(0, total + 1)), int(rng.integers(0, 300)))]
        perm = rng.permutation(c.n_sh)  # the third handle: the same filter rows dealt to other shards
        for k, (offset, limit) in enumerate(cuts):
            rows_f = c.rows_f[perm] if k == 2 else c.rows_f
            h = gpu_ctx.extract(bF, rows_f, c.shard_ids, offset, limit)
            handles.append((h, X.select(c.W[rows_f], c.shard_ids, offset, limit), (c, "offset", offset, "limit", limit, "handle", k)))
        # several handles alive, used alternately
        for h, (sh, pos, cols), what in handles:
            assert h.n == cols.size, what
            assert h.span() == ((int(sh.min()), int(sh.max() - sh.min() + 1)) if sh.size else (0, 0)), what
        for h, (sh, pos, cols), what in handles:
            assert np.array_equal(h.columns(), cols), what
        ev = [X.bsi_expected(c.S, c.depth, sh, pos) for _, (sh, pos, _), _ in handles]
        for (h, _, what), (vals, pres) in zip(reversed(handles), reversed(ev)):
            gv, gp = h.bsi(up.of("bsi"), c.base_rows, c.depth)
            assert np.array_equal(gp, pres) and np.array_equal(gv, vals), what
        for h, (sh, pos, cols), what in handles:
            cap = int(rng.integers(0, 4)) if rng.random() < 0.3 else None
            offs, items = h.rows(up.of("a"), c.rows_a, cap)
            eo, ei = X.rows_expected(c.A, sh, pos)
            assert np.array_equal(offs, eo) and np.array_equal(items, ei), what
    finally:
        for h, _, _ in handles:
            h.close()
        up.free()


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_quantiles_percentile(gpu_ctx, it):
    c = G.Case("quantiles", it)
    rng = c.rng
    up = Uploaded(gpu_ctx, c)
    try:
        bS, (bF, rf) = up.of("bsi"), filter_args(up, c)
        vals = c.values
        n = vals.size
        assert n == c.total
        some = [int(x) for x in rng.integers(0, n + 3, 6)]
        ranks = [0, 1, max(n - 1, 0), n, n + 5, G.TOP | 0, G.TOP | 1, G.TOP | max(n - 1, 0), G.TOP | n] + some + some[:3] + [G.TOP | k for k in some]
        ranks = [ranks[i] for i in rng.permutation(len(ranks))]
        gv, gc, gn = gpu_ctx.bsi_quantiles(bS, c.base_rows, c.depth, ranks, bF, rf)
        ev, ec, en = P.quantiles(vals, ranks)
        assert gn == en == n, c
        assert np.array_equal(gv, ev) and np.array_equal(gc, ec), (c, ranks)
        gv, gc, gn = gpu_ctx.bsi_quantiles(bS, c.base_rows, c.depth, [], bF, rf)  # the count alone
        assert gn == n and gv.size == 0, c
        base = c.percentile_base()
        nth = [0.0, 100.0, 50.0] + [float(x) for x in rng.uniform(0, 100, 5)] + [float(rng.integers(0, 101))]
        gv, gc, gn = gpu_ctx.bsi_percentile(bS, c.base_rows, c.depth, nth, base, bF, rf)
        assert gn == n, c
        for i, p in enumerate(nth):
            e = P.replay_on(vals, p, base)
            assert (int(gv[i]), int(gc[i])) == ((e[0], e[1]) if e is not None else (0, 0)), (c, "nth", p, "base", base, e)
        if n == 0:
            assert not gc.any()
    finally:
        up.free()


def _groupby_args(up, c):
    bF, rf = filter_args(up, c)
    return (up.of("a"), c.rows_a, up.of("b") if c.rows_b is not None else None, c.rows_b, up.of("bsi"), c.base_rows, c.depth, bF, rf)


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_groupby_sum(gpu_ctx, it):
    c = G.Case("groupby_sum", it)
    up = Uploaded(gpu_ctx, c)
    q = None
    try:
        args = _groupby_args(up, c)
        es, ec = c.msum_expected()
        sums, counts = gpu_ctx.count_matrix_sum(*args)
        assert np.array_equal(counts, ec), c
        assert np.array_equal(sums, es), c
        q = gpu_ctx.query_count_matrix_sum(*args)
        for _ in range(2):
            q.run()
            qs, qc = q.read()
            assert np.array_equal(qc, ec) and np.array_equal(qs, es), (c, "prepared")
        # the all-ones row (and column): Sum over the filter alone
        ts, tc = gpu_ctx.bsi_sum(up.of("bsi"), c.base_rows, c.depth, *filter_args(up, c))
        assert int(counts[c.i_full, c.j_full]) == int(tc.sum()) == c.total, c
        assert int(sums[c.i_full, c.j_full]) & ((1 << 64) - 1) == int(ts.view(np.uint64).sum(dtype=np.uint64)), c
    finally:
        if q is not None:
            q.free()
        up.free()


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_groupby_distinct(gpu_ctx, it):
    c = G.Case("groupby_distinct", it)
    up = Uploaded(gpu_ctx, c)
    try:
        args = _groupby_args(up, c)
        ed, ec = c.mdist_expected()
        dist, counts = gpu_ctx.count_matrix_distinct(*args)
        assert np.array_equal(counts, ec), c
        assert np.array_equal(dist, ed), c
        # without out_counts
        cargs, keep, n_shards, n_a, n_b = gpu_ctx._msum_args(args[0], args[1], args[2], args[3], args[4], args[5], args[7], args[8])
        alone = np.zeros((n_a, n_b), dtype=np.uint64)
        L.check(gpu_ctx.lib.fbk_count_matrix_distinct(*cargs, c.depth, n_shards, alone.ctypes.data, None))
        del keep
        assert np.array_equal(alone, ed), (c, "no out_counts")
        # the all-ones row (and column) is Distinct over the filter alone
        listed = gpu_ctx.bsi_distinct(up.of("bsi"), c.base_rows, c.depth, *filter_args(up, c))
        assert int(dist[c.i_full, c.j_full]) == listed.size, c
        assert np.array_equal(listed, np.unique(c.values)), c
    finally:
        up.free()


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_distinct_rows(gpu_ctx, oracle, it):
    c = G.Case("distinct_rows", it)
    rng = c.rng
    up = Uploaded(gpu_ctx, c)
    try:
        bS, (bF, rf) = up.of("bsi"), filter_args(up, c)
        listed = gpu_ctx.bsi_distinct(bS, c.base_rows, c.depth, bF, rf)
        for flags in (0, L.SETOP_OPTIMIZE):
            base = int(rng.integers(-(1 << 40) + 1, 1 << 40)) if rng.random() < 0.8 else 0
            what = (c, "flags", flags, "base", base)
            exp = c.distinct_rows_expected(base)
            batch, pos_sh, neg_sh, counts = gpu_ctx.bsi_distinct_rows(bS, c.base_rows, c.depth, base, bF, rf, flags, cap=int(rng.choice([0, 4, 1024])))
            try:
                rows = batch.download()
                assert pos_sh.tolist() == sorted(exp["pos"]) and neg_sh.tolist() == sorted(exp["neg"]), what
                want = [exp["pos"][s] for s in sorted(exp["pos"])] + [exp["neg"][s] for s in sorted(exp["neg"])]
                assert len(rows) == len(want) + 1 and rows[-1] == {}, what
                for r, e in enumerate(want):
                    assert np.array_equal(DR.row_positions(rows[r]), e), (what, "row", r)
                    assert int(counts[r]) == e.size == sum(k.n for k in rows[r].values()), (what, "row", r)
                if flags:
                    check_optimized(oracle, rows)
                pos = np.concatenate([DR.row_positions(r) for r in rows[:pos_sh.size]] + [np.zeros(0, dtype=np.uint64)]).astype(np.int64)
                neg = -(np.concatenate([DR.row_positions(r) for r in rows[pos_sh.size:-1]] + [np.zeros(0, dtype=np.uint64)]).astype(np.int64))
                assert np.array_equal(np.sort(np.concatenate([neg, pos])), listed + base), what
                # the result is an ordinary batch: join it with rows of the pool
                n = len(want)
                ia, ib = rng.integers(0, n + 1, 40), rng.integers(0, c.W.shape[0], 40)
                got = gpu_ctx.intersection_count(batch, ia, up.of("a"), ib)
                ej = [int(G.bit_at(c.W, np.int64(b), (want[a] & np.uint64(0xFFFFF)).astype(np.int64)).sum()) if a < n else 0 for a, b in zip(ia, ib)]
                assert got.tolist() == ej, what
            finally:
                batch.free()
    finally:
        up.free()


MINMAX_OUT = ("mins", "maxs", "min_counts", "max_counts")
MINMAX_PINS = {"auto": L.MINMAX_AUTO, "descent": L.MINMAX_DESCENT, "scatter": L.MINMAX_SCATTER}


def _minmax_equal(got, exp, counts, what):
    """bit for bit, every output; the message names the first differing group"""
    for k, name in enumerate(MINMAX_OUT):
        if k >= 2 and not counts:
            assert got[k] is None, what
            continue
        bad = np.argwhere(got[k] != exp[k])
        assert got[k].dtype == exp[k].dtype and bad.size == 0, (what, name, "group", bad[0].tolist(), "got", got[k][tuple(bad[0])], "expected", exp[k][tuple(bad[0])])


def _minmax_pins(n_cells, _cap=[]):
    """every path pin the shape admits: the descent up to kMinmaxDescentMaxCells groups"""
    if not _cap:
        _cap.append(MM.plan_constants()[1])
    return [p for p in ("auto", "descent", "scatter") if p != "descent" or n_cells <= _cap[0]]


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_groupby_minmax(gpu_ctx, it):
    """The identity of the all-ones row and column: the group is the filter alone, fbk_bsi_min / fbk_bsi_max per shard folded by
    ValCount.Smaller / Larger.  Those calls order the wrapped int64, so the identity is compared while no selected magnitude reaches
    2^63; and they count a sign bit over magnitude 0 apart from +0 (include/fbk.h, fbk_count_matrix_minmax), which changes the counts
    and never the values: the counts are compared where no selected column has one.  tests/test_fuzz_ops_cpu.py shows that the
    default iterations leave cases of either kind."""
    c = G.Case("groupby_minmax", it)
    up = Uploaded(gpu_ctx, c)
    try:
        args = _groupby_args(up, c)
        exp = c.minmax_expected()
        for pin in _minmax_pins(c.n_a * c.n_b):
            for counts in (True, False):
                got = gpu_ctx.count_matrix_minmax(*args, counts=counts, path=MINMAX_PINS[pin])
                _minmax_equal(got, exp, counts, (c, "path", pin, "counts", counts))
        held = c.group_counts() > 0  # a group holds a value exactly where GroupBy Sum's reference counts a column
        assert np.array_equal(exp[2] > 0, held) and np.array_equal(exp[3] > 0, held), c
        mag, sign = c.selected_magnitudes
        if mag.size == 0 or int(mag.max()) < 1 << 63:
            fa = filter_args(up, c)
            lo, hi = (0, 0), (0, 0)
            for v, n in zip(*gpu_ctx.bsi_min(up.of("bsi"), c.base_rows, c.depth, *fa)):
                lo = MM.smaller(lo, (int(v), int(n)))
            for v, n in zip(*gpu_ctx.bsi_max(up.of("bsi"), c.base_rows, c.depth, *fa)):
                hi = MM.larger(hi, (int(v), int(n)))
            mn, mx, n0, n1 = (int(e[c.i_full, c.j_full]) for e in exp)
            assert (lo[1] > 0, hi[1] > 0) == (n0 > 0, n1 > 0) and (n0 == 0 or (lo[0], hi[0]) == (mn, mx)), (c, lo, hi, mn, mx, n0, n1)
            if not (sign & (mag == 0)).any():
                assert (lo[1], hi[1]) == (n0, n1), (c, lo, hi, n0, n1)
    finally:
        up.free()


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_moments(gpu_ctx, it):
    c = G.Case("moments", it)
    up = Uploaded(gpu_ctx, c)
    try:
        y = (up.of("y"), c.base_rows_y, c.depth_y) if c.base_rows_y is not None else (None, None, 0)
        got = gpu_ctx.bsi_moments(up.of("bsi"), c.base_rows, c.depth, *y, *filter_args(up, c))
        exp = c.moments_expected()
        assert exp.n == c.total, c
        for name, g, e in zip(exp._fields, got, exp):
            assert int(g) == e, (c, name, int(g), e)
    finally:
        up.free()


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_groupby_cube(gpu_ctx, it):
    c = G.Case("groupby_cube", it)
    up = Uploaded(gpu_ctx, c)
    try:
        fa = filter_args(up, c)
        got = gpu_ctx.count_cube(up.of("p"), c.rows_p, up.of("a"), c.rows_a, up.of("b"), c.rows_b, *fa)
        exp = c.cube_expected()
        bad = np.argwhere(got != exp)
        assert got.shape == exp.shape and bad.size == 0, (c, "cell", bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
        # the all-ones row of P: the count matrix of A x B under the same filter; with the all-ones rows of A and B: the filter's count
        assert np.array_equal(got[c.p_full], gpu_ctx.count_matrix(up.of("a"), c.rows_a, up.of("b"), c.rows_b, *fa)), c
        assert int(got[c.p_full, c.i_full, c.j_full]) == c.total, c
    finally:
        up.free()


# ---- a shorter last chunk, one call per walk ------------------------------------------------------------------------------------
class ShortUploaded:
    def __init__(self, ctx, sc, names):
        self.b = {}
        for k, (w, rows) in sc.uploads().items():
            if k in names:
                self.b[k] = ctx.upload(rows) if rows is not None else ctx.upload_dense(w)

    def free(self):
        for b in self.b.values():
            b.free()


@pytest.mark.parametrize("name", ["sort", "sort_all_encoded", "sort_dense_field"])
def test_short_last_chunk_sort(gpu_ctx, name):
    sc = G.ShortCase(name)
    up = ShortUploaded(gpu_ctx, sc, ("bsi", "filter"))
    try:
        for desc, keep_zero, offset, limit in ((False, False, 0, None), (True, True, 3, 200), (False, True, 0, 40)):
            cols, vals, tot = gpu_ctx.bsi_sort(up.b["bsi"], sc.base_rows, sc.depth, sc.shard_ids, up.b["filter"], sc.rows_f, desc, keep_zero, offset, limit)
            ec, ev, et = SR.order(*sc.records, desc, keep_zero, offset, limit)
            assert tot == et and et > 100, (name, sc.chunks)
            assert np.array_equal(cols, ec) and np.array_equal(vals, ev), (name, sc.chunks, desc, keep_zero, offset, limit)
    finally:
        up.free()


def test_short_last_chunk_quantiles(gpu_ctx):
    sc = G.ShortCase("quantiles")
    up = ShortUploaded(gpu_ctx, sc, ("bsi", "filter"))
    try:
        vals = sc.records[1]
        n = vals.size
        ranks = [0, n // 3, n // 2, n - 1, n, G.TOP | 0, G.TOP | (n // 5)]
        gv, gc, gn = gpu_ctx.bsi_quantiles(up.b["bsi"], sc.base_rows, sc.depth, ranks, up.b["filter"], sc.rows_f)
        ev, ec, en = P.quantiles(vals, ranks)
        assert gn == en and en > 100 and np.array_equal(gv, ev) and np.array_equal(gc, ec), sc.chunks
        nth = [0.0, 25.0, 50.0, 99.5, 100.0]
        gv, gc, gn = gpu_ctx.bsi_percentile(up.b["bsi"], sc.base_rows, sc.depth, nth, 0, up.b["filter"], sc.rows_f)
        assert [(int(a), int(b)) for a, b in zip(gv, gc)] == [P.replay_on(vals, p, 0)[:2] for p in nth], sc.chunks
    finally:
        up.free()


def test_short_last_chunk_distinct_rows(gpu_ctx):
    sc = G.ShortCase("distinct_rows")
    up = ShortUploaded(gpu_ctx, sc, ("bsi", "filter"))
    try:
        base = -(1 << 22)
        exp = DR.from_values(sc.records[1], base)
        batch, pos_sh, neg_sh, counts = gpu_ctx.bsi_distinct_rows(up.b["bsi"], sc.base_rows, sc.depth, base, up.b["filter"], sc.rows_f)
        try:
            rows = batch.download()
            assert pos_sh.tolist() == sorted(exp["pos"]) and neg_sh.tolist() == sorted(exp["neg"]) and pos_sh.size and neg_sh.size, sc.chunks
            want = [exp["pos"][s] for s in sorted(exp["pos"])] + [exp["neg"][s] for s in sorted(exp["neg"])]
            for r, e in enumerate(want):
                assert np.array_equal(DR.row_positions(rows[r]), e) and int(counts[r]) == e.size, (sc.chunks, r)
        finally:
            batch.free()
    finally:
        up.free()


def test_short_last_chunk_extract_open(gpu_ctx):
    sc = G.ShortCase("extract_open")
    up = ShortUploaded(gpu_ctx, sc, ("filter",))
    try:
        sh, pos = sc.filter_columns
        cols = sc.shard_ids[sh] * np.uint64(1 << 20) + pos.astype(np.uint64)
        c0 = sc.chunks[0]
        first_of_second = int(np.searchsorted(sh, c0))  # the rank of the second chunk's first column
        for offset, limit in ((0, None), (first_of_second - 3, 500), (first_of_second + 1, 7)):
            with gpu_ctx.extract(up.b["filter"], sc.rows_f, sc.shard_ids, offset, limit) as h:
                e = cols[offset:] if limit is None else cols[offset:offset + limit]
                s = sh[offset:] if limit is None else sh[offset:offset + limit]
                assert h.n == e.size and np.array_equal(h.columns(), e), (sc.chunks, offset, limit)
                assert h.span() == (int(s.min()), int(s.max() - s.min() + 1)), (sc.chunks, offset, limit)
    finally:
        up.free()


def test_short_last_chunk_extract_bsi(gpu_ctx):
    sc = G.ShortCase("extract_bsi")
    up = ShortUploaded(gpu_ctx, sc, ("bsi", "filter"))
    try:
        sh, pos = sc.filter_columns
        with gpu_ctx.extract(up.b["filter"], sc.rows_f, sc.shard_ids) as h:
            assert h.span() == (0, sc.n_sh) and G.split(sc.n_sh, G.chunk_extract(sc.n_sh, 66)) == sc.chunks
            gv, gp = h.bsi(up.b["bsi"], sc.base_rows, sc.depth)
            ev, ep = G.sparse_values(sc.Wfrag, sc.base_rows, sc.depth, sh, pos)
            assert ep.any() and not ep.all()
            assert np.array_equal(gp, ep) and np.array_equal(gv, ev), sc.chunks
    finally:
        up.free()


def test_short_last_chunk_extract_rows(gpu_ctx):
    sc = G.ShortCase("extract_rows")
    up = ShortUploaded(gpu_ctx, sc, ("a", "filter"))
    try:
        sh, pos = sc.filter_columns
        with gpu_ctx.extract(up.b["filter"], sc.rows_f, sc.shard_ids) as h:
            assert h.span() == (0, sc.n_sh)
            offs, items = h.rows(up.b["a"], sc.rows_a)
            eo, ei = G.csr_of(G.sparse_rows(sc.Warow, sc.rows_a, sh, pos))
            assert ei.size > 1000 and np.array_equal(offs, eo) and np.array_equal(items, ei), sc.chunks
    finally:
        up.free()


def test_short_last_chunk_groupby_sum(gpu_ctx):
    sc = G.ShortCase("groupby_sum")
    up = ShortUploaded(gpu_ctx, sc, ("a", "b", "bsi", "filter"))
    try:
        es, ec, _ = sc.groupby()
        sums, counts = gpu_ctx.count_matrix_sum(up.b["a"], sc.rows_a, up.b["b"], sc.rows_b, up.b["bsi"], sc.base_rows, sc.depth, up.b["filter"], sc.rows_f)
        assert int(ec.sum()) > 20 and np.array_equal(counts, ec) and np.array_equal(sums, es), sc.chunks
    finally:
        up.free()


def test_short_last_chunk_groupby_distinct(gpu_ctx):
    sc = G.ShortCase("groupby_distinct")
    up = ShortUploaded(gpu_ctx, sc, ("a", "b", "bsi", "filter"))
    try:
        _, ec, ed = sc.groupby()
        dist, counts = gpu_ctx.count_matrix_distinct(up.b["a"], sc.rows_a, up.b["b"], sc.rows_b, up.b["bsi"], sc.base_rows, sc.depth, up.b["filter"], sc.rows_f)
        assert int(ed.sum()) > 100 and np.array_equal(counts, ec) and np.array_equal(dist, ed), sc.chunks
    finally:
        up.free()


def test_short_last_chunk_groupby_minmax(gpu_ctx):
    """65 shards as 33 + 32 and 61 groups: AUTO (the descent), the descent and the scatter pinned, with counts; a chunk of 33 shards
    is also more than a round of either kernel's grid, and the scatter's counting walk densifies the uneven chunks once more"""
    sc = G.ShortCase("groupby_minmax")
    up = ShortUploaded(gpu_ctx, sc, ("a", "b", "bsi", "filter"))
    try:
        exp = sc.groupby(minmax=True)
        assert int((exp[2] > 0).sum()) > 20 and ((exp[0] < exp[1]) & (exp[2] > 0)).any(), sc.chunks
        for pin in _minmax_pins(sc.n_a * sc.n_b):
            got = gpu_ctx.count_matrix_minmax(up.b["a"], sc.rows_a, up.b["b"], sc.rows_b, up.b["bsi"], sc.base_rows, sc.depth, up.b["filter"], sc.rows_f,
                                              path=MINMAX_PINS[pin])
            _minmax_equal(got, exp, True, (sc.chunks, "path", pin))
    finally:
        up.free()


@pytest.mark.parametrize("name", ["moments", "moments_dense_y"])
def test_short_last_chunk_moments(gpu_ctx, name):
    sc = G.ShortCase(name)
    up = ShortUploaded(gpu_ctx, sc, ("bsi", "y", "filter"))
    try:
        got = gpu_ctx.bsi_moments(up.b["bsi"], sc.base_rows, sc.depth, up.b["y"], sc.base_rows_y, sc.depth, up.b["filter"], sc.rows_f)
        exp = sc.moments()
        assert exp.n > 100 and tuple(int(g) for g in got) == tuple(exp), (name, sc.chunks, tuple(got), exp)
        if name == "moments":  # the one-field form over the same row lists (R = 67: one chunk)
            got = gpu_ctx.bsi_moments(up.b["bsi"], sc.base_rows, sc.depth, filt=up.b["filter"], rows_f=sc.rows_f)
            assert tuple(int(g) for g in got) == tuple(sc.moments(one_field=True)), (name, "one field")
    finally:
        up.free()


def test_short_last_chunk_groupby_cube(gpu_ctx):
    sc = G.ShortCase("groupby_cube")
    up = ShortUploaded(gpu_ctx, sc, ("p", "a", "b", "filter"))
    try:
        got = gpu_ctx.count_cube(up.b["p"], sc.rows_p, up.b["a"], sc.rows_a, up.b["b"], sc.rows_b, up.b["filter"], sc.rows_f)
        exp = sc.cube()
        bad = np.argwhere(got != exp)
        assert int((exp > 0).sum()) > 1000 and bad.size == 0, (sc.chunks, "cell", bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
    finally:
        up.free()
