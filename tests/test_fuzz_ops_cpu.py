"""The generator of the structural fuzz (tests/fuzz_ops_gen.py) checked without a GPU: iterations 0 .. 5 of every operator at the
default seed cover every structure choice and every container archetype, most cases have a participating set and one has none, the
expectations of the references agree with each other (and with the generator's second implementation on the filter's columns), and
every short-chunk case really deals its shards into chunks with a shorter last one by include/fbk.h's arithmetic.  For the three
operators added later (groupby_minmax, moments, groupby_cube): their expectations (minmax_ref, moments_ref, cube_ref) against a
second implementation on the selected columns (extremes compared as Python ints, moments_ref.brute, Python popcounts); the default
iterations hold groups with several columns at the minimum, negative minima, the one-field form of the moments, a y that shares
rows with x, and both forms of the cube's kernel; and the cases of the first six operators do not depend on the later ones."""
import numpy as np
import pytest

import cube_ref as CU
import datagen as D
import extract_ref as X
import fuzz_ops_gen as G
import moments_ref as M
import msum_ref as MS
import pct_ref as P

FEATURES = {
    "sort": ("filter", "no_filter", "empty", "alias_filter", "one_batch", "value_fragments"),
    "extract": ("filter", "empty", "alias_filter", "one_batch", "value_fragments", "big_tile"),
    "quantiles": ("filter", "no_filter", "empty", "alias_filter", "one_batch", "value_fragments"),
    "groupby_sum": ("filter", "no_filter", "two_field", "one_field", "empty", "alias_filter", "one_batch", "value_fragments", "big_tile"),
    "groupby_distinct": ("filter", "no_filter", "two_field", "one_field", "empty", "alias_filter", "one_batch", "value_fragments", "big_tile"),
    "distinct_rows": ("filter", "no_filter", "empty", "alias_filter", "one_batch", "value_fragments"),
    "groupby_minmax": ("filter", "no_filter", "two_field", "one_field", "empty", "alias_filter", "one_batch", "value_fragments", "big_tile"),
    "moments": ("filter", "no_filter", "empty", "alias_filter", "one_batch", "value_fragments", "one_field_y", "y_overlaps_x"),
    "groupby_cube": ("filter", "no_filter", "two_field", "one_field", "empty", "alias_filter", "one_batch", "value_fragments", "big_tile"),
}


@pytest.fixture(scope="module")
def all_cases(oracle):
    return {op: [G.Case(op, it) for it in range(6)] for op in G.OPS}


@pytest.mark.parametrize("op", G.OPS)
def test_structure_is_covered(all_cases, op):
    cs = all_cases[op]
    for f in FEATURES[op]:
        assert any(c.features[f] for c in cs), (op, f)
    assert any(all(c.enc.values()) for c in cs) and any(not any(c.enc.values()) for c in cs)  # one batch: the encoded, the dense
    assert any(len(set(c.enc.values())) == 2 for c in cs), "no case mixes dense and encoded operands"
    totals = [c.total for c in cs]
    assert sum(t > 0 for t in totals) >= 4 and any(t == 0 for t in totals), totals
    for c in cs:
        assert c.features["empty"] == (c.total == 0), c
        assert (np.diff(c.shard_ids.astype(object)) > 0).all() and int(c.shard_ids[-1]) < 1 << 44
        assert int(c.base_rows.max()) + c.depth + 2 <= c.W.shape[0]
    assert any(int(c.shard_ids[-1]) >= 1 << 12 for c in cs), "no column id beyond 2^32"
    if op == "distinct_rows":
        assert all(c.depth <= 40 for c in cs)


def test_every_archetype_is_read_through_the_encoded_batch(all_cases):
    seen = set()
    for cs in all_cases.values():
        for c in cs:
            for r in c.rows_read_encoded():
                seen |= c.pool.kinds[r]
    assert seen >= set(D.KINDS), set(D.KINDS) - seen


def test_row_lists_are_irregular(all_cases):
    cs = [c for v in all_cases.values() for c in v]
    assert any(np.unique(c.base_rows).size < c.n_sh for c in cs), "no fragment repeats across shards"
    assert any(c.n_sh > 1 and 0 < np.abs(np.diff(np.sort(c.base_rows.astype(np.int64)))).min() < c.depth + 2 for c in cs), "no fragments overlap"
    assert any(c.rows_f is not None and ((c.rows_f >= c.base_rows) & (c.rows_f < c.base_rows + c.depth + 2)).any() for c in cs)
    assert any(any(np.unique(r).size < r.size for r in c.rows_a) for c in cs), "no row repeats inside rows_a"
    assert any(c.rows_f is not None and c.n_sh > 1 and np.unique(c.rows_f).size == 1 for c in cs), "no filter row shared by every shard"
    assert any(c.n_a > 64 for c in cs)


@pytest.mark.parametrize("it", range(6))
def test_sort_percentile_and_distinct_rows_agree(all_cases, it):
    c = all_cases["sort"][it]
    vals = P.values(c.S, c.F, c.depth)
    cols, v, total = c.sort_expected(False, True, 0, None)
    assert total == vals.size == c.total and np.array_equal(np.sort(vals), v)
    n = vals.size
    ranks = [0, n // 2, max(n - 1, 0), n, G.TOP | 0, G.TOP | (n // 3)]
    qv, qc, qn = P.quantiles(vals, ranks)
    assert qn == n
    for r, a, b in zip(ranks, qv, qc):
        k = r & ~G.TOP
        at = n - 1 - k if r & G.TOP else k
        assert (int(a), int(b)) == ((int(v[at]), int((v == v[at]).sum())) if k < n else (0, 0)), (it, r)
    # the generator's evaluation on the filter's columns gives the same records
    sets = [c.base_rows] + ([c.rows_f] if c.rows_f is not None else [])
    sh, pos = G.sparse_columns(c.W, sets)
    sv, pres = G.sparse_values(c.W, c.base_rows, c.depth, sh, pos)
    assert pres.all() and np.array_equal(sv, vals)
    assert np.array_equal(c.shard_ids[sh] * np.uint64(1 << 20) + pos.astype(np.uint64), c.records[0])


@pytest.mark.parametrize("it", range(6))
def test_distinct_rows_positions(all_cases, it):
    c = all_cases["distinct_rows"][it]
    base = int(c.rng.integers(-(1 << 40) + 1, 1 << 40))
    exp = c.distinct_rows_expected(base)
    u = np.unique(c.values).astype(object) + base
    for sign, want in (("pos", [int(x) for x in u if x >= 0]), ("neg", sorted(int(-x) for x in u if x < 0))):
        got = [int(p) for sh in sorted(exp[sign]) for p in exp[sign][sh]]
        assert got == want, (it, sign)
        assert all(int(p) >> 20 == sh for sh, ps in exp[sign].items() for p in ps)
    assert sum(len(exp[s]) for s in exp) <= 700, "too many output rows for a quick test"


@pytest.mark.parametrize("it", range(6))
def test_groupby_sum_partition_and_columns_only_evaluation(all_cases, it):
    c = all_cases["groupby_sum"][it]
    part = np.zeros((c.n_sh, 2, 16, 1024), dtype=np.uint64)
    part[:, 0, :8], part[:, 1, 8:] = ~np.uint64(0), ~np.uint64(0)
    sums, counts = MS.numpy_expected(part, None, c.F, c.S, c.depth)
    vals = P.values(c.S, c.F, c.depth)
    assert int(counts.sum()) == vals.size == c.total
    assert int(sums.view(np.uint64).sum(dtype=np.uint64)) == int(vals.view(np.uint64).sum(dtype=np.uint64))
    # the case's own expectation, both ways; the all-ones row (and column) is the whole filtered field
    es, ec = c.msum_expected()
    ss, sc, _ = G.sparse_groupby(c.W, c.rows_a, c.rows_b, c.base_rows, c.rows_f, c.depth)
    assert np.array_equal(es, ss) and np.array_equal(ec, sc)
    assert int(ec[c.i_full, c.j_full]) == c.total


@pytest.mark.parametrize("it", [0, 1, 2, 3])
def test_groupby_distinct_both_ways(all_cases, it):
    c = all_cases["groupby_distinct"][it]
    ed, ec = c.mdist_expected()
    _, sc, sd = G.sparse_groupby(c.W, c.rows_a, c.rows_b, c.base_rows, c.rows_f, c.depth)
    assert np.array_equal(ed, sd) and np.array_equal(ec, sc)
    assert int(ed[c.i_full, c.j_full]) == np.unique(c.values).size


@pytest.mark.parametrize("it", range(6))
def test_extract_both_ways(all_cases, it):
    c = all_cases["extract"][it]
    off, lim = int(c.rng.integers(0, c.total + 1)), int(c.rng.integers(1, 5000))
    sh, pos, cols = X.select(c.F, c.shard_ids, off, lim)
    ssh, spos = G.sparse_columns(c.W, [c.rows_f])
    assert np.array_equal(ssh[off:off + lim], sh) and np.array_equal(spos[off:off + lim], pos)
    ev, ep = X.bsi_expected(c.S, c.depth, sh, pos)
    sv, sp = G.sparse_values(c.W, c.base_rows, c.depth, sh, pos)
    assert np.array_equal(ev, sv) and np.array_equal(ep, sp)
    eo, ei = X.rows_expected(c.A, sh, pos)
    so, si = G.csr_of(G.sparse_rows(c.W, c.rows_a, sh, pos))
    assert np.array_equal(eo, so) and np.array_equal(ei, si)
    assert np.array_equal(c.locate(cols)[0], sh) and np.array_equal(c.locate(cols)[1], pos)


def test_the_cases_of_the_first_six_operators_do_not_depend_on_the_later_ones():
    """a later operator draws from a stream of its own, and what only it needs after the draws every operator makes"""
    assert G.OPS[:6] == ("sort", "extract", "quantiles", "groupby_sum", "groupby_distinct", "distinct_rows") and G.NEW_OPS == G.OPS[6:]
    assert [G.STREAM[op] for op in G.OPS] == list(range(7400, 7400 + len(G.OPS)))
    assert G.SHORT_STREAM[:10] == sorted(G.SHORT_STREAM[:10]) and sorted(G.SHORT_STREAM) == sorted(G.SHORT)


@pytest.mark.parametrize("it", range(6))
def test_groupby_minmax_both_ways(all_cases, it):
    c = all_cases["groupby_minmax"][it]
    exp = c.minmax_expected()
    other = G.sparse_minmax(c.W, c.rows_a, c.rows_b, c.base_rows, c.rows_f, c.depth)
    for e, o, name in zip(exp, other, ("mins", "maxs", "min_counts", "max_counts")):
        assert e.dtype == o.dtype and np.array_equal(e, o), (it, name)
    # a group holds a value exactly where GroupBy Sum's reference counts a column; the all-ones row (and column) is the whole selection
    counts = MS.numpy_expected(c.A, c.Bw, c.F, c.S[:, :2], 0)[1]  # (the counts do not depend on the planes)
    assert counts.dtype == np.uint64 and np.array_equal(c.group_counts(), counts)
    assert np.array_equal(exp[2] > 0, counts > 0) and np.array_equal(exp[3] > 0, counts > 0)
    assert (exp[2] <= counts).all() and (exp[3] <= counts).all() and int(counts[c.i_full, c.j_full]) == c.total
    mag, sign = c.selected_magnitudes
    assert G.minmax_of(mag, sign) == tuple(int(e[c.i_full, c.j_full]) for e in exp)


def test_groupby_minmax_cases_hold_ties_and_negative_minima(all_cases):
    exps = [c.minmax_expected() for c in all_cases["groupby_minmax"]]
    assert sum(bool((e[2] > 1).any()) for e in exps) >= 2 and any((e[3] > 1).any() for e in exps), "no group with several columns at its minimum"
    assert any(((e[0] < 0) & (e[2] > 0)).any() for e in exps) and any(((e[0] >= 0) & (e[2] > 0)).any() for e in exps)
    # the identity with fbk_bsi_min / fbk_bsi_max is compared where no selected magnitude reaches 2^63 (the counts: where no selected
    # column has the sign bit over magnitude 0): the default cases must leave some of either
    small = [bool((c.selected_magnitudes[0] < np.uint64(1 << 63)).all()) for c in all_cases["groupby_minmax"]]
    plain = [not bool((c.selected_magnitudes[1] & (c.selected_magnitudes[0] == 0)).any()) for c in all_cases["groupby_minmax"]]
    nonempty = [c.total > 0 for c in all_cases["groupby_minmax"]]
    assert sum(s and n for s, n in zip(small, nonempty)) >= 3 and sum(s and p and n for s, p, n in zip(small, plain, nonempty)) >= 1, (small, plain)


@pytest.mark.parametrize("it", range(6))
def test_moments_both_ways(all_cases, it):
    c = all_cases["moments"][it]
    exp = c.moments_expected()
    sets = [c.base_rows] + ([c.base_rows_y] if c.base_rows_y is not None else []) + ([c.rows_f] if c.rows_f is not None else [])
    sh, pos = G.sparse_columns(c.W, sets)
    xs, px = G.sparse_ints(c.W, c.base_rows, c.depth, sh, pos)
    ys, py = G.sparse_ints(c.W, c.base_rows_y, c.depth_y, sh, pos) if c.base_rows_y is not None else (None, px)
    assert px.all() and py.all() and exp.n == len(xs) == c.total
    assert exp == M.brute(xs, ys), it
    if c.features["one_field_y"]:
        assert c.Sy is None and exp.sum_y == exp.sum_yy == exp.sum_xy == 0
    if c.features["y_overlaps_x"]:
        off = c.base_rows_y.astype(np.int64) - c.base_rows
        assert ((off >= 1) & (off <= c.depth + 1)).all() and int(c.base_rows_y.max()) + c.depth_y + 2 <= c.pool.n_plain
    assert c.base_rows_y is None or int(c.base_rows_y.max()) + c.depth_y + 2 <= c.pool.n_plain


@pytest.mark.parametrize("it", range(6))
def test_groupby_cube_both_ways(all_cases, it):
    c = all_cases["groupby_cube"][it]
    exp = c.cube_expected()
    assert exp.shape == (c.n_p, c.n_a, c.n_b) and 1 <= c.n_p <= 9 and exp.size <= G.CUBE_CELLS
    assert c.rows_p.shape == (c.n_sh, c.n_p) and c.rows_a.shape == (c.n_sh, c.n_a) and c.rows_b.shape == (c.n_sh, c.n_b)
    full = c.pool.full
    assert (c.rows_p[:, c.p_full] == full).all() and (c.rows_a[:, c.i_full] == full).all() and (c.rows_b[:, c.j_full] == full).all()
    triples = CU.sample_triples(c.rng, *exp.shape, k=6) + [(c.p_full, c.i_full, c.j_full)]
    assert G.sparse_cube(c.W, c.rows_p, c.rows_a, c.rows_b, c.rows_f, triples) == [int(exp[t]) for t in triples]
    assert int(exp[c.p_full, c.i_full, c.j_full]) == c.total


def test_groupby_cube_cases_take_both_forms_of_the_kernel(all_cases):
    n_p = [c.n_p for c in all_cases["groupby_cube"]]
    assert any(n <= 4 for n in n_p) and any(n > 4 for n in n_p), n_p
    assert any(max(c.n_a, c.n_b) > 64 for c in all_cases["groupby_cube"])


SPLITS = {"sort": [17, 16], "sort_all_encoded": [16, 15], "sort_dense_field": [1025, 1024], "quantiles": [17, 16], "distinct_rows": [17, 16], "extract_open": [1025, 1024],
          "extract_bsi": [17, 16], "extract_rows": [2, 1], "groupby_sum": [29, 28], "groupby_distinct": [33, 32],
          "groupby_minmax": [33, 32], "moments": [32, 31], "moments_dense_y": [62, 61], "groupby_cube": [33, 32]}
ALL_ENCODED = ("sort_all_encoded", "moments")


@pytest.mark.parametrize("name", sorted(G.SHORT))
def test_short_chunk_cases_split_unevenly(name):
    c = G.ShortCase(name)
    assert c.chunks == SPLITS[name] and sum(c.chunks) == c.n_sh
    c0 = c.chunks[0]
    assert len(c.chunks) >= 2 and c.chunks[-1] < c.chunks[0]
    assert all(len(set(G.split(n, c.chunk_of(n)))) == 1 for n in range(1, c.n_sh)), "a smaller count splits unevenly too"
    assert any(c.dense.values()) or name in ALL_ENCODED
    assert 3 not in c.rows_f[:c0] and (3 in c.rows_f[c0:] or c.chunks[-1] <= 2), "the filter row of the last chunk alone"
    # the arithmetic, once more from the numbers in include/fbk.h: the examples of the issue
    assert G.chunk_extract(31, 67) == 16 and (1 << 28) // ((1 << 17) * 67) == 30
    assert G.chunk_extract(3, 1024) == 2
    assert (1 << 30) // (10 * (1 << 20) + 16 + 69 * (1 << 17)) == 54 and G.chunk_msum(55, 1, 1, 64, 69) == 28
    # the walk's later chunks read other rows than its first (else an offset that stays 0 would go unseen), and find columns there
    sh, _ = c.filter_columns
    assert (sh >= c0).any() and (sh < c0).any()
    lists = [c.base_rows, c.rows_f] + ([c.rows_a.reshape(c.n_sh, -1)[:, 0]] if name in ("extract_rows", "groupby_sum", "groupby_distinct") else [])
    for lst in lists:
        if np.unique(lst).size > 1:
            assert not np.array_equal(lst[c0:c0 + c.chunks[-1]], lst[:c.chunks[-1]]), name


@pytest.mark.parametrize("name", ["groupby_minmax", "moments", "moments_dense_y", "groupby_cube"])
def test_short_chunk_cases_of_the_later_calls(name):
    """what test_short_chunk_cases_split_unevenly asks of a row list, for the lists these calls add; the arithmetic of their
    entries in include/fbk.h; and that the expectation has something to tell"""
    c = G.ShortCase(name)
    c0, last = c.chunks[0], c.chunks[-1]
    lists = [c.base_rows_y] if name.startswith("moments") else [c.rows_a[:, 0], c.rows_b[:, 0]] + ([c.rows_p[:, 0]] if c.n_p else [])
    for lst in lists:
        assert lst[c0] != lst[0] and not np.array_equal(lst[c0:c0 + last], lst[:last]), name
    if name == "groupby_minmax":
        assert (1 << 30) // ((1 << 17) * 128) == 64 and (c.n_a, c.n_b, c.depth) == (1, 61, 64) and c.dense["a"] and sum(c.dense.values()) == 1
        assert c.n_sh == 65 and c.chunks[0] > 8, "the first chunk takes both kernels past one round of their grid"
        mn, mx, c0n, c1n = c.groupby(minmax=True)
        assert int((c0n > 0).sum()) > 20 and ((mn < mx) & (c0n > 0)).any() and (mn[c0n > 0] < 0).any()
        assert np.array_equal(c0n > 0, c.groupby()[1] > 0)
    elif name.startswith("moments"):
        r = 66 + 1 + (0 if c.dense["y"] else 66)
        assert (1 << 30) // ((1 << 17) * r) == {133: 61, 67: 122}[r] and c.n_sh == {133: 63, 67: 123}[r]
        assert M.densify_chunk(c.n_sh, False, 64, c.dense["y"], 64, False) == c.chunks[0]
        same = c.base_rows_y == c.base_rows
        assert same[:c0].any() and (~same[:c0]).any() and same[c0:].any() and (~same[c0:]).any()
        m, m1 = c.moments(), c.moments(one_field=True)
        assert 100 < m.n < m1.n and m.sum_xy != m.sum_xx and m1.sum_xx != m.sum_xx and m.sum_y != m.sum_x
    else:
        per = 8 * c.n_p * c.n_a * c.n_b + (1 << 17) * (c.n_a + c.n_b + 1)
        assert c.dense == {"bsi": False, "filter": False, "a": False, "b": False, "p": True} and c.n_p <= 4
        assert (1 << 17) * (c.n_a + c.n_b + 1) > 100 * 8 * c.n_p * c.n_a * c.n_b, "the densified rows dominate the chunk"
        assert (1 << 30) // per == 63 and CU.chunk(c.n_sh, c.n_p, c.n_a, c.n_b, True, False, False, False) == c.chunks[0]
        assert c.chunks[0] * per <= 1 << 30
        cube = c.cube()
        assert cube.shape == (c.n_p, c.n_a, c.n_b) and int((cube > 0).sum()) > 1000
