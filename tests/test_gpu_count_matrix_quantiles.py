"""GPU parity of fbk_count_matrix_quantiles (GroupBy with a percentile of an int field per group).  Every case runs AUTO and each path
pin that takes the shape — GLOBAL always, LDS where the (group, request) pairs are within its cap, and where only the groups are,
with as many of the requests as fit —, and every result is compared bit for bit with the numpy model (tests/gquant_ref.py; the
CPU test checks the model).  Dense batches over shard counts, shapes and depths (0, 1, 63, 64 and around the digit of each path);
value sets a wrong pass gives away; cross-checks against fbk_count_matrix_minmax, fbk_bsi_quantiles and fbk_count_matrix on the
same operands; encoded batches (the densify path) and calls that densify in more than one chunk; 19 shards, at which the kernels
go round their grid-stride loops; n_q = 0, 16 and repeated requests; every error, each followed by a good call."""
import numpy as np
import pytest

import datagen as D
import gquant_ref as G
import minmax_ref as M
import test_gpu_count_matrix_minmax as TM  # its mutex-like rows
import test_gpu_count_matrix_sum as T  # its builders of dense and encoded cases
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu

AUTO, LDS, GLOBAL = L.GQUANT_AUTO, L.GQUANT_LDS, L.GQUANT_GLOBAL
FR3 = [(0, 1), (1, 2), (1, 1)]
FR5 = [(1, 2), (0, 1), (99, 100), (1, 4), (1, 1)]


@pytest.fixture(scope="module")
def plan():
    return G.plan_constants()


def _equal(got, exp, what=()):
    for k, name in enumerate(("values", "counts", "totals")):
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, what + (name, got[k].shape, exp[k].shape)
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, what + (name, bad[:4].tolist(), got[k][tuple(bad[0])], exp[k][tuple(bad[0])])


def _all_paths(ctx, plan, exp, bA, ra, bB, rb, bS, base, depth, fr, bF=None, rf=None):
    """the call under AUTO and every pin that takes the shape, each against the model `exp` of the fractions `fr`.  Returns AUTO's."""
    n_a = np.asarray(ra).shape[1]
    cells = n_a * (np.asarray(rb).shape[1] if bB is not None else 1)
    got = None
    for p in (AUTO, GLOBAL, LDS):
        n_fit = len(fr)
        if p == LDS:
            if cells > plan["lds_cap"]:
                continue
            n_fit = min(len(fr), plan["lds_cap"] // cells)  # the requests that fit the LDS beside each other (0: the totals alone)
        g = ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, fr[:n_fit], bF, rf, path=p)
        _equal(g, (exp[0][..., :n_fit], exp[1][..., :n_fit], exp[2]), ("path", p))
        got = got or g
    return got


def _depths(plan):
    """0, 1, 63, 64 and, for the digit d of each path, d - 1, d, d + 1 and 2 d"""
    ds = {0, 1, 63, 64}
    for d in (plan["lds_digit"], plan["global_digit"]):
        ds |= {d - 1, d, d + 1, 2 * d}
    return sorted(ds)


# shapes (None: the one-field form): one group; a few (LDS with several requests); 35 groups (LDS with one request); a full transpose
# of both sides; more B rows than a transpose holds; more A rows than one
SHAPES = [(1, None), (3, 2), (5, 7), (64, 64), (33, 65), (70, None)]
# every shape at 1, 2 and 3 shards, the depths and the filter going round (the case index picks them)
SHAPE_CASES = [(sh, n_sh, k) for k, (sh, n_sh) in enumerate((sh, s) for sh in SHAPES for s in (1, 2, 3))]


@pytest.mark.parametrize("shape,n_sh,k", SHAPE_CASES)
def test_dense_shapes(gpu_ctx, plan, shape, n_sh, k):
    n_a, n_b = shape
    ds = _depths(plan)
    depth, with_filter = ds[(5 * k + 3) % len(ds)], k % 2 == 1
    rng = D.rng_for(9200, n_sh, n_a, n_b or 0, depth)
    A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b or 1, depth, exists_ands=2 if n_a * (n_b or 1) <= 64 else 6)
    if n_b is None:
        Bw = None
    if depth > 3:
        S[:, 5:] &= T._rnd(rng, (n_sh, depth - 3, 16, 1024), 3)  # the higher planes sparse: columns share values
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        Fx = F if with_filter else None
        exp = G.numpy_expected(A, Bw, Fx, S, depth, FR3)
        got = _all_paths(gpu_ctx, plan, exp, bA, ra, bB, rb, bS, base, depth, FR3, bF if with_filter else None, rf if with_filter else None)
        assert (got[2] > 0).any() and (depth > 9 or (got[1] > 1).any())
    finally:
        for b in (bA, bB, bF, bS):
            if b is not None:
                b.free()


@pytest.mark.parametrize("with_filter", [False, True])
def test_every_depth(gpu_ctx, plan, with_filter):
    """(3, 2) — within the LDS cap with three requests — at every depth of the list, two shards"""
    n_sh, n_a, n_b = 2, 3, 2
    for depth in _depths(plan):
        rng = D.rng_for(9300, depth, int(with_filter))
        A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=4)
        if depth > 3:
            S[:, 5:] &= T._rnd(rng, (n_sh, depth - 3, 16, 1024), 2)
        bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
        try:
            exp = G.numpy_expected(A, Bw, F if with_filter else None, S, depth, FR5)
            _all_paths(gpu_ctx, plan, exp, bA, ra, bB, rb, bS, base, depth, FR5, bF if with_filter else None, rf if with_filter else None)
            assert depth < 7 or ((exp[0][..., 1] < 0).all() and (exp[0][..., 4] > 0).all())
        finally:
            for b in (bA, bB, bF, bS):
                b.free()


def _hi(depth):
    return 1 << (depth - 1)


# (depth, values (sign, magnitude), name)
VALUE_SETS = [
    (7, [(False, 77)], "all equal"),
    (20, [(False, 1000), (False, 1001)], "lowest bit"),
    (20, [(True, 1000), (True, 1001)], "lowest bit, negative"),
    (20, [(False, 5), (False, 5 | _hi(20))], "highest plane"),
    (64, [(False, 5), (False, 5 | _hi(64))], "highest plane of 64"),
    (63, [(False, 5), (False, 5 | _hi(63)), (True, 5 | _hi(63))], "highest plane of 63"),
    (16, [(False, 300), (True, 300)], "+m and -m"),
    (20, [(True, 0)], "sign over zero"),
    (9, [(True, 0), (False, 0), (True, 1), (False, 1)], "zeros of both signs"),
]


@pytest.mark.parametrize("depth,values,what", VALUE_SETS)
def test_value_sets(gpu_ctx, plan, depth, values, what):
    """mutex-like rows (6 x 4 groups, two shards).  A row 0 is empty; A row 1 is cut down to ONE column; A row 2 keeps only its
    columns of the last shard"""
    rng = D.rng_for(9400, depth, len(values))
    n_sh, n_a, n_b = 2, 6, 4
    A, Bw, F, S = TM._mutex_case(rng, n_sh, n_a, n_b, depth, values)
    A[0, 2] = 0
    ex = np.nonzero(M.bits(S[1, 0] & A[1, 1]))[0]
    A[:, 1] = 0
    A[1, 1].reshape(-1)[ex[0] // 64] = np.uint64(1) << np.uint64(ex[0] % 64)
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        for with_filter in (False, True):
            exp = G.numpy_expected(A, Bw, F if with_filter else None, S, depth, FR5)
            got = _all_paths(gpu_ctx, plan, exp, bA, ra, bB, rb, bS, base, depth, FR5, bF if with_filter else None, rf if with_filter else None)
            v, c, t = got
            assert not t[0].any() and not v[0].any() and not c[0].any()  # the empty groups
            assert (t[2:] > 50).all()
            if not with_filter:
                assert t[1].sum() == 1 and (c[1][t[1] == 1] == 1).all()  # the one-column group
            if what == "all equal":
                assert (v[2:] == 77).all() and (c[2:] == t[2:, :, None]).all()
            if what == "sign over zero":
                assert not v.any() and (c[2:] == t[2:, :, None]).all()
            if what == "+m and -m":
                assert (v[2:, :, 1] == -300).all() and (v[2:, :, 4] == 300).all()
            if what == "highest plane of 64":  # the wrapped int64 order: 5 | 2^63 is written INT64_MIN + 5 and is the minimum
                assert (v[2:, :, 1] == M.INT64_MIN + 5).all() and (v[2:, :, 4] == 5).all()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


@pytest.mark.parametrize("depth", [7, 20])
@pytest.mark.parametrize("shape", [(5, 7), (33, 65), (70, None)])
def test_launches_that_go_round_their_loops(gpu_ctx, plan, shape, depth):
    """minmax_ref.many_shard_case: 19 shards over 5 stored ones; the extremes and the ties of a group lie beyond the first round of
    either kernel's grid (2048 blocks x 4 units: 8 shards; the LDS path's 1024 blocks: 4 shards)"""
    n_a, n_b = shape
    A, Bw, F, S = M.many_shard_case(n_a, n_b, depth)
    bA, _, bB, _, bF, _, bS, _ = T._upload_dense(gpu_ctx, A, Bw, F, S)
    ra, rb, rf, base = M.many_shard_lists(n_a, n_b, depth)
    try:
        gA, gB, gF, gS = M.many_shard_words(A, Bw, F, S)
        for with_filter in (False, True):
            exp = G.numpy_expected(gA, gB, gF if with_filter else None, gS, depth, FR3)
            assert (exp[2] > 0).sum() * 2 > exp[2].size
            _all_paths(gpu_ctx, plan, exp, bA, ra, bB, rb, bS, base, depth, FR3, bF if with_filter else None, rf if with_filter else None)
    finally:
        for b in (bA, bB, bF, bS):
            if b is not None:
                b.free()


@pytest.mark.parametrize("depth", [8, 20, 63, 64])
def test_cross_checks_against_the_merged_calls(gpu_ctx, plan, depth):
    rng = D.rng_for(9500, depth)
    n_sh, n_a, n_b = 3, 5, 7
    A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=3)
    S[:, 5:] &= T._rnd(rng, (n_sh, depth - 3, 16, 1024), 2)
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        for p in (AUTO, GLOBAL):
            v, c, t = gpu_ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, [(0, 1), (1, 1)], bF, rf, path=p)
            # the totals: fbk_count_matrix's with the exists row ANDed in (the exists row as its filter; the quantiles call without F)
            _, _, t0 = gpu_ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, [], path=p)
            assert np.array_equal(t0, gpu_ctx.count_matrix(bA, ra, bB, rb, bS, base))
            if depth <= 63:  # (at depth 64 the two calls order differently by contract)
                mn, mx, cmn, cmx = gpu_ctx.count_matrix_minmax(bA, ra, bB, rb, bS, base, depth, bF, rf)
                assert (t > 0).all()
                assert np.array_equal(v[..., 0], mn) and np.array_equal(v[..., 1], mx) and np.array_equal(c[..., 0], cmn) and np.array_equal(c[..., 1], cmx)
        # one group, A = the exists row: fbk_bsi_quantiles with the ranks computed on the host
        fr = FR5 + [(1, 1 << 20), (3, 7)]
        for p in (AUTO, LDS, GLOBAL):
            v, c, t = gpu_ctx.count_matrix_quantiles(bS, base[:, None], None, None, bS, base, depth, fr, bF, rf, path=p)
            n = int(t[0, 0])
            qv, qc, qn = gpu_ctx.bsi_quantiles(bS, base, depth, [G.disc_rank(n, *f) for f in fr], bF, rf)
            assert qn == n > 0 and np.array_equal(v[0, 0], qv) and np.array_equal(c[0, 0], qc)
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


@pytest.mark.parametrize("depth", [0, 7, 20, 63])
def test_encoded_batches(gpu_ctx, oracle, plan, depth):
    """mixed containers, rows missing in some shards, BSI fragments from bsi_fragment_from_values: the densify path"""
    from oracle import pybsi

    pybsi._lib()
    rng = D.rng_for(9600, depth)
    n_sh, n_a, n_b = 5, 6, 9
    a_rows, b_rows, f_rows, frags, A, Bw, F, S, _ = T._encoded_case(oracle, pybsi, rng, n_sh, n_a, n_b, depth)
    flat = lambda rows: [D.to_fbk_row(r) for sh in rows for r in sh]
    bA, bB = gpu_ctx.upload(flat(a_rows)), gpu_ctx.upload(flat(b_rows))
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    bF = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    bS, base = T._upload_bsi(gpu_ctx, frags)
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        for with_filter in (False, True):
            exp = G.numpy_expected(A, Bw, F if with_filter else None, S, depth, FR3)
            _all_paths(gpu_ctx, plan, exp, bA, ra, bB, rb, bS, base, depth, FR3, bF if with_filter else None, rf if with_filter else None)
        exp = G.numpy_expected(A, None, F, S, depth, FR5)  # the one-field form over encoded rows
        got = _all_paths(gpu_ctx, plan, exp, bA, ra, None, None, bS, base, depth, FR5, bF, rf)
        assert (got[2] > 0).any()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


@pytest.mark.parametrize("n_sh,n_a,two_fields,chunk", [(8, 1024, False, 4), (3, 4096, True, 1)])
def test_densify_in_several_chunks(gpu_ctx, oracle, plan, n_sh, n_a, two_fields, chunk):
    """the shapes of the minmax test: encoded batches and a long row list (cycling over 8 stored rows per shard); 1024 rows and the
    BSI rows take two chunks of four shards, 4096 x 2 rows one shard at a time; every pass densifies every chunk again"""
    from oracle import pybsi

    pybsi._lib()
    rng = D.rng_for(9700, n_sh, n_a)
    depth, stored, n_b = 20, 8, 2 if two_fields else 1
    assert TM._chunk(n_sh, n_a + (n_b if two_fields else 0) + 1 + depth + 2) == chunk < n_sh
    assert G.plan_check(["C %d %d" % (n_sh, n_a + (n_b if two_fields else 0) + 1 + depth + 2)])[0][0] == chunk
    a_rows, b_rows, f_rows, frags, A, Bw, F, S, _ = T._encoded_case(oracle, pybsi, rng, n_sh, stored, 2, depth, n_vals=3000)
    bA = gpu_ctx.upload([D.to_fbk_row(r) for sh in a_rows for r in sh])
    bB = gpu_ctx.upload([D.to_fbk_row(r) for sh in b_rows for r in sh])
    bF = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    bS, base = T._upload_bsi(gpu_ctx, frags)
    cyc = np.arange(n_a) % stored
    ra = (np.arange(n_sh)[:, None] * stored + cyc[None, :]).astype(np.uint32)
    rb = np.arange(n_sh * 2, dtype=np.uint32).reshape(n_sh, 2)
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        exp8 = G.numpy_expected(A, Bw if two_fields else None, F, S, depth, FR3)
        exp = tuple(e[cyc] for e in exp8)
        for p in (AUTO, GLOBAL):
            got = gpu_ctx.count_matrix_quantiles(bA, ra, bB if two_fields else None, rb if two_fields else None, bS, base, depth, FR3, bF, rf, path=p)
            _equal(got, exp, ("path", p))
        assert (got[2] > 0).any() and (got[0][..., 0] < got[0][..., 2]).any()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def test_request_lists(gpu_ctx, plan):
    """n_q = 0 (the totals alone, the value outputs NULL), n_q = 16, requests repeated and out of order"""
    rng = D.rng_for(9800)
    n_sh, n_a, n_b, depth = 2, 3, 2, 20
    A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=4)
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        fr16 = [(1, 1), (1, 2), (1, 2), (0, 1), (7, 9), (1, 1 << 20), ((1 << 20) - 1, 1 << 20), (1 << 20, 1 << 20), (1, 3), (2, 3), (1, 2), (0, 5), (5, 5), (1, 100),
                (99, 100), (1, 2)]
        assert len(fr16) == plan["max_requests"] == 16
        exp = G.numpy_expected(A, Bw, F, S, depth, fr16)
        for p in (AUTO, GLOBAL):
            _equal(gpu_ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, fr16, bF, rf, path=p), exp, ("path", p))
            v, c, t = gpu_ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, [], bF, rf, path=p)
            assert v.shape == (n_a, n_b, 0) and c.shape == (n_a, n_b, 0) and np.array_equal(t, exp[2])
        # the LDS pin: one group, sixteen requests; and three groups, sixteen requests where the cap allows
        e1 = G.numpy_expected(A[:, :1], None, F, S, depth, fr16)
        _equal(gpu_ctx.count_matrix_quantiles(bA, ra[:, :1], None, None, bS, base, depth, fr16, bF, rf, path=LDS), e1)
        if 3 * 16 <= plan["lds_cap"]:
            e3 = G.numpy_expected(A, None, F, S, depth, fr16)
            _equal(gpu_ctx.count_matrix_quantiles(bA, ra, None, None, bS, base, depth, fr16, bF, rf, path=LDS), e3)
        _, _, t = gpu_ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, [], bF, rf, path=LDS)
        assert np.array_equal(t, exp[2])
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def test_errors_then_recovery(gpu_ctx, plan):
    rng = D.rng_for(9900)
    n_sh, n_a, n_b, depth = 2, 33, 65, 8
    A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=6)
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    cq = gpu_ctx.count_matrix_quantiles
    try:
        good = G.numpy_expected(A[:, :3], Bw[:, :4], F, S, depth, FR3)
        bad_base = base.copy()
        bad_base[1] = n_sh * (depth + 2) - 1  # the fragment's rows run past the batch
        wide = np.zeros((n_sh, 4097), dtype=np.uint32)
        most = plan["scratch_bound"] // (8 << plan["global_digit"])  # (group, request) pairs of the scratch bound
        side = 1 << ((most.bit_length() + 1) // 2)  # side * side * 2 requests: twice the bound at least
        assert side <= 4096 and side * side * 2 > most
        big = np.zeros((n_sh, side), dtype=np.uint32)

        def raw(**kw):  # the C call itself: NULL pointers and counts the wrapper would not pass
            num, den = np.array([1], np.uint32), np.array([2], np.uint32)
            o = [np.zeros(n_a * n_b, t) for t in (np.int64, np.uint64, np.uint64)]
            a = dict(ctx=gpu_ctx.h, a=bA.h, ra=ra.ctypes.data, n_a=n_a, b=bB.h, rb=rb.ctypes.data, n_b=n_b, f=None, rf=None, s=bS.h, base=base.ctypes.data, depth=depth,
                     n_sh=n_sh, num=num.ctypes.data, den=den.ctypes.data, n_q=1, flags=0, v=o[0].ctypes.data, c=o[1].ctypes.data, t=o[2].ctypes.data)
            a.update(kw)
            L.check(gpu_ctx.lib.fbk_count_matrix_quantiles(*a.values()))

        calls = {
            "NULL a": lambda: raw(a=None),
            "NULL bsi": lambda: raw(s=None),
            "NULL base_rows": lambda: raw(base=None),
            "NULL out_totals": lambda: raw(t=None),
            "NULL q_num": lambda: raw(num=None),
            "NULL q_den": lambda: raw(den=None),
            "NULL out_values": lambda: raw(v=None),
            "NULL out_counts": lambda: raw(c=None),
            "den == 0": lambda: cq(bA, ra, bB, rb, bS, base, depth, [(0, 0)]),
            "den > 2^20": lambda: cq(bA, ra, bB, rb, bS, base, depth, [(1, (1 << 20) + 1)]),
            "num > den": lambda: cq(bA, ra, bB, rb, bS, base, depth, [(1, 2), (3, 2)]),
            "n_q > 16": lambda: cq(bA, ra, bB, rb, bS, base, depth, [(1, 2)] * 17),
            "n_a > 4096": lambda: cq(bA, wide, bB, rb, bS, base, depth, FR3),
            "n_b > 4096": lambda: cq(bA, ra, bB, wide, bS, base, depth, FR3),
            "bit_depth > 64": lambda: cq(bA, ra, bB, rb, bS, base, 65, FR3),
            "b NULL, n_b 2": lambda: raw(b=None, rb=None, n_b=2),
            "A row beyond the batch": lambda: cq(bA, ra + np.uint32(n_sh * n_a), bB, rb, bS, base, depth, FR3),
            "B row beyond the batch": lambda: cq(bA, ra, bB, rb + np.uint32(n_sh * n_b), bS, base, depth, FR3),
            "filter row beyond the batch": lambda: cq(bA, ra, bB, rb, bS, base, depth, FR3, bF, rf + np.uint32(n_sh)),
            "fragment beyond the batch": lambda: cq(bA, ra, bB, rb, bS, bad_base, depth, FR3),
            "unknown flags": lambda: cq(bA, ra, bB, rb, bS, base, depth, FR3, path=3),
            "LDS beyond its cap": lambda: cq(bA, ra, bB, rb, bS, base, depth, FR3, path=LDS),
            "scratch beyond its bound": lambda: cq(bA, big, bB, big, bS, base, depth, [(1, 2), (1, 1)], path=GLOBAL),
        }
        for name, call in calls.items():
            with pytest.raises(L.FbkError) as e:
                call()
            assert e.value.code == L.FBK_E_INVALID, name
            if name == "scratch beyond its bound":
                assert "block the leading field" in str(e.value)
            _equal(cq(bA, ra[:, :3], bB, rb[:, :4], bS, base, depth, FR3, bF, rf), good, (name,))  # the next good call
        # the NULL context: an error, and the good context is untouched
        with pytest.raises(L.FbkError):
            raw(ctx=None)
        _equal(cq(bA, ra[:, :3], bB, rb[:, :4], bS, base, depth, FR3, bF, rf), good)
        # no shards: the empty-group values; no groups: nothing to write
        o = [np.ones(12 * 3, np.int64), np.ones(12 * 3, np.uint64), np.ones(12, np.uint64)]
        num, den = np.array([0, 1, 1], np.uint32), np.array([1, 2, 1], np.uint32)
        L.check(gpu_ctx.lib.fbk_count_matrix_quantiles(gpu_ctx.h, bA.h, ra.ctypes.data, 3, bB.h, rb.ctypes.data, 4, None, None, bS.h, base.ctypes.data, depth, 0,
                                                       num.ctypes.data, den.ctypes.data, 3, 0, *[x.ctypes.data for x in o]))
        assert not o[0].any() and not o[1].any() and not o[2].any()
        L.check(gpu_ctx.lib.fbk_count_matrix_quantiles(gpu_ctx.h, bA.h, ra.ctypes.data, 0, bB.h, rb.ctypes.data, 4, None, None, bS.h, base.ctypes.data, depth, n_sh,
                                                       num.ctypes.data, den.ctypes.data, 3, 0, *[x.ctypes.data for x in o]))
        assert not o[0].any() and not o[1].any() and not o[2].any()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()
