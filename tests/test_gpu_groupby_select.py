"""fbk_count_matrix_select, fbk_count_cube_select and fbk_count_matrix_sum_select: the groups of a GroupBy through having / sort /
offset / limit without the download of all of them.  Expected: the model of the reference (groupby_select_ref.py) applied to the output of
the existing full call on the same operands, and applied to the numpy brute force of cube_ref.py / msum_ref.py.  Both paths of the
stage are pinned (FBK_GROUPSEL_DEVICE / FBK_GROUPSEL_HOST) and must agree bit for bit.  Row lists repeat row indexes, so that equal
counts and equal sums are certain."""
import ctypes as C

import numpy as np
import pytest

import cube_ref
import datagen as D
import groupby_select_ref as R
import msum_ref as M
from featurebase_amd import lib as L
from featurebase_amd.roaring import GroupSelect

pytestmark = pytest.mark.gpu

PT = cube_ref.PT
SLOTS = (0, 9)


def _rnd(rng, shape):
    w = np.zeros(shape + (16, 1024), dtype=np.uint64)
    for sl in SLOTS:
        w[..., sl, :] = rng.integers(0, 1 << 63, shape + (1024,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (1024,), dtype=np.uint64)
    return w


def _field(ctx, rng, n_sh, n, distinct):
    """a dense batch of `distinct` rows per shard and a row list [n_sh, n] that repeats them: (batch, list, the words the list names)"""
    distinct = min(distinct, n)
    W = _rnd(rng, (n_sh, distinct))
    rl = (np.arange(n_sh, dtype=np.uint32)[:, None] * distinct + (np.arange(n, dtype=np.uint32) % distinct)[None, :]).astype(np.uint32)
    return ctx.upload_dense(W.reshape(-1)), rl, W[:, np.arange(n) % distinct]


def _filter(ctx, rng, n_sh):
    F = _rnd(rng, (n_sh,))
    return ctx.upload_dense(F.reshape(-1)), np.arange(n_sh, dtype=np.uint32), F


def _specs(counts, aggs):
    """a few selections with bounds that occur in the data; aggs None: a count-only call"""
    live = np.sort(counts[counts > 0])
    mid, top = (int(live[live.size // 2]), int(live[-1])) if live.size else (1, 2)
    out = [
        dict(),
        dict(offset=2, limit=3),
        dict(sort=[("count", True)], limit=3),
        dict(sort=[("count", False)], offset=1, limit=4),
        dict(sort=[("count", True)]),
        dict(having=("count", "gte", mid, 0)),
        dict(having=("count", "btwn_lt_lte", mid, top), sort=[("count", True)], limit=2),
        dict(having=("count", "neq", mid, 0), offset=1),
        dict(sort=[("count", True)], offset=10 ** 6, limit=5),
    ]
    if aggs is not None:
        s = np.sort(aggs[counts > 0]) if live.size else np.zeros(1, dtype=np.int64)
        a_mid, a_top = int(s[s.size // 2]), int(s[-1])
        out += [
            dict(sort=[("sum", True), ("count", False)], limit=3),
            dict(sort=[("sum", False)], offset=2, limit=3),
            dict(sort=[("count", False), ("sum", True)]),
            dict(having=("sum", "lt", a_mid, 0), sort=[("sum", True)]),
            dict(having=("sum", "between", a_mid, a_top), limit=4),
            dict(having=("sum", "gt", a_mid, 0), sort=[("count", True), ("sum", False)], offset=1, limit=2),
        ]
    return out


def _sel(spec, path):
    hv = spec.get("having")
    return GroupSelect(sort=spec.get("sort"), having=None if hv is None else (hv[0], R.OP_CODE[hv[1]], hv[2], hv[3]), offset=spec.get("offset", 0),
                       limit=spec.get("limit"), path=path)


def _check(call, full_counts, full_aggs, brute_counts, brute_aggs):
    """call(sel) -> (cells, counts[, aggs], matched) against the model over the full call's output and over the brute force"""
    fc, fa = full_counts.reshape(-1), None if full_aggs is None else full_aggs.reshape(-1)
    assert np.array_equal(fc, brute_counts.reshape(-1)) and (fa is None or np.array_equal(fa, brute_aggs.reshape(-1)))
    assert np.unique(fc[fc > 0]).size < (fc > 0).sum(), "the case has no equal counts"
    for spec in _specs(fc, fa):
        for src_c, src_a in ((fc, fa), (brute_counts.reshape(-1), None if fa is None else brute_aggs.reshape(-1))):
            exp, matched = R.select(src_c, src_a, spec.get("sort", ()), spec.get("having"), spec.get("offset", 0), spec.get("limit"))
            for path in ("device", "host"):
                out = call(_sel(spec, path))
                what = (spec, path)
                assert out[-1] == matched, what
                assert list(out[0]) == exp, what
                assert np.array_equal(out[1], src_c[exp]), what
                if fa is not None:
                    assert np.array_equal(out[2], src_a[exp]), what


@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7), (PT + 1, 33, 2)])
def test_cube_select(gpu_ctx, shape, with_filter):
    rng = D.rng_for(9310, *shape, int(with_filter))
    n_sh = 3
    (bP, rp, P), (bA, ra, A), (bB, rb, B) = (_field(gpu_ctx, rng, n_sh, n, d) for n, d in zip(shape, (2, 3, 2)))
    bF, rf, F = _filter(gpu_ctx, rng, n_sh)
    f = (bF, rf) if with_filter else (None, None)
    try:
        full = gpu_ctx.count_cube(bP, rp, bA, ra, bB, rb, *f)
        brute = cube_ref.numpy_expected(P, A, B, F if with_filter else None)
        _check(lambda sel: gpu_ctx.count_cube_select(bP, rp, bA, ra, bB, rb, sel, *f), full, None, brute, None)
    finally:
        for b in (bP, bA, bB, bF):
            b.free()


def test_cube_select_over_encoded_batches(gpu_ctx):
    """array / run / bitmap containers: the densify pass runs in front of the selection"""
    rng = D.rng_for(9311)
    n_sh, (n_p, n_a, n_b) = 3, (2, 5, 7)
    rows = {k: [[D.random_row(rng, 0, p_missing=0.3) for _ in range(d)] for _ in range(n_sh)] for k, d in (("p", 2), ("a", 3), ("b", 2))}
    words = lambda rs: np.stack([np.stack([M.words_of_row(r) for r in sh]) for sh in rs])
    ups, lists, W = {}, {}, {}
    for (k, d), n in zip((("p", 2), ("a", 3), ("b", 2)), (n_p, n_a, n_b)):
        ups[k] = gpu_ctx.upload([D.to_fbk_row(r) for sh in rows[k] for r in sh])
        lists[k] = (np.arange(n_sh, dtype=np.uint32)[:, None] * d + (np.arange(n, dtype=np.uint32) % d)[None, :]).astype(np.uint32)
        W[k] = words(rows[k])[:, np.arange(n) % d]
    try:
        args = (ups["p"], lists["p"], ups["a"], lists["a"], ups["b"], lists["b"])
        full = gpu_ctx.count_cube(*args)
        assert full.any()
        _check(lambda sel: gpu_ctx.count_cube_select(*args, sel), full, None, cube_ref.numpy_expected(W["p"], W["a"], W["b"], None), None)
    finally:
        for b in ups.values():
            b.free()


def _matrix_brute(A, B, F):
    return cube_ref.numpy_expected(np.ones_like(A[:, :1]) * np.uint64((1 << 64) - 1), A, B, F)[0]


@pytest.mark.parametrize("shape", [(5, 7), (33, 65), (300, 1)])
def test_count_matrix_select(gpu_ctx, shape):
    rng = D.rng_for(9312, *shape)
    n_sh, (n_a, n_b) = 3, shape
    bA, ra, A = _field(gpu_ctx, rng, n_sh, n_a, 3)
    bB, rb, B = _field(gpu_ctx, rng, n_sh, n_b, 2)  # (n_b == 1: B is the filter row of the one-field GroupBy)
    bF, rf, F = _filter(gpu_ctx, rng, n_sh)
    f = (None, None) if n_b == 1 else (bF, rf)
    try:
        full = gpu_ctx.count_matrix(bA, ra, bB, rb, *f)
        brute = _matrix_brute(A, B, None if n_b == 1 else F)
        _check(lambda sel: gpu_ctx.count_matrix_select(bA, ra, bB, rb, sel, *f), full, None, brute, None)
    finally:
        for b in (bA, bB, bF):
            b.free()


def _bsi(ctx, rng, n_sh, depth, negative):
    S = _rnd(rng, (n_sh, depth + 2))  # exists, sign, planes
    S[:, 1] = negative  # the columns of these words hold the negative values: their groups' sums are negative, the others' positive
    return ctx.upload_dense(S.reshape(-1)), (np.arange(n_sh, dtype=np.uint32) * (depth + 2)).astype(np.uint32), S


@pytest.mark.parametrize("depth", [0, 5])
@pytest.mark.parametrize("shape", [(5, 7), (33, 2), (33, None)])
def test_count_matrix_sum_select(gpu_ctx, shape, depth):
    n_sh, (n_a, n_b) = 3, shape
    rng = D.rng_for(9313, n_a, n_b or 0, depth)
    bA, ra, A = _field(gpu_ctx, rng, n_sh, n_a, 3)
    bB, rb, B = _field(gpu_ctx, rng, n_sh, n_b or 1, 2)
    bF, rf, F = _filter(gpu_ctx, rng, n_sh)
    bS, base, S = _bsi(gpu_ctx, rng, n_sh, depth, A[:, 0])
    b_args = (bB, rb) if n_b else (None, None)
    try:
        sums, counts = gpu_ctx.count_matrix_sum(bA, ra, *b_args, bS, base, depth, bF, rf)
        e_sums, e_counts = M.numpy_expected(A, B if n_b else None, F, S, depth)
        assert depth == 0 or ((sums < 0).any() and (sums > 0).any())
        _check(lambda sel: gpu_ctx.count_matrix_sum_select(bA, ra, *b_args, bS, base, depth, sel, bF, rf), counts, sums, e_counts, e_sums)
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def test_errors_leave_the_context_usable(gpu_ctx):
    rng = D.rng_for(9314)
    n_sh = 2
    bA, ra, _ = _field(gpu_ctx, rng, n_sh, 5, 3)
    bB, rb, _ = _field(gpu_ctx, rng, n_sh, 7, 2)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cells, oc = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint64)
    n, matched = C.c_uint64(), C.c_uint64()

    def matrix(st, cells_p=cells.ctypes.data, cap=64):
        return lib.fbk_count_matrix_select(h, bA.h, ra.ctypes.data, 5, bB.h, rb.ctypes.data, 7, None, None, n_sh, C.byref(st), cells_p, oc.ctypes.data, cap,
                                           C.byref(n), C.byref(matched))

    def cube(st):
        return lib.fbk_count_cube_select(h, bA.h, ra.ctypes.data, 5, bA.h, ra.ctypes.data, 5, bB.h, rb.ctypes.data, 7, None, None, n_sh, C.byref(st),
                                         cells.ctypes.data, oc.ctypes.data, 64, C.byref(n), C.byref(matched))

    try:
        for call in (matrix, cube):
            for path in ("device", "host"):
                bad = []
                bad.append(GroupSelect(sort="sum desc", path=path).struct())  # the aggregate as a subject of a count-only call
                bad.append(GroupSelect(having="sum > 1", path=path).struct())
                s = GroupSelect(sort="count desc", path=path).struct()
                s.n_sort = 3
                bad.append(s)
                s = GroupSelect(sort="count desc", path=path).struct()
                s.n_sort, s.sort[1].subject = 2, L.GROUPSEL_COUNT  # a repeated subject
                bad.append(s)
                s = GroupSelect(path=path).struct()
                s.flags = L.GROUPSEL_DEVICE | L.GROUPSEL_HOST
                bad.append(s)
                s = GroupSelect(having="count > 1", path=path).struct()
                s.having_op = 0  # an unknown op
                bad.append(s)
                for s in bad:
                    assert call(s) == L.FBK_E_INVALID
                assert call(GroupSelect(sort="count desc", limit=3, path=path).struct()) == L.FBK_OK and n.value == 3
        assert matrix(GroupSelect().struct(), cells_p=None) == L.FBK_E_INVALID  # NULL outputs with cap > 0
        assert matrix(GroupSelect().struct(), cap=1) == L.FBK_E_CAPACITY and n.value == matched.value > 1
        assert matrix(GroupSelect().struct()) == L.FBK_OK
        st = GroupSelect().struct()
        assert lib.fbk_count_matrix_select(h, bA.h, ra.ctypes.data, 5, bB.h, rb.ctypes.data, 7, None, None, 0, C.byref(st), None, None, 0, C.byref(n),
                                           C.byref(matched)) == L.FBK_OK and n.value == 0 and matched.value == 0  # no shards: no groups
    finally:
        bA.free()
        bB.free()
