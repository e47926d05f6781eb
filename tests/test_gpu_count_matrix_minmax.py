"""GPU parity of fbk_count_matrix_minmax (GroupBy with Min / Max of an int field per group).  Every case runs the three path pins
— AUTO, DESCENT (where n_a * n_b is within its cap) and SCATTER —, which must agree bit for bit with each other and with the numpy
brute force for every pair (tests/minmax_ref.py); where the data has neither a sign bit over magnitude 0 nor a magnitude of 2^63
or more, sampled pairs are also checked against the reference's composition (the CPU test shows the two agree there).  Dense
batches over shard counts, shapes on both sides of the path rule and depths 0..64; mutex-like rows with few distinct values;
counts=False; the one-field form; encoded batches (the densify path); calls that densify in more than one chunk; 19 shards, at
which every kernel goes round its grid-stride loop more than once (by steps that are no whole number of shards, too); the row-list
limits; recovery after an error."""
import numpy as np
import pytest

import datagen as D
import minmax_ref as M
import test_gpu_count_matrix_sum as T  # its builders of dense and encoded cases
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu

AUTO, DESCENT, SCATTER = L.MINMAX_AUTO, L.MINMAX_DESCENT, L.MINMAX_SCATTER


@pytest.fixture(scope="module")
def B(oracle):
    from oracle import pybsi

    pybsi._lib()
    return pybsi


@pytest.fixture(scope="module")
def plan():
    return M.plan_constants()  # (kMinmaxDescentCells, kMinmaxDescentMaxCells)


def _all_paths(ctx, plan, n_cells, *args, counts=True, **kw):
    """the call under every pin that takes the shape; the results must be identical.  Returns AUTO's."""
    got = {p: ctx.count_matrix_minmax(*args, counts=counts, path=p, **kw) for p in ([AUTO, DESCENT, SCATTER] if n_cells <= plan[1] else [AUTO, SCATTER])}
    for p, g in got.items():
        for k, name in enumerate(("mins", "maxs", "min_counts", "max_counts")):
            if counts:
                assert np.array_equal(g[k], got[AUTO][k]), (name, "path", p)
            elif k >= 2:
                assert g[k] is None
            else:
                assert np.array_equal(g[k], got[AUTO][k]), (name, "path", p)
    return got[AUTO]


def _equal(got, exp, counts=True, what=()):
    for k, name in enumerate(("mins", "maxs", "min_counts", "max_counts")[: 4 if counts else 2]):
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, what + (name, bad[:4].tolist(), got[k][tuple(bad[0])], exp[k][tuple(bad[0])])


def _clean(S, depth):
    """no sign over magnitude 0 and no magnitude >= 2^63 inside exists: what the reference's composition agrees on"""
    if depth == 64:
        S[:, 65] &= ~S[:, 0]
    anymag = np.bitwise_or.reduce(S[:, 2:], axis=1) if depth else np.zeros_like(S[:, 0])
    S[:, 1] &= anymag | ~S[:, 0]


def _check_oracle(O, B, rng, got, A, Bw, F, S, depth, a_bms=None, b_bms=None, f_bms=None, frags=None, k=4):
    n_sh, n_a = A.shape[:2]
    n_b = Bw.shape[1] if Bw is not None else 1
    pairs = T._sample_pairs(rng, n_a, n_b, k)
    if a_bms is None:
        a_bms = [{i: M.bitmap_of_words(O, A[s, i]) for i, _ in pairs} for s in range(n_sh)]
        b_bms = [{j: M.bitmap_of_words(O, Bw[s, j]) for _, j in pairs} for s in range(n_sh)] if Bw is not None else None
        f_bms = [M.bitmap_of_words(O, F[s]) for s in range(n_sh)] if F is not None else None
        frags = [M.fragment_of_words(O, B, S[s]) for s in range(n_sh)]
    for (i, j), want in M.oracle_expected(O, B, a_bms, b_bms, f_bms, frags, depth, pairs).items():
        assert (int(got[0][i, j]), int(got[1][i, j]), int(got[2][i, j]), int(got[3][i, j])) == want, (i, j)


# shapes: one group; a few; one full tile of the descent; one tile by rows; more B rows than a transpose holds; "cells" / "next" /
# "cap": n_a * n_b exactly kMinmaxDescentCells (AUTO's last descent), one more (its first scatter) and exactly the descent's cap;
# (33, 65) is above the cap
SHAPES = [(1, 1), (5, 7), (8, 8), (64, 1), (3, 70), "cells", "next", "cap", (33, 65)]
DEPTHS = [0, 1, 7, 20, 63, 64]
DENSE_CASES = [(n_sh, sh, DEPTHS[k % 6], k % 2 == 1, k % 4 < 2) for k, (sh, n_sh) in enumerate((sh, s) for sh in SHAPES for s in (1, 3))]
DENSE_CASES += [(3, (5, 7), d, f, not f) for d in DEPTHS for f in (False, True)]


@pytest.mark.parametrize("n_sh,shape,depth,with_filter,clean", DENSE_CASES)
def test_dense_batches(gpu_ctx, oracle, B, plan, n_sh, shape, depth, with_filter, clean):
    n_a, n_b = {"cells": (plan[0] // 8, 8), "next": (plan[0] + 1, 1), "cap": (plan[1] // 32, 32)}.get(shape, shape)
    rng = D.rng_for(8200, n_sh, n_a, n_b, depth, int(with_filter))
    A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=1 if n_a * n_b <= 64 else 6)  # (a shard without values, an empty container)
    if clean:
        _clean(S, depth)
    Fx = F if with_filter else None
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        got = _all_paths(gpu_ctx, plan, n_a * n_b, bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
        _equal(got, M.numpy_expected(A, Bw, Fx, S, depth))
        if clean:
            _check_oracle(oracle, B, rng, got, A, Bw, Fx, S, depth)
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


N_COLS = 2 << 16  # the mutex-like cases keep their columns in the first two containers of a shard


def _words_of_mask(mask):
    """[..., N_COLS] bool -> [..., 16, 1024] uint64"""
    w = np.zeros(mask.shape[:-1] + (16, 1024), dtype=np.uint64)
    w[..., :2, :] = np.packbits(mask, axis=-1, bitorder="little").view(np.uint64).reshape(mask.shape[:-1] + (2, 1024))
    return w


def _mutex_case(rng, n_sh, n_a, n_b, depth, values):
    """every column in exactly one A row (never row 0) and one B row; three quarters of them with a value drawn from `values`
    (a pair (sign, magnitude) each); sign and plane bits also on columns without exists"""
    ia, jb = rng.integers(1, n_a, (n_sh, N_COLS)), rng.integers(0, n_b, (n_sh, N_COLS))
    A = _words_of_mask(ia[:, None, :] == np.arange(n_a)[None, :, None])
    Bw = _words_of_mask(jb[:, None, :] == np.arange(n_b)[None, :, None])
    pick = rng.integers(0, len(values), (n_sh, N_COLS))
    sign = np.array([v[0] for v in values], dtype=bool)[pick]
    mag = np.array([v[1] for v in values], dtype=np.uint64)[pick]
    rows = [rng.random((n_sh, N_COLS)) < 0.75, sign] + [((mag >> np.uint64(k)) & np.uint64(1)).astype(bool) for k in range(depth)]
    S = _words_of_mask(np.stack(rows, axis=1))
    F = T._rnd(rng, (n_sh, 16, 1024))
    return A, Bw, F, S


FEW = [(True, 9), (True, 2), (False, 0), (True, 0), (False, 2), (False, 9), (False, 1000)]
MUTEX_CASES = [
    (16, 16, 20, FEW, "few"),
    (300, 20, 20, FEW, "few"),
    (16, 16, 7, [(False, 77)], "same"),       # every column the same value: the holders pass under contention
    (16, 16, 7, [(True, 5), (True, 5), (True, 120)], "negatives"),
    (16, 16, 20, [(True, 0)], "sign over zero"),  # the only members: value 0
    (16, 16, 64, [(True, (1 << 64) - 1), (False, (1 << 63) + 5), (False, 3), (True, 1 << 63)], "65 bits"),
]


@pytest.mark.parametrize("n_a,n_b,depth,values,what", MUTEX_CASES)
def test_mutex_like_rows(gpu_ctx, plan, n_a, n_b, depth, values, what):
    rng = D.rng_for(8300, n_a, n_b, depth, len(values))
    n_sh = 2
    A, Bw, F, S = _mutex_case(rng, n_sh, n_a, n_b, depth, values)
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        for with_filter in (False, True):
            got = _all_paths(gpu_ctx, plan, n_a * n_b, bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
            exp = M.numpy_expected(A, Bw, F if with_filter else None, S, depth)
            _equal(got, exp)
            # A row 0 holds no column: the sentinels, counts 0
            assert (got[0][0] == M.INT64_MAX).all() and (got[1][0] == M.INT64_MIN).all() and not got[2][0].any() and not got[3][0].any()
            assert (got[2][1:] > 1).any() and (got[3][1:] > 1).any()
            if what == "same":
                assert (got[0][1:] == 77).all() and (got[1][1:] == 77).all() and np.array_equal(got[2], got[3]) and got[2][1:].min() > 50
            if what == "negatives":
                assert (got[0][1:] == -120).all() and (got[1][1:] == -5).all()
            if what == "sign over zero":
                assert not got[0][1:].any() and not got[1][1:].any() and np.array_equal(got[2], got[3]) and got[2][1:].min() > 50
            if what == "65 bits" and not with_filter:  # by value, not by the wrapped int64: -(2^64 - 1) is written 1, 2^63 + 5 wraps
                assert (got[0][1:] == 1).all() and (got[1][1:] == M.INT64_MIN + 5).all()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


@pytest.mark.parametrize("n_a,n_b", [(5, 7), (33, 65)])
def test_without_counts(gpu_ctx, plan, n_a, n_b):
    rng = D.rng_for(8400, n_a, n_b)
    n_sh, depth = 2, 20
    A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=5)
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        got = _all_paths(gpu_ctx, plan, n_a * n_b, bA, ra, bB, rb, bS, base, depth, bF, rf, counts=False)
        _equal(got, M.numpy_expected(A, Bw, F, S, depth), counts=False)
        with pytest.raises(L.FbkError) as e:  # one count pointer only
            L.check(gpu_ctx.lib.fbk_count_matrix_minmax(gpu_ctx.h, bA.h, ra.ctypes.data, n_a, bB.h, rb.ctypes.data, n_b, None, None, bS.h, base.ctypes.data, depth,
                                                        n_sh, 0, got[0].ctypes.data, got[1].ctypes.data, np.zeros(n_a * n_b, np.uint64).ctypes.data, None))
        assert e.value.code == L.FBK_E_INVALID
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


@pytest.mark.parametrize("depth", [0, 20, 64])
def test_one_field_dense(gpu_ctx, oracle, B, plan, depth):
    rng = D.rng_for(8500, depth)
    n_sh, n_a = 3, 70
    A, _, F, S = T._dense_case(rng, n_sh, n_a, 1, depth, exists_ands=3)
    _clean(S, depth)
    bA, ra, _, _, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, None, F, S)
    try:
        for with_filter in (False, True):
            got = _all_paths(gpu_ctx, plan, n_a, bA, ra, None, None, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
            _equal(got, M.numpy_expected(A, None, F if with_filter else None, S, depth))
            _check_oracle(oracle, B, rng, got, A, None, F if with_filter else None, S, depth)
        with pytest.raises(L.FbkError):  # without B rows n_b must be 1
            o = [np.zeros(2 * n_a, t) for t in (np.int64, np.int64, np.uint64, np.uint64)]
            L.check(gpu_ctx.lib.fbk_count_matrix_minmax(gpu_ctx.h, bA.h, ra.ctypes.data, n_a, None, None, 2, None, None, bS.h, base.ctypes.data, depth, n_sh, 0,
                                                        *[x.ctypes.data for x in o]))
    finally:
        for b in (bA, bF, bS):
            b.free()


@pytest.mark.parametrize("depth", [0, 7, 20, 63])
def test_encoded_batches(gpu_ctx, oracle, B, plan, depth):
    """mixed containers, rows missing in some shards, BSI fragments from bsi_fragment_from_values (no sign over zero)"""
    rng = D.rng_for(8600, depth)
    n_sh, n_a, n_b = 5, 6, 9
    a_rows, b_rows, f_rows, frags, A, Bw, F, S, (abm, bbm, fbm) = T._encoded_case(oracle, B, rng, n_sh, n_a, n_b, depth)
    flat = lambda rows: [D.to_fbk_row(r) for sh in rows for r in sh]
    bA, bB = gpu_ctx.upload(flat(a_rows)), gpu_ctx.upload(flat(b_rows))
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    bF = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    bS, base = T._upload_bsi(gpu_ctx, frags)
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        for with_filter in (False, True):
            got = _all_paths(gpu_ctx, plan, n_a * n_b, bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
            _equal(got, M.numpy_expected(A, Bw, F if with_filter else None, S, depth))
            _check_oracle(oracle, B, rng, got, A, Bw, F if with_filter else None, S, depth, abm, bbm, fbm if with_filter else None, frags, k=6)
        got = _all_paths(gpu_ctx, plan, n_a, bA, ra, None, None, bS, base, depth, bF, rf)  # the one-field form over encoded rows
        _equal(got, M.numpy_expected(A, None, F, S, depth))
        _check_oracle(oracle, B, rng, got, A, None, F, S, depth, abm, None, fbm, frags, k=6)
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def _chunk(n_shards, densified_rows):
    """the densify chunk of a call (include/fbk.h, fbk_count_matrix_minmax)"""
    most = max(1, min(n_shards, (1 << 30) // ((1 << 17) * densified_rows)))
    passes = -(-n_shards // most)
    return -(-n_shards // passes)


@pytest.mark.parametrize("n_sh,n_a,two_fields,chunk", [(8, 1024, False, 4), (3, 4096, True, 1)])
def test_densify_in_several_chunks(gpu_ctx, oracle, B, plan, n_sh, n_a, two_fields, chunk):
    """encoded batches and a long row list (cycling over 8 stored rows per shard): 1024 rows (every path) and the BSI rows take two
    chunks of four shards; 4096 x 2 rows (the scatter, walking twice for the counts) one shard at a time"""
    rng = D.rng_for(8700, n_sh, n_a)
    depth, stored, n_b = 20, 8, 2 if two_fields else 1
    assert _chunk(n_sh, n_a + (n_b if two_fields else 0) + 1 + depth + 2) == chunk < n_sh
    a_rows, b_rows, f_rows, frags, A, Bw, F, S, _ = T._encoded_case(oracle, B, rng, n_sh, stored, 2, depth, n_vals=3000)
    bA = gpu_ctx.upload([D.to_fbk_row(r) for sh in a_rows for r in sh])
    bB = gpu_ctx.upload([D.to_fbk_row(r) for sh in b_rows for r in sh])
    bF = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    bS, base = T._upload_bsi(gpu_ctx, frags)
    cyc = np.arange(n_a) % stored
    ra = (np.arange(n_sh)[:, None] * stored + cyc[None, :]).astype(np.uint32)
    rb = np.arange(n_sh * 2, dtype=np.uint32).reshape(n_sh, 2)
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        got = _all_paths(gpu_ctx, plan, n_a * n_b, bA, ra, bB if two_fields else None, rb if two_fields else None, bS, base, depth, bF, rf)
        exp8 = M.numpy_expected(A, Bw if two_fields else None, F, S, depth)
        _equal(got, tuple(e[cyc] for e in exp8))
        assert (got[2] > 0).any() and (got[0] < got[1]).any()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


# 19 shards: on one tile two whole rounds of 8 shards of either kernel's grid and a partial one.  (5, 7): one tile, the descent
# steps by exactly 8 shards and the scatter by 8192 units.  (13, 11): 3 tiles, the descent's grid is 682 blocks = 2728 units a step,
# no multiple of a shard's 1024, so the steps advance by 2 or 3 shards, and k_minmax_fold gets 682 partials.  (33, 65): above the
# descent's cap, two words of B rows.  (70, None): the one-field form, two tiles.  tests/test_count_matrix_minmax_cpu.py shows what
# these numbers rest on, and that the data tells a shard skipped beyond the first round.
MANY_SHARD_CASES = [((5, 7), (AUTO, DESCENT, SCATTER)), ((13, 11), (DESCENT, SCATTER)), ((33, 65), (AUTO, SCATTER)), ((70, None), (AUTO, DESCENT, SCATTER))]


@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("depth", [7, 20])
@pytest.mark.parametrize("shape,pins", MANY_SHARD_CASES)
def test_launches_that_go_round_their_loops(gpu_ctx, plan, shape, pins, depth, with_filter):
    n_a, n_b = shape
    assert DESCENT not in pins or n_a * (n_b or 1) <= plan[1]
    A, Bw, F, S = M.many_shard_case(n_a, n_b, depth)
    bA, _, bB, _, bF, _, bS, _ = T._upload_dense(gpu_ctx, A, Bw, F, S)
    ra, rb, rf, base = M.many_shard_lists(n_a, n_b, depth)
    try:
        gA, gB, gF, gS = M.many_shard_words(A, Bw, F, S)
        exp = M.numpy_expected(gA, gB, gF if with_filter else None, gS, depth)
        assert (exp[2] > 0).sum() * 2 > exp[2].size
        for p in pins:
            for counts in (True, False):
                got = gpu_ctx.count_matrix_minmax(bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None, counts=counts, path=p)
                assert counts or (got[2] is None and got[3] is None)
                _equal(got, exp, counts=counts, what=("path", p, "counts", counts))
    finally:
        for b in (bA, bB, bF, bS):
            if b is not None:
                b.free()


def test_row_list_limits(gpu_ctx, plan):
    """n_a = 4096 (the most a side takes) x n_b = 2 over 8 stored dense rows; 4097 is an error"""
    rng = D.rng_for(8800)
    n_sh, stored, n_a, depth = 2, 8, 4096, 20
    A, Bw, F, S = T._dense_case(rng, n_sh, stored, 2, depth, exists_ands=4)
    bA, _, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    cyc = np.arange(n_a) % stored
    ra = (np.arange(n_sh)[:, None] * stored + cyc[None, :]).astype(np.uint32)
    try:
        got = _all_paths(gpu_ctx, plan, n_a * 2, bA, ra, bB, rb, bS, base, depth, bF, rf)
        _equal(got, tuple(e[cyc] for e in M.numpy_expected(A, Bw, F, S, depth)))
        ra1 = (np.arange(n_sh)[:, None] * stored + (np.arange(n_a + 1) % stored)[None, :]).astype(np.uint32)
        with pytest.raises(L.FbkError) as e:
            gpu_ctx.count_matrix_minmax(bA, ra1, bB, rb, bS, base, depth)
        assert e.value.code == L.FBK_E_INVALID
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def test_errors_then_recovery(gpu_ctx, plan):
    rng = D.rng_for(8900)
    n_sh, n_a, n_b, depth = 2, 33, 65, 8  # above the descent's cap
    A, Bw, F, S = T._dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=6)
    bA, ra, bB, rb, bF, rf, bS, base = T._upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        assert n_a * n_b > plan[1]
        good = M.numpy_expected(A[:, :3], Bw[:, :4], F, S, depth)
        bad = base.copy()
        bad[1] = n_sh * (depth + 2) - 1  # the fragment's rows run past the batch
        for call in (lambda: gpu_ctx.count_matrix_minmax(bA, ra, bB, rb, bS, base, depth, path=DESCENT),
                     lambda: gpu_ctx.count_matrix_minmax(bA, ra, bB, rb, bS, bad, depth),
                     lambda: gpu_ctx.count_matrix_minmax(bA, ra, bB, rb, bS, base, 65),
                     lambda: gpu_ctx.count_matrix_minmax(bA, ra, bB, rb, bS, base, depth, path=3),
                     lambda: gpu_ctx.count_matrix_minmax(bA, ra + np.uint32(n_sh * n_a), bB, rb, bS, base, depth)):
            with pytest.raises(L.FbkError) as e:
                call()
            assert e.value.code == L.FBK_E_INVALID
            got = gpu_ctx.count_matrix_minmax(bA, ra[:, :3], bB, rb[:, :4], bS, base, depth, bF, rf)  # the next good call
            _equal(got, good)
        # no shards: the empty-group values
        o = [np.ones(12, t) for t in (np.int64, np.int64, np.uint64, np.uint64)]
        L.check(gpu_ctx.lib.fbk_count_matrix_minmax(gpu_ctx.h, bA.h, ra.ctypes.data, 3, bB.h, rb.ctypes.data, 4, None, None, bS.h, base.ctypes.data, depth, 0, 0,
                                                    *[x.ctypes.data for x in o]))
        assert (o[0] == M.INT64_MAX).all() and (o[1] == M.INT64_MIN).all() and not o[2].any() and not o[3].any()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()
