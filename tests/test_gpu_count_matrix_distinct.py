"""GPU parity of fbk_count_matrix_distinct (GroupBy with aggregate=Count(Distinct(field))): bit-exact against the numpy brute
force of tests/mdist_ref.py (the CPU test shows it agrees with the per-group path).  Dense and encoded batches, the one- and
two-field forms with and without a filter, groups with columns but no value, shards without values, 4096 rows on a side, calls
that tile the presence bitmap (by A rows and by value ranks) and densify in several chunks, and the defining identity: a group's
distinct count is fbk_bsi_distinct's count over the materialised A_i ∩ B_j ∩ F."""
import numpy as np
import pytest

import datagen as D
import mdist_ref as M
from featurebase_amd import lib as L
from featurebase_amd.roaring import Container

pytestmark = pytest.mark.gpu


def _rnd(rng, shape, ands=0):
    w = rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    for _ in range(ands):
        w &= rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    return w


def _dense_case(rng, n_sh, n_a, n_b, depth):
    """random rows; planes 4.. sparse so that values repeat across columns and groups; the sign bit everywhere (also outside
    exists and over magnitude 0); A row 0 without any existing column (a group with columns but no value); shard 1 without
    values"""
    A = _rnd(rng, (n_sh, n_a, 16, 1024))
    Bw = _rnd(rng, (n_sh, n_b, 16, 1024))
    F = _rnd(rng, (n_sh, 16, 1024))
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    S[:, 0] &= _rnd(rng, (n_sh, 16, 1024), 1)
    if depth > 4:
        S[:, 6:] &= _rnd(rng, (n_sh, depth - 4, 16, 1024), 4)
    A[:, 0] &= ~S[:, 0]
    if n_sh > 2:
        S[1, 0] = 0
    return A, Bw, F, S


def _upload_dense(ctx, A, Bw, F, S):
    n_sh, n_a = A.shape[:2]
    bA, bS, bF = ctx.upload_dense(A.reshape(-1)), ctx.upload_dense(S.reshape(-1)), ctx.upload_dense(F.reshape(-1))
    bB = ctx.upload_dense(Bw.reshape(-1)) if Bw is not None else None
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * Bw.shape[1], dtype=np.uint32).reshape(n_sh, -1) if Bw is not None else None
    return bA, ra, bB, rb, bF, np.arange(n_sh, dtype=np.uint32), bS, np.arange(n_sh, dtype=np.uint32) * S.shape[1]


CASES = [(1, 1, 1, 20), (3, 5, 7, 0), (3, 5, 7, 1), (3, 5, 7, 20), (3, 5, 7, 64), (2, 33, 65, 12), (17, 4, 3, 8), (3, 64, None, 20)]


@pytest.mark.parametrize("n_sh,n_a,n_b,depth", CASES)
@pytest.mark.parametrize("with_filter", [False, True])
def test_dense_batches(gpu_ctx, n_sh, n_a, n_b, depth, with_filter):
    rng = D.rng_for(7700, n_sh, n_a, n_b or 0, depth, int(with_filter))
    A, Bw, F, S = _dense_case(rng, n_sh, n_a, n_b or 1, depth)
    if n_b is None:
        Bw = None
    bA, ra, bB, rb, bF, rf, bS, base = _upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        got = gpu_ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
        exp = M.numpy_expected(A, Bw, F if with_filter else None, S, depth)
        assert np.array_equal(got[1], exp[1]), "counts"
        assert np.array_equal(got[0], exp[0]), "distinct"
        assert (exp[0][0] == 0).all()  # A row 0: no value
    finally:
        for b in (bA, bB, bF, bS):
            if b is not None:
                b.free()


def _rows_of_words(W):
    """[n, 16, 1024] words -> n fbk rows of mixed encodings (bitmap slots, array slots, run slots)"""
    out = []
    for r in range(W.shape[0]):
        row = {}
        for sl in range(16):
            w = W[r, sl]
            if not w.any():
                continue
            vals = np.nonzero(np.unpackbits(w.view(np.uint8), bitorder="little"))[0]
            if vals.size < 4096 and sl % 2:
                row[sl] = Container.array(vals)
            else:
                row[sl] = Container.bitmap(w)
        out.append(row)
    return out


def _runs_slot(rng, shape):
    """words with a few long runs of set bits in slot 2"""
    w = np.zeros(shape + (16, 1024), dtype=np.uint64)
    flat = w.reshape(-1, 16, 1024)
    for k in range(flat.shape[0]):
        for _ in range(3):
            lo = int(rng.integers(0, 60000))
            bits = np.zeros(65536, dtype=np.uint8)
            bits[lo:lo + int(rng.integers(100, 5000))] = 1
            flat[k, 2] |= np.packbits(bits, bitorder="little").view(np.uint64)
    return w


@pytest.mark.parametrize("one_field", [False, True])
@pytest.mark.parametrize("with_filter", [False, True])
def test_encoded_batches(gpu_ctx, one_field, with_filter):
    rng = D.rng_for(7800, int(one_field), int(with_filter))
    n_sh, n_a, n_b, depth = 4, 6, 9, 16
    A, Bw, F, S = _dense_case(rng, n_sh, n_a, n_b, depth)
    for X in (A, Bw, F, S):  # sparse slots (arrays), an empty slot, run slots
        X[..., 1::2, :] &= _rnd(rng, X[..., 1::2, :].shape, 5)
        X[..., 4, :] = 0
    A |= _runs_slot(rng, A.shape[:2])
    S[:, 0] |= _runs_slot(rng, (n_sh,))
    if one_field:
        Bw = None
    bA = gpu_ctx.upload(_rows_of_words(A.reshape(-1, 16, 1024)))
    bB = gpu_ctx.upload(_rows_of_words(Bw.reshape(-1, 16, 1024))) if Bw is not None else None
    bF = gpu_ctx.upload(_rows_of_words(F))
    bS = gpu_ctx.upload(_rows_of_words(S.reshape(-1, 16, 1024)))
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b) if Bw is not None else None
    rf, base = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint32) * (depth + 2)
    try:
        got = gpu_ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
        exp = M.numpy_expected(A, Bw, F if with_filter else None, S, depth)
        assert np.array_equal(got[1], exp[1]), "counts"
        assert np.array_equal(got[0], exp[0]), "distinct"
    finally:
        for b in (bA, bB, bF, bS):
            if b is not None:
                b.free()


def _categorical(rng, n_sh, n_rows, cols):
    """one row per column (a hash), the rows of every shard as array containers in slot 0: ([n_sh][n_rows] fbk rows, row of
    each column [n_sh, len(cols)])"""
    which = rng.integers(0, n_rows, (n_sh, cols.size))
    rows = []
    for s in range(n_sh):
        order = np.argsort(which[s], kind="stable")
        bounds = np.searchsorted(which[s][order], np.arange(n_rows + 1))
        for r in range(n_rows):
            c = np.sort(cols[order[bounds[r]:bounds[r + 1]]])
            rows.append({0: Container.array(c)} if c.size else {})
    return rows, which


def _sparse_case(gpu_ctx, rng, n_sh, n_a, n_b, n_vals, depth=14, n_cols=30000):
    """categorical A and B fields of n_a / n_b rows over n_cols columns of slot 0 per shard, values uniform in [0, n_vals) on
    most of them (the rest: no value), a filter on three quarters"""
    cols = np.sort(rng.choice(65536, n_cols, replace=False))
    a_rows, wa = _categorical(rng, n_sh, n_a, cols)
    b_rows, wb = _categorical(rng, n_sh, n_b, cols)
    vals = rng.integers(0, n_vals, (n_sh, n_cols))
    has = rng.random((n_sh, n_cols)) < 0.9
    inf = rng.random((n_sh, n_cols)) < 0.75
    S = np.zeros((n_sh, depth + 2, 16, 1024), dtype=np.uint64)
    F = np.zeros((n_sh, 16, 1024), dtype=np.uint64)
    for s in range(n_sh):
        c = cols[has[s]]
        np.bitwise_or.at(S[s, 0, 0], c >> 6, np.uint64(1) << (c & 63).astype(np.uint64))
        for k in range(depth):
            ck = c[((vals[s][has[s]] >> k) & 1) == 1]
            np.bitwise_or.at(S[s, 2 + k, 0], ck >> 6, np.uint64(1) << (ck & 63).astype(np.uint64))
        cf = cols[inf[s]]
        np.bitwise_or.at(F[s, 0], cf >> 6, np.uint64(1) << (cf & 63).astype(np.uint64))
    bA, bB = gpu_ctx.upload(a_rows), gpu_ctx.upload(b_rows)
    bS, bF = gpu_ctx.upload_dense(S.reshape(-1)), gpu_ctx.upload_dense(F.reshape(-1))

    def expected(with_filter):
        dist = np.zeros(n_a * n_b, dtype=np.uint64)
        counts = np.zeros(n_a * n_b, dtype=np.uint64)
        g_all, v_all = [], []
        for s in range(n_sh):
            m = has[s] & (inf[s] if with_filter else True)
            g = wa[s][m].astype(np.int64) * n_b + wb[s][m]
            counts += np.bincount(g, minlength=n_a * n_b).astype(np.uint64)
            g_all.append(g)
            v_all.append(vals[s][m])
        pairs = np.unique(np.stack([np.concatenate(g_all), np.concatenate(v_all)], axis=1), axis=0)
        dist += np.bincount(pairs[:, 0], minlength=n_a * n_b).astype(np.uint64)
        return dist.reshape(n_a, n_b), counts.reshape(n_a, n_b)

    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    return bA, ra, bB, rb, bF, np.arange(n_sh, dtype=np.uint32), bS, np.arange(n_sh, dtype=np.uint32) * (depth + 2), expected


def _presence_tiles(n_a, n_b, m):
    """the tiles of fbk.h's presence arithmetic: (A row tiles, rank tiles)"""
    wb, m64 = (n_b + 63) // 64, (m + 63) // 64 * 64
    row, budget = 8 * wb * m64, 1 << 27
    if n_a * row <= budget:
        return 1, 1
    if 64 * row <= budget:
        return -(-n_a // (budget // row // 64 * 64)), 1
    ta = min(n_a, 64)
    return -(-n_a // ta), -(-m64 // (budget // (8 * wb * ta) // 64 * 64))


@pytest.mark.parametrize("n_a,n_b,n_vals,with_filter", [(4096, 4096, 1000, False), (4096, 4096, 1000, True), (64, 4096, 6000, True),
                                                        (4096, 1, 3000, True), (7, 4096, 500, False)])
def test_large_shapes_tiles_and_chunks(gpu_ctx, n_a, n_b, n_vals, with_filter):
    """4096 rows on a side; 4096 x 4096 with ~1000 values takes 16 tiles of A rows, 64 x 4096 with ~5500 values two tiles of
    ranks; encoded 4096 x 4096 rows densify 1 GiB per shard: every shard is a chunk of its own"""
    rng = D.rng_for(7900, n_a, n_b, n_vals, int(with_filter))
    n_sh = 3
    bA, ra, bB, rb, bF, rf, bS, base, expected = _sparse_case(gpu_ctx, rng, n_sh, n_a, n_b, n_vals)
    try:
        if n_b == 1:  # the one-field form
            bB.free()
            bB, rb = None, None
        got = gpu_ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, 14, bF if with_filter else None, rf if with_filter else None)
        ed, ec = expected(with_filter)
        assert np.array_equal(got[1], ec), "counts"
        assert np.array_equal(got[0], ed), "distinct"
        m = len(gpu_ctx.bsi_distinct(bS, base, 14, bF if with_filter else None, rf if with_filter else None))
        if (n_a, n_b) == (4096, 4096):
            assert _presence_tiles(n_a, n_b, m) == (16, 1)
        if (n_a, n_b) == (64, 4096):
            assert _presence_tiles(n_a, n_b, m) == (1, 2)
    finally:
        for b in (bA, bB, bF, bS):
            if b is not None:
                b.free()


def test_identity_with_bsi_distinct(gpu_ctx):
    """distinct[i][j] == len(fbk_bsi_distinct over A_i ∩ B_j ∩ F), the intersections materialised with fbk_setop"""
    rng = D.rng_for(8000)
    n_sh, n_a, n_b, depth = 3, 5, 6, 20
    A, Bw, F, S = _dense_case(rng, n_sh, n_a, n_b, depth)
    bA, ra, bB, rb, bF, rf, bS, base = _upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        dist, _ = gpu_ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, depth, bF, rf)
        for (i, j) in [(0, 0), (1, 2), (4, 5), (3, 1)]:
            ab, _ = gpu_ctx.setop(L.OP_AND, bA, ra[:, i], bB, rb[:, j])
            abf, _ = gpu_ctx.setop(L.OP_AND, ab, np.arange(n_sh, dtype=np.uint32), bF, rf)
            try:
                vals = gpu_ctx.bsi_distinct(bS, base, depth, abf, np.arange(n_sh, dtype=np.uint32))
                assert int(dist[i, j]) == len(vals), (i, j)
            finally:
                ab.free()
                abf.free()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def test_errors_then_recovery(gpu_ctx):
    rng = D.rng_for(8100)
    A, Bw, F, S = _dense_case(rng, 2, 3, 4, 8)
    bA, ra, bB, rb, bF, rf, bS, base = _upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        with pytest.raises(L.FbkError):
            gpu_ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base + 100, 8)  # fragment rows past the batch
        with pytest.raises(L.FbkError):
            gpu_ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, 65)  # depth > 64
        got = gpu_ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, 8)
        assert np.array_equal(got[0], M.numpy_expected(A, Bw, None, S, 8)[0])
    finally:
        for b in (bA, bB, bF, bS):
            b.free()
