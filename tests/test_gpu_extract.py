"""GPU parity of fbk_extract_* (Extract(Limit(filter, limit=, offset=), Rows(f1), ...)): bit-exact against the numpy brute force
of tests/extract_ref.py (the CPU test shows it agrees with the reference's per-row / per-plane procedure on the oracle's rows).
Dense and encoded filter / BSI / set-field batches in every combination, bit depths 0 .. 64 with sign bits everywhere, shards
without values or without selected columns, shard ids with gaps and beyond 2^32 columns, 1 .. 4096 field rows, offset / limit
boundaries, the capacity protocol, calls that densify in several chunks, identities with the existing calls, and handles that
live side by side."""
import ctypes as C

import numpy as np
import pytest

import datagen as D
import extract_ref as X
from featurebase_amd import lib as L
from featurebase_amd.roaring import Container

pytestmark = pytest.mark.gpu

U64MAX = (1 << 64) - 1


def _rnd(rng, shape, ands=0):
    w = rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    for _ in range(ands):
        w &= rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    return w


def _rows_of_words(W):
    """[n, 16, 1024] words -> n fbk rows of mixed encodings: bitmap slots, array slots (odd slots under 4096 values), run slots
    (slot 2 when it is made of few runs), absent slots"""
    out = []
    for r in range(W.shape[0]):
        row = {}
        for sl in range(16):
            w = W[r, sl]
            if not w.any():
                continue
            b = np.unpackbits(w.view(np.uint8), bitorder="little")
            vals = np.nonzero(b)[0]
            edges = np.nonzero(np.diff(np.concatenate(([0], b, [0])).astype(np.int8)))[0]
            if sl == 2 and edges.size <= 64:
                row[sl] = Container.run([(int(edges[k]), int(edges[k + 1]) - 1) for k in range(0, edges.size, 2)])
            elif vals.size < 4096 and sl % 2:
                row[sl] = Container.array(vals)
            else:
                row[sl] = Container.bitmap(w)
        out.append(row)
    return out


def _runs(rng, shape):
    """[shape, 1024] words of three long runs of set bits"""
    w = np.zeros(shape + (1024,), dtype=np.uint64)
    flat = w.reshape(-1, 1024)
    for k in range(flat.shape[0]):
        bits = np.zeros(65536, dtype=np.uint8)
        for _ in range(3):
            lo = int(rng.integers(0, 60000))
            bits[lo:lo + int(rng.integers(100, 5000))] = 1
        flat[k] = np.packbits(bits, bitorder="little").view(np.uint64)
    return w


def _case(rng, n_sh, n_a, depth, density_ands=1):
    """filter at 2^-(1 + density_ands) in the even slots, sparse in the odd ones (arrays when encoded), runs in slot 2, slot 4
    absent; exists about half the columns; sign and plane bits everywhere (outside exists, over magnitude 0); shard 1 without
    a value; the last shard's columns 0 / 1: selected, in no row / in every row"""
    F = _rnd(rng, (n_sh, 16, 1024), density_ands)
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    A = _rnd(rng, (n_sh, n_a, 16, 1024), 1)
    for Y in (F, S, A):
        Y[..., 1::2, :] &= _rnd(rng, Y[..., 1::2, :].shape, 5)
        Y[..., 4, :] = 0
        Y[..., 2, :] = _runs(rng, Y.shape[:-2])
    S[:, 2:, 0, :4] = 0  # magnitude 0 on the first 256 columns (the sign bit stays)
    if n_sh > 1:
        S[1, 0] = 0
    F[-1, 0, 0] |= np.uint64(3)
    A[-1, :, 0, 0] &= ~np.uint64(1)
    A[-1, :, 0, 0] |= np.uint64(2)
    return F, S, A


def _upload(ctx, W, encoded):
    """[n, 16, 1024] words -> batch"""
    W = np.ascontiguousarray(W).reshape(-1, 16, 1024)
    return ctx.upload(_rows_of_words(W)) if encoded else ctx.upload_dense(W.reshape(-1))


def _check(ctx, h, F, ids, offset, limit, bS=None, S=None, depth=0, bA=None, A=None, rows_f=None, base=None, ra=None):
    sh, pos, cols = X.select(F, ids, offset, limit)
    assert h.n == cols.size, (h.n, cols.size)
    got = h.columns()
    assert got.dtype == np.uint64 and np.array_equal(got, cols), "columns"
    if bS is not None:
        n_sh = F.shape[0]
        base = np.arange(n_sh, dtype=np.uint32) * (depth + 2) if base is None else base
        vals, pres = h.bsi(bS, base, depth)
        ev, ep = X.bsi_expected(S, depth, sh, pos)
        assert np.array_equal(pres, ep), "present"
        assert np.array_equal(vals, ev), "values"
    if bA is not None:
        n_sh, n_a = F.shape[0], A.shape[1]
        ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a) if ra is None else ra
        offs, items = h.rows(bA, ra)
        eo, ei = X.rows_expected(A, sh, pos)
        assert np.array_equal(offs, eo), "offsets"
        assert items.dtype == np.uint32 and np.array_equal(items, ei), "items"
    return sh, pos, cols


@pytest.fixture(scope="module")
def small():
    rng = D.rng_for(8100)
    return _case(rng, 3, 5, 20)


@pytest.mark.parametrize("enc_f", [False, True])
@pytest.mark.parametrize("enc_s", [False, True])
@pytest.mark.parametrize("enc_a", [False, True])
def test_dense_and_encoded_combinations(gpu_ctx, small, enc_f, enc_s, enc_a):
    F, S, A = small
    ids = [0, 1, 4]
    bF, bS, bA = _upload(gpu_ctx, F, enc_f), _upload(gpu_ctx, S, enc_s), _upload(gpu_ctx, A, enc_a)
    try:
        with gpu_ctx.extract(bF, np.arange(3), ids) as h:
            sh, pos, cols = _check(gpu_ctx, h, F, ids, 0, None, bS, S, 20, bA, A)
            assert h.span() == (0, 3) and cols.size > 100000
        with gpu_ctx.extract(bF, np.arange(3), ids, offset=int((sh == 0).sum()) + 77, limit=12345) as h:
            _check(gpu_ctx, h, F, ids, int((sh == 0).sum()) + 77, 12345, bS, S, 20, bA, A)
            assert h.span() == (1, 1)
    finally:
        for b in (bF, bS, bA):
            b.free()


@pytest.mark.parametrize("depth", [0, 1, 20, 64])
def test_bit_depths_signs_gaps_and_large_shard_ids(gpu_ctx, depth):
    rng = D.rng_for(8200, depth)
    n_sh = 5
    F, S, A = _case(rng, n_sh, 2, depth, 3)
    F[2] = 0  # a shard with an empty filter row
    if depth == 64:
        S[:, 40:] |= _rnd(rng, (n_sh, 26, 16, 1024), 2)  # magnitudes near 2^64: int64 wrap-around
    ids = [0, 1, 4, 1 << 40, (1 << 40) + 3]
    bF, bS = _upload(gpu_ctx, F, False), _upload(gpu_ctx, S, depth == 20)
    try:
        with gpu_ctx.extract(bF, np.arange(n_sh), ids) as h:
            sh, pos, cols = _check(gpu_ctx, h, F, ids, 0, None, bS, S, depth)
            assert int(cols[-1]) >> 20 == (1 << 40) + 3 and not (sh == 2).any()
            vals, pres = X.bsi_expected(S, depth, sh, pos)
            assert not pres[sh == 1].any() and pres.any() and (~pres).any()
            if depth:
                assert (vals < 0).any() and (vals[pres] == 0).any()
    finally:
        bF.free()
        bS.free()


@pytest.mark.parametrize("n_a", [1, 2, 64, 65])
def test_field_row_counts(gpu_ctx, n_a):
    rng = D.rng_for(8300, n_a)
    F, S, A = _case(rng, 2, n_a, 0, 4)
    bF, bA = _upload(gpu_ctx, F, False), _upload(gpu_ctx, A, n_a == 65)
    try:
        with gpu_ctx.extract(bF, np.arange(2), [0, 1]) as h:
            sh, pos, cols = _check(gpu_ctx, h, F, [0, 1], 0, None, bA=bA, A=A)
            offs, items = h.rows(bA, np.arange(2 * n_a).reshape(2, n_a))
            k0 = int(np.nonzero(cols == (1 << 20))[0][0])  # the last shard's columns 0 and 1
            assert offs[k0 + 1] == offs[k0] and offs[k0 + 2] - offs[k0 + 1] == n_a  # in no row; in every row
    finally:
        bF.free()
        bA.free()


def test_4096_rows_dense(gpu_ctx):
    rng = D.rng_for(8400)
    n_a = 4096
    F = np.zeros((1, 16, 1024), dtype=np.uint64)
    F[0, 0, :3] = _rnd(rng, (3,))
    F[0, 9, 1000:1002] = _rnd(rng, (2,))
    A = np.zeros((1, n_a, 16, 1024), dtype=np.uint64)
    A[0, :, 0, :3] = _rnd(rng, (n_a, 3), 4)
    A[0, :, 9, 1000:1002] = _rnd(rng, (n_a, 2), 1)
    F[0, 0, 0] |= np.uint64(1)
    A[0, :, 0, 0] |= np.uint64(1)  # the first column: in all 4096 rows
    bF, bA = _upload(gpu_ctx, F, False), _upload(gpu_ctx, A, False)
    try:
        with gpu_ctx.extract(bF, [0], [7]) as h:
            _check(gpu_ctx, h, F, [7], 0, None, bA=bA, A=A)
            offs, _ = h.rows(bA, np.arange(n_a).reshape(1, n_a))
            assert offs[1] == n_a
    finally:
        bF.free()
        bA.free()


def test_offset_limit_boundaries(gpu_ctx):
    rng = D.rng_for(8500)
    n_sh, n_a, depth = 3, 3, 8
    F = np.zeros((n_sh, 16, 1024), dtype=np.uint64)
    F[:, 0, :40] = _rnd(rng, (n_sh, 40))
    F[:, 15, 1000:] = _rnd(rng, (n_sh, 24), 2)
    F[0, 0, 0] = np.uint64(U64MAX)
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    A = _rnd(rng, (n_sh, n_a, 16, 1024), 1)
    ids = [2, 3, 9]
    sh, _, _ = X.select(F, ids)
    total, c0, c01 = sh.size, int((sh == 0).sum()), int((sh <= 1).sum())
    w0 = 64 + bin(int(F[0, 0, 1])).count("1")  # the columns of shard 0's first two words
    bF, bS, bA = _upload(gpu_ctx, F, False), _upload(gpu_ctx, S, False), _upload(gpu_ctx, A, False)
    sweeps = [(0, None), (3, 10), (64, 64), (64, w0 - 64), (w0, 1), (5, w0 - 5), (c0, None), (c0 - 1, 2), (c0, c01 - c0), (c0 + 5, c01 - c0),
              (0, c0), (0, 0), (7, 0), (total, None), (total, 5), (total + 7, None), (total - 1, None), (U64MAX, 5), (3, U64MAX), (3, U64MAX - 1),
              (c01 + 1, U64MAX - 2), (1, total - 2)]
    try:
        for off, lim in sweeps:
            with gpu_ctx.extract(bF, np.arange(n_sh), ids, offset=off, limit=lim) as h:
                esh, _, _ = _check(gpu_ctx, h, F, ids, off, lim, bS, S, depth, bA, A)
                if esh.size:
                    assert h.span() == (int(esh[0]), int(esh[-1]) - int(esh[0]) + 1), (off, lim)
                else:
                    assert h.n == 0 and h.span()[1] == 0
                    offs, items = h.rows(bA, np.arange(n_sh * n_a).reshape(n_sh, n_a))
                    assert offs.tolist() == [0] and items.size == 0
    finally:
        for b in (bF, bS, bA):
            b.free()


def test_empty_inputs(gpu_ctx):
    F = np.zeros((2, 16, 1024), dtype=np.uint64)
    bF = _upload(gpu_ctx, F, False)
    bE = _upload(gpu_ctx, F, True)
    try:
        for b, rows, ids in ((bF, [0, 1], [0, 1]), (bE, [0, 1], [5, 6]), (bF, [], [])):
            with gpu_ctx.extract(b, rows, ids) as h:
                assert h.n == 0 and h.columns().size == 0 and h.span() == (0, 0)
                vals, pres = h.bsi(bF, np.zeros(len(rows), dtype=np.uint32), 0)
                assert vals.size == 0 and pres.size == 0
    finally:
        bF.free()
        bE.free()


def test_capacity_protocol(gpu_ctx, small):
    F, S, A = small
    bF, bA = _upload(gpu_ctx, F, False), _upload(gpu_ctx, A, False)
    try:
        with gpu_ctx.extract(bF, np.arange(3), [0, 1, 4], offset=1000, limit=5000) as h:
            sh, pos, _ = X.select(F, [0, 1, 4], 1000, 5000)
            eo, ei = X.rows_expected(A, sh, pos)
            ra = np.arange(15, dtype=np.uint32).reshape(3, 5)
            offs, items, m = np.full(h.n + 1, 77, dtype=np.uint64), np.full(16, 0xABCD, dtype=np.uint32), C.c_uint64(5)
            rc = gpu_ctx.lib.fbk_extract_rows(gpu_ctx.h, h.h, bA.h, ra.ctypes.data, 5, offs.ctypes.data, items.ctypes.data, 16, C.byref(m))
            assert rc == L.FBK_E_CAPACITY and m.value == ei.size > 16
            assert np.array_equal(offs, eo) and (items == 0xABCD).all()
            o2, i2 = h.rows(bA, ra, cap=1)  # the wrapper retries once with the reported size
            assert np.array_equal(o2, eo) and np.array_equal(i2, ei)
    finally:
        bF.free()
        bA.free()


def _chunks(shards, rows_per_shard):
    """include/fbk.h's densify arithmetic: (shards per launch, rows per launch)"""
    per_shard = (1 << 17) * rows_per_shard
    if per_shard <= 1 << 28:
        most = max(1, min(shards, (1 << 28) // per_shard))
        passes = -(-shards // most)
        return -(-shards // passes), rows_per_shard
    return 1, (1 << 28) >> 17


def test_several_densify_chunks(gpu_ctx):
    """encoded operands past the 2^28-byte scratch: a set field of 4096 rows (blocks of 2048 rows, one shard per launch), a
    depth-64 int field over 40 shards (two chunks of 20), a filter over 2100 shards (two chunks of 1050).  Every shard uses the
    same few fragment rows (row lists may repeat rows), so the data stays small."""
    rng = D.rng_for(8600)
    # set field
    n_a = 4096
    assert _chunks(2, n_a) == (1, 2048)
    F = np.zeros((2, 16, 1024), dtype=np.uint64)
    F[:, 0, 5:7] = _rnd(rng, (2, 2))
    F[:, 11, 500] = _rnd(rng, (2,))
    A1 = np.zeros((1, n_a, 16, 1024), dtype=np.uint64)
    A1[0, :, 0, 5:7] = _rnd(rng, (n_a, 2), 3)
    A1[0, :, 11, 500] = _rnd(rng, (n_a,), 1)
    bF, bA = _upload(gpu_ctx, F, True), _upload(gpu_ctx, A1, True)
    try:
        with gpu_ctx.extract(bF, [0, 1], [3, 8]) as h:
            A = np.broadcast_to(A1, (2, n_a, 16, 1024))
            _check(gpu_ctx, h, F, [3, 8], 0, None, bA=bA, A=A, ra=np.tile(np.arange(n_a, dtype=np.uint32), (2, 1)))
    finally:
        bF.free()
        bA.free()
    # int field, depth 64
    n_sh, depth = 40, 64
    assert _chunks(n_sh, depth + 2) == (20, 66)
    F = np.zeros((n_sh, 16, 1024), dtype=np.uint64)
    F[:, 3, 100:102] = _rnd(rng, (n_sh, 2), 1)
    S1 = np.zeros((2, depth + 2, 16, 1024), dtype=np.uint64)
    S1[:, :, 3, 100:102] = _rnd(rng, (2, depth + 2, 2))
    S = S1[np.arange(n_sh) % 2]
    bF, bS = _upload(gpu_ctx, F, True), _upload(gpu_ctx, S1, True)
    try:
        with gpu_ctx.extract(bF, np.arange(n_sh), np.arange(n_sh) * 3) as h:
            _check(gpu_ctx, h, F, np.arange(n_sh) * 3, 0, None, bS, S, depth, base=(np.arange(n_sh, dtype=np.uint32) % 2) * (depth + 2))
    finally:
        bF.free()
        bS.free()
    # filter
    n_sh = 2100
    assert _chunks(n_sh, 1) == (1050, 1)
    F1 = np.zeros((3, 16, 1024), dtype=np.uint64)
    F1[1, 0, 0] = np.uint64(0b1011)
    F1[2, 13, 77] = np.uint64(1) << np.uint64(63)
    pick = np.zeros(n_sh, dtype=np.uint32)
    pick[[0, 1049, 1050, 2099]] = [1, 2, 1, 2]
    pick[1500:1510] = 1
    F = F1[pick]
    bF = _upload(gpu_ctx, F1, True)
    try:
        ids = np.arange(n_sh) + 10
        with gpu_ctx.extract(bF, pick, ids) as h:
            _check(gpu_ctx, h, F, ids, 0, None)
            assert h.span() == (0, n_sh)
        with gpu_ctx.extract(bF, pick, ids, offset=5, limit=31) as h:
            _check(gpu_ctx, h, F, ids, 5, 31)
            assert h.span() == (1050, 1509 - 1050 + 1)
    finally:
        bF.free()


def test_identities_with_existing_calls(gpu_ctx, small):
    F, S, A = small
    n_sh, n_a, depth = 3, 5, 20
    bF, bS, bA = _upload(gpu_ctx, F, False), _upload(gpu_ctx, S, False), _upload(gpu_ctx, A, True)
    rf, base = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint32) * (depth + 2)
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    try:
        with gpu_ctx.extract(bF, rf, [0, 1, 2]) as h:
            cols = h.columns()
            vals, pres = h.bsi(bS, base, depth)
            offs, items = h.rows(bA, ra)
        assert np.array_equal(np.unique(vals[pres]), gpu_ctx.bsi_distinct(bS, base, depth, bF, rf))
        sums, counts = gpu_ctx.bsi_sum(bS, base, depth, bF, rf)
        assert int(pres.sum()) == int(counts.sum()) and int(vals[pres].sum()) == int(sums.sum())
        per_row = gpu_ctx.intersection_count(bA, ra.reshape(-1), bF, np.repeat(rf, n_a)).reshape(n_sh, n_a).sum(axis=0)
        assert np.array_equal(np.bincount(items, minlength=n_a).astype(np.uint64), per_row)
        down = bF.download()
        exp = []
        for s in range(n_sh):
            for key in sorted(down[s]):
                w = down[s][key].words()
                exp.append((s << 20) + ((key & 15) << 16) + np.nonzero(np.unpackbits(w.view(np.uint8), bitorder="little"))[0])
        assert np.array_equal(cols, np.concatenate(exp).astype(np.uint64))
    finally:
        for b in (bF, bS, bA):
            b.free()


def test_handles_own_their_state(gpu_ctx, small):
    """two handles alive at once, used alternately, with a count matrix of the same context in between"""
    F, S, A = small
    ids = [0, 1, 4]
    bF, bS, bA = _upload(gpu_ctx, F, True), _upload(gpu_ctx, S, False), _upload(gpu_ctx, A, False)
    ra = np.arange(15, dtype=np.uint32).reshape(3, 5)
    h1 = gpu_ctx.extract(bF, np.arange(3), ids, offset=10, limit=70000)
    h2 = gpu_ctx.extract(bF, np.arange(3), ids, offset=200000)
    try:
        for _ in range(2):
            _check(gpu_ctx, h1, F, ids, 10, 70000, bS, S, 20)
            _check(gpu_ctx, h2, F, ids, 200000, None, bA=bA, A=A)
            gpu_ctx.count_matrix(bA, ra, bA, ra, bF, np.arange(3))
            _check(gpu_ctx, h2, F, ids, 200000, None, bS, S, 20)
            _check(gpu_ctx, h1, F, ids, 10, 70000, bA=bA, A=A)
        other = gpu_ctx.fork()
        try:
            out = np.zeros(h1.n, dtype=np.uint64)
            assert other.lib.fbk_extract_columns(other.h, h1.h, out.ctypes.data) == L.FBK_E_INVALID  # another context's handle
        finally:
            other.close()
    finally:
        h1.close()
        h2.close()
        for b in (bF, bS, bA):
            b.free()
