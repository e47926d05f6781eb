"""GPU parity of fbk_count_matrix_sum (GroupBy with aggregate=Sum): bit-exact against the numpy brute force for every pair and
against the oracle's composition (intersect, then BSI Sum over that filter) for sampled pairs (tests/msum_ref.py; the CPU test
shows the two agree).  Dense batches over shard counts, matrix shapes and depths 0..64; encoded batches (the densify path);
the one-field form; the prepared query; a call that densifies in more than one chunk; recovery after an error."""
import numpy as np
import pytest

import datagen as D
import msum_ref as R
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu

DEPTHS = [0, 1, 7, 8, 20, 63, 64]
SHAPES = [(1, 1), (5, 7), (32, 32), (33, 65), (64, 1)]


@pytest.fixture(scope="module")
def B(oracle):
    from oracle import pybsi

    pybsi._lib()
    return pybsi


def _rnd(rng, shape, ands=0):
    w = rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    for _ in range(ands):
        w &= rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    return w


def _dense_case(rng, n_sh, n_a, n_b, depth, exists_ands):
    A = _rnd(rng, (n_sh, n_a, 16, 1024))
    Bw = _rnd(rng, (n_sh, n_b, 16, 1024))
    F = _rnd(rng, (n_sh, 16, 1024))
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    S[:, 0] &= _rnd(rng, (n_sh, 16, 1024), exists_ands)
    if n_sh > 2:
        S[1, 0] = 0  # a shard without values
    A[0, 0, 3] = 0  # an empty container in a row
    return A, Bw, F, S


def _sample_pairs(rng, n_a, n_b, k=4):
    pairs = {(0, 0), (n_a - 1, n_b - 1)}
    while len(pairs) < min(k, n_a * n_b):
        pairs.add((int(rng.integers(0, n_a)), int(rng.integers(0, n_b))))
    return sorted(pairs)


def _check(O, B, rng, got, A, Bw, F, S, depth, a_bms=None, b_bms=None, f_bms=None, frags=None, k=4):
    sums, counts = got
    es, ec = R.numpy_expected(A, Bw, F, S, depth)
    assert np.array_equal(counts, ec), "counts"
    assert np.array_equal(sums, es), "sums"
    n_sh, n_a = A.shape[:2]
    n_b = Bw.shape[1] if Bw is not None else 1
    pairs = _sample_pairs(rng, n_a, n_b, k)
    if a_bms is None:
        a_bms = [{i: R.bitmap_of_words(O, A[s, i]) for i, _ in pairs} for s in range(n_sh)]
        b_bms = [{j: R.bitmap_of_words(O, Bw[s, j]) for _, j in pairs} for s in range(n_sh)] if Bw is not None else None
        f_bms = [R.bitmap_of_words(O, F[s]) for s in range(n_sh)] if F is not None else None
        frags = [R.fragment_of_words(O, B, S[s]) for s in range(n_sh)]
    for (i, j), (sm, c) in R.oracle_expected(O, B, a_bms, b_bms, f_bms, frags, pairs).items():
        assert (int(sums[i, j]), int(counts[i, j])) == (sm, c), (i, j)


def _upload_dense(ctx, A, Bw, F, S):
    n_sh, n_a = A.shape[:2]
    rps = S.shape[1]
    bA, bS, bF = ctx.upload_dense(A.reshape(-1)), ctx.upload_dense(S.reshape(-1)), ctx.upload_dense(F.reshape(-1))
    bB = ctx.upload_dense(Bw.reshape(-1)) if Bw is not None else None
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * Bw.shape[1], dtype=np.uint32).reshape(n_sh, -1) if Bw is not None else None
    return bA, ra, bB, rb, bF, np.arange(n_sh, dtype=np.uint32), bS, np.arange(n_sh, dtype=np.uint32) * rps


DENSE_CASES = [(n_sh, na, nb, DEPTHS[k % 7], k % 2 == 1) for k, (n_sh, (na, nb)) in enumerate((s, sh) for sh in SHAPES for s in (1, 3, 17))]
DENSE_CASES += [(3, 5, 7, d, f) for d in DEPTHS for f in (False, True)]


@pytest.mark.parametrize("n_sh,n_a,n_b,depth,with_filter", DENSE_CASES)
def test_dense_batches(gpu_ctx, oracle, B, n_sh, n_a, n_b, depth, with_filter):
    rng = D.rng_for(7200, n_sh, n_a, n_b, depth, int(with_filter))
    A, Bw, F, S = _dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=1 if n_a * n_b <= 64 else 6)
    bA, ra, bB, rb, bF, rf, bS, base = _upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        got = gpu_ctx.count_matrix_sum(bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
        _check(oracle, B, rng, got, A, Bw, F if with_filter else None, S, depth)
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def _encoded_case(oracle, B, rng, n_sh, n_a, n_b, depth, n_vals=3000):
    """mixed containers (datagen's archetypes, nil slots), some rows missing in some shards (an empty row), BSI fragments
    built with optimize() (planes as arrays and runs); returns the fbk rows and the words / oracle bitmaps of every row"""
    O = oracle

    def rows(n):
        out = [[D.random_row(rng, 0, p_missing=0.3) for _ in range(n)] for _ in range(n_sh)]
        for s in range(n_sh):
            if rng.random() < 0.5:
                out[s][int(rng.integers(0, n))] = {}  # the row does not exist in this shard
        return out

    a_rows, b_rows = rows(n_a), rows(n_b)
    f_rows = [D.random_row(rng, 0, p_missing=0.2) for _ in range(n_sh)]
    frags, S = [], np.zeros((n_sh, depth + 2, 16, 1024), dtype=np.uint64)
    lim = (1 << depth) - 1
    for s in range(n_sh):
        cols = rng.choice(1 << 20, size=n_vals, replace=False)
        cols[: n_vals // 3] = (cols[: n_vals // 3] & 0xFFFF) | (5 << 16)  # a third of them in one container (runs / bitmaps)
        vals = {}
        for c in np.unique(cols).tolist():
            m = int(rng.integers(0, lim, endpoint=True, dtype=np.uint64))
            vals[c] = -m if rng.random() < 0.4 else m
        fr = B.bsi_fragment_from_values(vals, depth)
        frags.append(fr)
        for r in range(depth + 2):
            S[s, r] = R.words_of_bitmap(fr.rows[r])
    A = np.stack([np.stack([R.words_of_row(r) for r in sh]) for sh in a_rows])
    Bw = np.stack([np.stack([R.words_of_row(r) for r in sh]) for sh in b_rows])
    F = np.stack([R.words_of_row(r) for r in f_rows])
    ob = lambda r: O.OBitmap.from_containers([(k & 15, c) for k, c in r.items()]) if r else None
    bms = ([[ob(r) for r in sh] for sh in a_rows], [[ob(r) for r in sh] for sh in b_rows], [ob(r) for r in f_rows])
    return a_rows, b_rows, f_rows, frags, A, Bw, F, S, bms


def _upload_bsi(ctx, frags):
    rows, base = [], []
    for fr in frags:
        base.append(len(rows))
        for r, bm in enumerate(fr.rows):
            rows.append({r * 16 + k: D.to_fbk(c) for k, c in bm.items() if c.n} if bm is not None else {})
    return ctx.upload(rows), np.array(base, dtype=np.uint32)


@pytest.mark.parametrize("depth", [0, 7, 20, 64])
@pytest.mark.parametrize("same_batch", [False, True])
def test_encoded_batches(gpu_ctx, oracle, B, depth, same_batch):
    rng = D.rng_for(7300, depth, int(same_batch))
    n_sh, n_a, n_b = 5, 6, 9
    a_rows, b_rows, f_rows, frags, A, Bw, F, S, (abm, bbm, fbm) = _encoded_case(oracle, B, rng, n_sh, n_a, n_b, depth)
    flat = lambda rows: [D.to_fbk_row(r) for sh in rows for r in sh]
    if same_batch:  # A and B rows in ONE batch, different row lists
        bA = gpu_ctx.upload(flat(a_rows) + flat(b_rows))
        bB = bA
        ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
        rb = n_sh * n_a + np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    else:
        bA, bB = gpu_ctx.upload(flat(a_rows)), gpu_ctx.upload(flat(b_rows))
        ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
        rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    bF = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    bS, base = _upload_bsi(gpu_ctx, frags)
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        for with_filter in (False, True):
            got = gpu_ctx.count_matrix_sum(bA, ra, bB, rb, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
            _check(oracle, B, rng, got, A, Bw, F if with_filter else None, S, depth, abm, bbm, fbm if with_filter else None, frags, k=6)
        # the one-field form over encoded rows
        got = gpu_ctx.count_matrix_sum(bA, ra, None, None, bS, base, depth, bF, rf)
        _check(oracle, B, rng, got, A, None, F, S, depth, abm, None, fbm, frags, k=6)
    finally:
        for b in {id(x): x for x in (bA, bB, bF, bS)}.values():
            b.free()


@pytest.mark.parametrize("depth", [0, 20, 64])
def test_one_field_dense(gpu_ctx, oracle, B, depth):
    rng = D.rng_for(7400, depth)
    n_sh, n_a = 3, 40
    A, _, F, S = _dense_case(rng, n_sh, n_a, 1, depth, exists_ands=3)
    bA, ra, _, _, bF, rf, bS, base = _upload_dense(gpu_ctx, A, None, F, S)
    try:
        for with_filter in (False, True):
            got = gpu_ctx.count_matrix_sum(bA, ra, None, None, bS, base, depth, bF if with_filter else None, rf if with_filter else None)
            _check(oracle, B, rng, got, A, None, F if with_filter else None, S, depth)
        with pytest.raises(L.FbkError):  # without B rows n_b must be 1
            L.check(gpu_ctx.lib.fbk_count_matrix_sum(gpu_ctx.h, bA.h, ra.ctypes.data, n_a, None, None, 2, None, None, bS.h,
                                                                      base.ctypes.data, depth, n_sh, np.zeros(2 * n_a, np.int64).ctypes.data,
                                                                      np.zeros(2 * n_a, np.uint64).ctypes.data))
    finally:
        for b in (bA, bF, bS):
            b.free()


def test_prepared_query(gpu_ctx, oracle, B):
    rng = D.rng_for(7500)
    n_sh, n_a, n_b, depth = 4, 12, 20, 20
    A, Bw, F, S = _dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=2)
    bA, ra, bB, rb, bF, rf, bS, base = _upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        one = gpu_ctx.count_matrix_sum(bA, ra, bB, rb, bS, base, depth, bF, rf)
        _check(oracle, B, rng, one, A, Bw, F, S, depth)
        q = gpu_ctx.query_count_matrix_sum(bA, ra, bB, rb, bS, base, depth, bF, rf)
        other = gpu_ctx.prepare_count_matrix(bA, ra, bB, rb)
        try:
            for _ in range(2):
                q.run()
                s, c = q.read()
                assert np.array_equal(s, one[0]) and np.array_equal(c, one[1])
            other.run()  # another query in between
            q.run()
            s, c = q.read()
            assert np.array_equal(s, one[0]) and np.array_equal(c, one[1])
            p, nbytes = q.result_ptr()
            assert p and nbytes == n_a * n_b * 16
            with pytest.raises(L.FbkError):
                q.run(device_ptr=p)
            with pytest.raises(L.FbkError):
                q.run(accumulate=True)
            s, c = q.read()  # the rejected runs changed nothing
            assert np.array_equal(s, one[0]) and np.array_equal(c, one[1])
        finally:
            q.free()
            other.free()
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def _chunk(n_shards, n_a, n_b, depth, a_dense, b_dense, f_dense, bsi_dense):
    """the densify chunk of a call (include/fbk.h, fbk_count_matrix_sum)"""
    per = -(-depth // 7) * (1 << 20) + 16 * n_a * n_b
    per += (1 << 17) * ((0 if a_dense else n_a) + (0 if b_dense else n_b) + (0 if f_dense else 1) + (0 if bsi_dense else depth + 2))
    most = max(1, min(n_shards, (1 << 30) // per))
    passes = -(-n_shards // most)
    return -(-n_shards // passes)


def test_densify_in_several_chunks(gpu_ctx, oracle, B):
    """encoded A, B, filter and BSI at depth 64: at most 54 shards per chunk, so 60 shards take two chunks of 30"""
    rng = D.rng_for(7600)
    n_sh, n_a, n_b, depth = 60, 1, 1, 64
    assert _chunk(n_sh, n_a, n_b, depth, False, False, False, False) == 30
    a_rows, b_rows, f_rows, frags, A, Bw, F, S, (abm, bbm, fbm) = _encoded_case(oracle, B, rng, n_sh, n_a, n_b, depth, n_vals=400)
    bA = gpu_ctx.upload([D.to_fbk_row(r) for sh in a_rows for r in sh])
    bB = gpu_ctx.upload([D.to_fbk_row(r) for sh in b_rows for r in sh])
    bF = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    bS, base = _upload_bsi(gpu_ctx, frags)
    ra = np.arange(n_sh, dtype=np.uint32).reshape(n_sh, 1)
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        got = gpu_ctx.count_matrix_sum(bA, ra, bB, ra, bS, base, depth, bF, rf)
        _check(oracle, B, rng, got, A, Bw, F, S, depth, abm, bbm, fbm, frags, k=1)
        assert got[1][0, 0] > 0
    finally:
        for b in (bA, bB, bF, bS):
            b.free()


def test_error_leaves_the_context_usable(gpu_ctx, oracle, B):
    rng = D.rng_for(7700)
    n_sh, n_a, n_b, depth = 2, 4, 3, 8
    A, Bw, F, S = _dense_case(rng, n_sh, n_a, n_b, depth, exists_ands=1)
    bA, ra, bB, rb, bF, rf, bS, base = _upload_dense(gpu_ctx, A, Bw, F, S)
    try:
        bad = base.copy()
        bad[1] = n_sh * (depth + 2) - 1  # the fragment's rows run past the batch
        with pytest.raises(L.FbkError) as e:
            gpu_ctx.count_matrix_sum(bA, ra, bB, rb, bS, bad, depth)
        assert e.value.code == L.FBK_E_INVALID
        with pytest.raises(L.FbkError):
            gpu_ctx.query_count_matrix_sum(bA, ra, bB, rb, bS, bad, depth)
        for call in (gpu_ctx.count_matrix_sum, gpu_ctx.query_count_matrix_sum):  # a depth past 64 bits
            with pytest.raises(L.FbkError) as e:
                call(bA, ra, bB, rb, bS, base, 65)
            assert e.value.code == L.FBK_E_INVALID and "bit depth" in str(e.value)
        got = gpu_ctx.count_matrix_sum(bA, ra, bB, rb, bS, base, depth, bF, rf)
        _check(oracle, B, rng, got, A, Bw, F, S, depth)
    finally:
        for b in (bA, bB, bF, bS):
            b.free()
