"""GPU parity of fbk_count_cube (GroupBy over three fields in one pass): bit-exact against the numpy brute force over the words
for every cell and against the oracle's composition (intersect, intersect, intersection_count) for sampled triples
(tests/cube_ref.py; the CPU test shows the two agree).  Dense batches over shard counts and cube shapes around the kernel's tile
(32 x 32 rows of A and B, PT rows of P); every slots-per-block value; the reference's own vector; encoded batches (the densify
path) and mixes; the existing two-call path on the device; a call that densifies in more than one chunk; limits and recovery;
a batch uploaded with wrong cardinalities."""
import numpy as np
import pytest

import cube_ref as R
import datagen as D
import msum_ref as M
from featurebase_amd import lib as L
from featurebase_amd.roaring import Container

pytestmark = pytest.mark.gpu

PT = R.PT
SHAPES = [(1, 1, 1), (2, 5, 7), (PT, 32, 32), (PT + 1, 33, 2), (3, 2, 65), (2 * PT + 1, 1, 33), (4, 2, 3), (5, 3, 2)]
SMALL = 2 * 5 * 7  # cells up to which the words fill all 16 slots; above, slots 0, 9 and 15 (the brute force stays cheap)


def _rnd(rng, shape, slots):
    w = np.zeros(shape + (16, 1024), dtype=np.uint64)
    for sl in slots:
        w[..., sl, :] = rng.integers(0, 1 << 63, shape + (1024,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (1024,), dtype=np.uint64)
    return w


def _dense_case(rng, n_sh, n_p, n_a, n_b):
    slots = tuple(range(16)) if n_p * n_a * n_b <= SMALL else (0, 9, 15)
    P, A, B, F = _rnd(rng, (n_sh, n_p), slots), _rnd(rng, (n_sh, n_a), slots), _rnd(rng, (n_sh, n_b), slots), _rnd(rng, (n_sh,), slots)
    A[0, 0, 9] = 0  # an empty container in a row
    if n_p > 1:
        P[n_sh - 1, n_p - 1] = 0  # an empty P row
    if n_sh > 1:
        F[1] = 0  # a shard whose filter row is empty
    return P, A, B, F


def _upload_dense(ctx, *words):
    """one dense batch per operand; row lists [n_shards, n] (the filter's: [n_shards])"""
    out = []
    for W in words:
        n_sh = W.shape[0]
        out.append((ctx.upload_dense(W.reshape(-1)), np.arange(W.size // (16 * 1024), dtype=np.uint32).reshape(n_sh, -1) if W.ndim == 4 else np.arange(n_sh, dtype=np.uint32)))
    return out


def _check(O, rng, got, P, A, B, F, bms=None, k=4):
    exp = R.numpy_expected(P, A, B, F)
    assert got.shape == exp.shape and got.dtype == np.uint64
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:5]
    n_sh = P.shape[0]
    triples = R.sample_triples(rng, *exp.shape, k=k)
    if bms is None:
        of = lambda W, idx: [{i: M.bitmap_of_words(O, W[s, i]) for i in idx} for s in range(n_sh)]
        bms = (of(P, {t[0] for t in triples}), of(A, {t[1] for t in triples}), of(B, {t[2] for t in triples}),
               [M.bitmap_of_words(O, F[s]) for s in range(n_sh)] if F is not None else None)
    for t, n in R.oracle_expected(*bms, triples).items():
        assert int(got[t]) == n, t


@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("n_sh", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_dense_batches(gpu_ctx, oracle, shape, n_sh, with_filter):
    rng = D.rng_for(7900, n_sh, *shape, int(with_filter))
    P, A, B, F = _dense_case(rng, n_sh, *shape)
    (bP, rp), (bA, ra), (bB, rb), (bF, rf) = ups = _upload_dense(gpu_ctx, P, A, B, F)
    try:
        got = gpu_ctx.count_cube(bP, rp, bA, ra, bB, rb, bF if with_filter else None, rf if with_filter else None)
        _check(oracle, rng, got, P, A, B, F if with_filter else None)
        assert got.any()
    finally:
        for b, _ in ups:
            b.free()


def test_every_slots_per_block_value_gives_the_same_cube(gpu_ctx, oracle):
    rng = D.rng_for(7910)
    P, A, B, F = _dense_case(rng, 3, PT + 1, 33, 33)
    (bP, rp), (bA, ra), (bB, rb), (bF, rf) = ups = _upload_dense(gpu_ctx, P, A, B, F)
    try:
        cubes = []
        for spb in (1, 2, 4, 8, 16):
            gpu_ctx.set_option("matrix_spb", spb)
            cubes.append(gpu_ctx.count_cube(bP, rp, bA, ra, bB, rb, bF, rf))
        gpu_ctx.set_option("matrix_spb", 0)
        for c in cubes[1:]:
            assert np.array_equal(c, cubes[0])
        _check(oracle, rng, cubes[0], P, A, B, F)
    finally:
        gpu_ctx.set_option("matrix_spb", 0)
        for b, _ in ups:
            b.free()


def test_the_reference_s_own_vector(gpu_ctx):
    """executor_test.go:6337-6383: rows 0..3 of one field over four shards, column 0 in every row, columns 91000, 2^20, 2 * 2^20
    and 3 * 2^20 in row 3 only; GroupBy over the field three times: every group counts 1, (3, 3, 3) counts 5"""
    n_sh, n = 4, 4
    rows = []
    for s in range(n_sh):
        for r in range(n):
            cols = ([0] if s == 0 else []) + ([91000] if s == 0 and r == 3 else []) + ([0] if s > 0 and r == 3 else [])
            by_slot = {}
            for c in sorted(set(cols)):
                by_slot.setdefault(c >> 16, []).append(c & 0xFFFF)
            rows.append({sl: Container.array(np.array(v, dtype=np.uint16)) for sl, v in by_slot.items()})
    b = gpu_ctx.upload(rows)
    rl = np.arange(n_sh * n, dtype=np.uint32).reshape(n_sh, n)
    try:
        got = gpu_ctx.count_cube(b, rl, b, rl, b, rl)
        exp = np.ones((n, n, n), dtype=np.uint64)
        exp[3, 3, 3] = 5
        assert np.array_equal(got, exp)
    finally:
        b.free()


def _encoded_rows(rng, n_sh, n):
    """datagen's mixed containers with nil slots, some rows missing in some shards"""
    out = [[D.random_row(rng, 0, p_missing=0.3) for _ in range(n)] for _ in range(n_sh)]
    for s in range(n_sh):
        if rng.random() < 0.5:
            out[s][int(rng.integers(0, n))] = {}
    return out


def _obm(O, r):
    return O.OBitmap.from_containers([(k & 15, c) for k, c in r.items()]) if r else None


@pytest.mark.parametrize("mix", ["p_encoded", "all_encoded", "filter_encoded", "one_batch"])
def test_encoded_batches(gpu_ctx, oracle, mix):
    O = oracle
    rng = D.rng_for(7920, ["p_encoded", "all_encoded", "filter_encoded", "one_batch"].index(mix))
    n_sh, n_p, n_a, n_b = 3, 3, 5, 6
    p_rows, a_rows, b_rows = _encoded_rows(rng, n_sh, n_p), _encoded_rows(rng, n_sh, n_a), _encoded_rows(rng, n_sh, n_b)
    f_rows = [D.random_row(rng, 0, p_missing=0.2) for _ in range(n_sh)]
    words = lambda rows: np.stack([np.stack([M.words_of_row(r) for r in sh]) for sh in rows])
    P, A, B, F = words(p_rows), words(a_rows), words(b_rows), np.stack([M.words_of_row(r) for r in f_rows])
    bms = ([[_obm(O, r) for r in sh] for sh in p_rows], [[_obm(O, r) for r in sh] for sh in a_rows], [[_obm(O, r) for r in sh] for sh in b_rows],
           [_obm(O, r) for r in f_rows])
    flat = lambda rows: [D.to_fbk_row(r) for sh in rows for r in sh]
    lists = lambda n, at=0: at + np.arange(n_sh * n, dtype=np.uint32).reshape(n_sh, n)
    enc = {"p_encoded": (True, False, False, False), "all_encoded": (True, True, True, True), "filter_encoded": (False, False, False, True),
           "one_batch": (True, True, True, True)}[mix]
    if mix == "one_batch":  # the three fields' rows in ONE batch, different row lists
        bP = bA = bB = gpu_ctx.upload(flat(p_rows) + flat(a_rows) + flat(b_rows))
        rp, ra, rb = lists(n_p), lists(n_a, n_sh * n_p), lists(n_b, n_sh * (n_p + n_a))
    else:
        up = lambda rows, W, e: gpu_ctx.upload(flat(rows)) if e else gpu_ctx.upload_dense(W.reshape(-1))
        bP, bA, bB = up(p_rows, P, enc[0]), up(a_rows, A, enc[1]), up(b_rows, B, enc[2])
        rp, ra, rb = lists(n_p), lists(n_a), lists(n_b)
    bF = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows]) if enc[3] else gpu_ctx.upload_dense(F.reshape(-1))
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        for with_filter in (False, True):
            got = gpu_ctx.count_cube(bP, rp, bA, ra, bB, rb, bF if with_filter else None, rf if with_filter else None)
            _check(O, rng, got, P, A, B, F if with_filter else None, bms[:3] + (bms[3] if with_filter else None,), k=6)
            assert got.any()
    finally:
        for b in {id(x): x for x in (bP, bA, bB, bF)}.values():
            b.free()


def test_the_two_call_path_on_the_device_gives_the_same_planes(gpu_ctx):
    """for sampled p: fbk_setop(AND, P_p, F) then fbk_count_matrix(A, B, filter = that) == cube[p]"""
    rng = D.rng_for(7930)
    n_sh, n_p, n_a, n_b = 3, PT + 2, 9, 34
    P, A, B, F = _dense_case(rng, n_sh, n_p, n_a, n_b)
    (bP, rp), (bA, ra), (bB, rb), (bF, rf) = ups = _upload_dense(gpu_ctx, P, A, B, F)
    try:
        cube = gpu_ctx.count_cube(bP, rp, bA, ra, bB, rb, bF, rf)
        for p in (0, PT - 1, PT, n_p - 1):
            pf, _ = gpu_ctx.setop(L.OP_AND, bP, rp[:, p], bF, rf)
            try:
                plane = gpu_ctx.count_matrix(bA, ra, bB, rb, pf, np.arange(n_sh, dtype=np.uint32))
            finally:
                pf.free()
            assert np.array_equal(np.asarray(plane), cube[p]), p
        assert cube.any()
    finally:
        for b, _ in ups:
            b.free()


def test_densify_in_several_chunks(gpu_ctx):
    """every operand encoded, 16 x 32 x 32 groups: at most 99 shards per chunk, so 100 shards take two chunks of 50.  Sparse
    rows: a few columns per shard, every row a subset of them, the expectation a product of the membership matrices."""
    rng = D.rng_for(7940)
    n_sh, n_p, n_a, n_b, n_cols = 100, 16, 32, 32, 24
    assert R.chunk(n_sh, n_p, n_a, n_b, False, False, False, False) == 50
    exp = np.zeros((n_p, n_a, n_b), dtype=np.int64)
    rows = {"p": [], "a": [], "b": [], "f": []}
    for s in range(n_sh):
        cols = np.sort(rng.choice(1 << 20, size=n_cols, replace=False))
        member = {k: rng.random((n, n_cols)) < d for k, n, d in (("p", n_p, 0.5), ("a", n_a, 0.4), ("b", n_b, 0.4), ("f", 1, 0.8))}
        if s % 7 == 3:
            member["a"][5] = False  # the row does not exist in this shard
        exp += np.einsum("pc,ic,jc->pij", (member["p"] & member["f"][0]).astype(np.int64), member["a"].astype(np.int64), member["b"].astype(np.int64))
        for k, m in member.items():
            for r in range(m.shape[0]):
                by_slot = {}
                for c in cols[m[r]].tolist():
                    by_slot.setdefault(c >> 16, []).append(c & 0xFFFF)
                rows[k].append({sl: Container.array(np.array(v, dtype=np.uint16)) for sl, v in by_slot.items()})
    bP, bA, bB, bF = (gpu_ctx.upload(rows[k]) for k in "pabf")
    lists = lambda n: np.arange(n_sh * n, dtype=np.uint32).reshape(n_sh, n)
    try:
        got = gpu_ctx.count_cube(bP, lists(n_p), bA, lists(n_a), bB, lists(n_b), bF, np.arange(n_sh, dtype=np.uint32))
        assert np.array_equal(got, exp.astype(np.uint64))
        assert exp[0, 0, 0] > 0 and exp[n_p - 1, n_a - 1, n_b - 1] > 0
    finally:
        for b in (bP, bA, bB, bF):
            b.free()


def test_limits_and_recovery(gpu_ctx, oracle):
    rng = D.rng_for(7950)
    n_sh, n_p, n_a, n_b = 2, 3, 4, 5
    P, A, B, F = _dense_case(rng, n_sh, n_p, n_a, n_b)
    (bP, rp), (bA, ra), (bB, rb), (bF, rf) = ups = _upload_dense(gpu_ctx, P, A, B, F)
    try:
        z = lambda n: np.zeros((1, n), dtype=np.uint32)
        with pytest.raises(L.FbkError) as e:  # 97 * 257 * 673 = 2^24 + 1 groups
            gpu_ctx.count_cube(bP, z(97), bA, z(257), bB, z(673))
        assert e.value.code == L.FBK_E_INVALID and "block the leading field" in str(e.value)
        with pytest.raises(L.FbkError) as e:
            gpu_ctx.count_cube(bP, z(4097), bA, z(1), bB, z(1))
        assert e.value.code == L.FBK_E_INVALID
        for which in range(4):  # a row index beyond the batch, in every list
            lists = [rp.copy(), ra.copy(), rb.copy(), rf.copy()]
            lists[which].reshape(-1)[-1] = [n_sh * n_p, n_sh * n_a, n_sh * n_b, n_sh][which]
            with pytest.raises(L.FbkError) as e:
                gpu_ctx.count_cube(bP, lists[0], bA, lists[1], bB, lists[2], bF, lists[3])
            assert e.value.code == L.FBK_E_INVALID and "out of range" in str(e.value), which
        got = gpu_ctx.count_cube(bP, rp, bA, ra, bB, rb, bF, rf)
        _check(oracle, rng, got, P, A, B, F)
        # no shards: a complete all-zero cube; no rows in a field: nothing to write
        e0 = lambda n: np.zeros((0, n), dtype=np.uint32)
        assert not gpu_ctx.count_cube(bP, e0(n_p), bA, e0(n_a), bB, e0(n_b)).any()
        assert gpu_ctx.count_cube(bP, rp, bA, np.zeros((n_sh, 0), dtype=np.uint32), bB, rb).shape == (n_p, 0, n_b)
    finally:
        for b, _ in ups:
            b.free()


def test_a_wrong_stored_cardinality_changes_nothing(gpu_ctx):
    """bitmap and run containers uploaded with a wrong n: the cube comes from the words"""
    rng = D.rng_for(7960)
    n_sh, n_p, n_a, n_b = 2, 2, 3, 3
    slots = (0, 9)
    P, A, B = _rnd(rng, (n_sh, n_p), slots), _rnd(rng, (n_sh, n_a), slots), _rnd(rng, (n_sh, n_b), slots)
    run = [(100, 4000), (5000, 5000), (60000, 65535)]
    run_words = D.words_of(np.concatenate([np.arange(a, b + 1) for a, b in run]))
    A[:, :, 3] = run_words  # slot 3 of every A row: a run container
    P[:, :, 3] = ~np.uint64(0)
    B[:, :, 3] = _rnd(rng, (n_sh, n_b), (0,))[:, :, 0]

    def rows(W, wrong):
        out = []
        for s in range(n_sh):
            for r in range(W.shape[1]):
                row = {}
                for sl in (0, 3, 9):
                    true_n = int(np.bitwise_count(W[s, r, sl]).sum())
                    n = [7, 65536, true_n // 2][(s + r + sl) % 3] if wrong else true_n
                    row[sl] = Container.run(run, n) if W is A and sl == 3 else Container.bitmap(W[s, r, sl], n=n)
                out.append(row)
        return out

    lists = lambda n: np.arange(n_sh * n, dtype=np.uint32).reshape(n_sh, n)
    exp = R.numpy_expected(P, A, B, None)
    for wrong in (False, True):
        bP, bA, bB = gpu_ctx.upload(rows(P, wrong)), gpu_ctx.upload(rows(A, wrong)), gpu_ctx.upload(rows(B, wrong))
        try:
            got = gpu_ctx.count_cube(bP, lists(n_p), bA, lists(n_a), bB, lists(n_b))
            assert np.array_equal(got, exp), wrong
        finally:
            for b in (bP, bA, bB):
                b.free()
