"""fbk_count_cube without a device: the ABI is declared and bound, bad arguments are errors (not crashes), the two ways the GPU
tests compute expected values — a numpy brute force over the words and the oracle's composition (intersect, intersect,
intersection_count) — agree on random small fragments, and the helper that restates the documented chunk arithmetic gives the
values worked out by hand."""
import numpy as np
import pytest

import cube_ref as R
import datagen as D
import msum_ref as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


def test_signature_declared(lib):
    assert "fbk_count_cube" in lib.SIGNATURES
    assert getattr(lib.load(), "fbk_count_cube") is not None
    assert len(lib.SIGNATURES["fbk_count_cube"][1]) == 14


def test_null_and_over_limit_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    rows = np.zeros(4, dtype=np.uint32)
    out = np.zeros(64, dtype=np.uint64)
    r, o = rows.ctypes.data, out.ctypes.data
    assert l.fbk_count_cube(None, None, None, 0, None, None, 0, None, None, 0, None, None, 0, None) == lib.FBK_E_INVALID
    assert l.fbk_count_cube(None, None, r, 1, None, r, 1, None, r, 1, None, None, 1, o) == lib.FBK_E_INVALID
    assert b"NULL" in l.fbk_last_error(None)
    # the limits are checked first: more than 4096 rows in a field, more than 2^24 groups (97 * 257 * 673 = 2^24 + 1)
    for n_p, n_a, n_b in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097), (97, 257, 673), (4096, 4096, 2)):
        assert l.fbk_count_cube(None, None, r, n_p, None, r, n_a, None, r, n_b, None, None, 1, o) == lib.FBK_E_INVALID
        assert b"block the leading field" in l.fbk_last_error(None), (n_p, n_a, n_b)
    assert 97 * 257 * 673 == (1 << 24) + 1


def _random_case(rng, n_sh, n_p, n_a, n_b, slots=(0, 9)):
    def rnd(*shape):
        w = np.zeros(shape + (16, 1024), dtype=np.uint64)
        for sl in slots:
            w[..., sl, :] = rng.integers(0, 1 << 63, shape + (1024,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (1024,), dtype=np.uint64)
        return w

    return rnd(n_sh, n_p), rnd(n_sh, n_a), rnd(n_sh, n_b), rnd(n_sh)


@pytest.mark.parametrize("with_filter", [False, True])
def test_oracle_composition_equals_numpy_brute_force(oracle, with_filter):
    O = oracle
    rng = D.rng_for(7800, int(with_filter))
    n_sh, n_p, n_a, n_b = 2, 2, 3, 4
    P, A, B, F = _random_case(rng, n_sh, n_p, n_a, n_b)
    P[1, 0] = 0  # a row that does not exist in a shard
    A[0, 1, 9] = 0  # an empty container
    cube = R.numpy_expected(P, A, B, F if with_filter else None)
    bms = lambda W: [[M.bitmap_of_words(O, W[s, i]) for i in range(W.shape[1])] for s in range(n_sh)]
    f_bms = [M.bitmap_of_words(O, F[s]) for s in range(n_sh)] if with_filter else None
    triples = [(p, i, j) for p in range(n_p) for i in range(n_a) for j in range(n_b)]
    exp = R.oracle_expected(bms(P), bms(A), bms(B), f_bms, triples)
    for t, n in exp.items():
        assert int(cube[t]) == n, t
    assert cube.sum() > 0 and int(cube[0, 0, 0]) > int(cube[0, 1, 0]) > 0  # (A row 1 lost a container in shard 0)


def test_numpy_brute_force_by_hand():
    """one shard; columns 3 and 70 in all three rows, column 5 in P and A only; the filter keeps column 70"""
    W = np.zeros((1, 1, 16, 1024), dtype=np.uint64)
    W[0, 0, 0, 0] = (1 << 3) | (1 << 5)
    W[0, 0, 0, 1] = 1 << 6
    Bw = W.copy()
    Bw[0, 0, 0, 0] = 1 << 3
    assert R.numpy_expected(W, W, Bw, None).tolist() == [[[2]]]
    F = np.zeros((1, 16, 1024), dtype=np.uint64)
    F[0, 0, 1] = ~np.uint64(0)
    assert R.numpy_expected(W, W, Bw, F).tolist() == [[[1]]]


def test_chunk_arithmetic_by_hand():
    # dense operands: 8 bytes per cell and shard; 2^30 / (8 * 8 * 32 * 32) = 16384 shards at a time
    assert R.chunk(1024, 8, 32, 32, True, True, True) == 1024
    assert R.chunk(20000, 8, 32, 32, True, True, True) == 10000  # two chunks, dealt evenly
    # the largest cube: 128 MiB a shard, 8 shards a chunk
    assert R.chunk(20, 4096, 4096, 1, True, True, True) == 7  # most = 8 -> 3 chunks -> 7, 7, 6
    # every operand encoded: (16 + 32 + 32 + 1) rows of 128 KiB + 128 KiB of cells -> at most 99 shards
    assert (1 << 30) // (81 * (1 << 17) + 8 * 16 * 32 * 32) == 99
    assert R.chunk(100, 16, 32, 32, False, False, False, False) == 50
    assert R.chunk(99, 16, 32, 32, False, False, False, False) == 99
    # P encoded only
    assert R.chunk(3000, 3, 5, 7, False, True, True) == 1500  # 2^30 / (3 * 2^17 + 840) = 2724
