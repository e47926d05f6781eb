"""fbk_count_matrix_sum without a device: the ABI is declared and bound, bad arguments are errors (not crashes), and the two ways
the GPU tests compute expected values — the oracle's composition (intersect, then BSI Sum over that filter) and a numpy brute
force in uint64 wrap-around — agree on random small fragments: negative values, depth-64 magnitudes near 2^64, sign and plane
bits outside exists."""
import numpy as np
import pytest

import datagen as D
import msum_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


@pytest.fixture(scope="module")
def B(oracle):
    from oracle import pybsi

    pybsi._lib()
    return pybsi


def test_signatures_declared(lib):
    for name in ("fbk_count_matrix_sum", "fbk_query_count_matrix_sum"):
        assert name in lib.SIGNATURES
        assert getattr(lib.load(), name) is not None
    assert len(lib.SIGNATURES["fbk_count_matrix_sum"][1]) == 15
    assert len(lib.SIGNATURES["fbk_query_count_matrix_sum"][1]) == 14


def test_null_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    s, c = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.uint64)
    rows = np.zeros(4, dtype=np.uint32)
    assert l.fbk_count_matrix_sum(None, None, None, 0, None, None, 1, None, None, None, None, 0, 0, None, None) == lib.FBK_E_INVALID
    assert l.fbk_count_matrix_sum(None, None, rows.ctypes.data, 1, None, None, 1, None, None, None, rows.ctypes.data, 20, 1, s.ctypes.data,
                                  c.ctypes.data) == lib.FBK_E_INVALID
    assert l.fbk_query_count_matrix_sum(None, None, None, 0, None, None, 1, None, None, None, None, 0, 0, None) == lib.FBK_E_INVALID
    assert l.fbk_last_error(None) is not None


def _random_case(rng, n_sh, n_a, n_b, depth, slots=(0, 9)):
    """words with bits in two slots: A / B / F about half the columns, exists a quarter, sign and planes everywhere (also
    outside exists); at depth 64 most columns carry magnitudes near 2^64"""
    def rnd(*shape):
        w = np.zeros(shape + (16, 1024), dtype=np.uint64)
        for sl in slots:
            w[..., sl, :] = rng.integers(0, 1 << 63, shape + (1024,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (1024,), dtype=np.uint64)
        return w

    A, Bw, F = rnd(n_sh, n_a), rnd(n_sh, n_b), rnd(n_sh)
    S = rnd(n_sh, depth + 2)
    S[:, 0] &= rnd(n_sh)  # exists: a quarter of the columns
    if depth == 64:
        S[:, 10:] |= rnd(n_sh, 56) | rnd(n_sh, 56)  # planes 8..63 set on three quarters of the columns
    return A, Bw, F, S


@pytest.mark.parametrize("depth", [0, 1, 7, 20, 63, 64])
@pytest.mark.parametrize("with_filter", [False, True])
def test_oracle_composition_equals_numpy_brute_force(oracle, B, depth, with_filter):
    O = oracle
    rng = D.rng_for(7100, depth, int(with_filter))
    n_sh, n_a, n_b = 2, 3, 4
    A, Bw, F, S = _random_case(rng, n_sh, n_a, n_b, depth)
    Fx = F if with_filter else None
    sums, counts = R.numpy_expected(A, Bw, Fx, S, depth)
    a_bms = [[R.bitmap_of_words(O, A[s, i]) for i in range(n_a)] for s in range(n_sh)]
    b_bms = [[R.bitmap_of_words(O, Bw[s, j]) for j in range(n_b)] for s in range(n_sh)]
    f_bms = [R.bitmap_of_words(O, F[s]) for s in range(n_sh)] if with_filter else None
    frags = [R.fragment_of_words(O, B, S[s]) for s in range(n_sh)]
    pairs = [(i, j) for i in range(n_a) for j in range(n_b)]
    exp = R.oracle_expected(O, B, a_bms, b_bms, f_bms, frags, pairs)
    for (i, j), (sm, c) in exp.items():
        assert (int(sums[i, j]), int(counts[i, j])) == (sm, c), (i, j)
    assert counts.sum() > 0
    if depth:
        assert (sums != 0).any()
    if depth == 64:
        assert (sums < 0).any() or (sums > (1 << 62)).any()  # the wrap-around is exercised
    # the one-field form: B absent
    s1, c1 = R.numpy_expected(A, None, Fx, S, depth)
    e1 = R.oracle_expected(O, B, a_bms, None, f_bms, frags, [(i, 0) for i in range(n_a)])
    for (i, _), (sm, c) in e1.items():
        assert (int(s1[i, 0]), int(c1[i, 0])) == (sm, c), i


def test_numpy_brute_force_by_hand():
    """one shard, one column of each kind: value -5 on column 3 (exists), 6 on column 70 (exists, outside the filter),
    a sign / plane bit on column 5 that has no exists bit"""
    S = np.zeros((1, 5, 16, 1024), dtype=np.uint64)
    S[0, 0, 0, 0] = 1 << 3
    S[0, 0, 0, 1] = 1 << 6         # column 70
    S[0, 1, 0, 0] = (1 << 3) | (1 << 5)
    S[0, 2, 0, 0] = (1 << 3) | (1 << 5)  # plane 0
    S[0, 4, 0, 0] = 1 << 3          # plane 2: |v| = 5
    S[0, 3, 0, 1] = 1 << 6          # plane 1
    S[0, 4, 0, 1] = 1 << 6          # plane 2: 6
    A = np.zeros((1, 1, 16, 1024), dtype=np.uint64)
    A[0, 0, 0, 0] = (1 << 3) | (1 << 5)
    A[0, 0, 0, 1] = 1 << 6
    sums, counts = R.numpy_expected(A, None, None, S, 3)
    assert (int(sums[0, 0]), int(counts[0, 0])) == (1, 2)
    F = np.zeros((1, 16, 1024), dtype=np.uint64)
    F[0, 0, 0] = ~np.uint64(0)
    sums, counts = R.numpy_expected(A, None, F, S, 3)
    assert (int(sums[0, 0]), int(counts[0, 0])) == (-5, 1)
