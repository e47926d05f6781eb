"""fbk_count_matrix_distinct without a device: the ABI is declared and bound, bad arguments are errors (not crashes), and the two
ways the GPU tests compute expected values — a numpy brute force over (group, value) pairs and a slow per-group path (the oracle's
intersect, then every column's value read from the planes) — agree on random small fragments: depth-64 magnitudes, negative
values, a set sign bit with magnitude 0, sign and plane bits outside exists."""
import numpy as np
import pytest

import datagen as D
import mdist_ref as M
import msum_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


def test_signature_declared(lib):
    assert "fbk_count_matrix_distinct" in lib.SIGNATURES
    assert getattr(lib.load(), "fbk_count_matrix_distinct") is not None
    assert len(lib.SIGNATURES["fbk_count_matrix_distinct"][1]) == 15


def test_null_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    d, c = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    rows = np.zeros(4, dtype=np.uint32)
    f = l.fbk_count_matrix_distinct
    assert f(None, None, None, 0, None, None, 1, None, None, None, None, 0, 0, None, None) == lib.FBK_E_INVALID
    assert f(None, None, rows.ctypes.data, 1, None, None, 1, None, None, None, rows.ctypes.data, 20, 1, d.ctypes.data, c.ctypes.data) == lib.FBK_E_INVALID
    assert f(None, None, rows.ctypes.data, 1, None, None, 1, None, None, None, rows.ctypes.data, 20, 1, d.ctypes.data, None) == lib.FBK_E_INVALID
    assert f(None, None, rows.ctypes.data, 4097, None, None, 1, None, None, None, rows.ctypes.data, 65, 1, None, None) == lib.FBK_E_INVALID
    assert l.fbk_last_error(None) is not None


def _random_case(rng, n_sh, n_a, n_b, depth, slots=(0, 9)):
    """A / B / F about half the columns of two slots, exists a quarter, sign and planes everywhere (also outside exists); few
    distinct magnitudes so that groups share values; at depth 64 some magnitudes near 2^64 and some sign bits over magnitude 0"""
    def rnd(*shape):
        w = np.zeros(shape + (16, 1024), dtype=np.uint64)
        for sl in slots:
            w[..., sl, :] = rng.integers(0, 1 << 63, shape + (1024,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (1024,), dtype=np.uint64)
        return w

    A, Bw, F = rnd(n_sh, n_a), rnd(n_sh, n_b), rnd(n_sh)
    S = rnd(n_sh, depth + 2)
    S[:, 0] &= rnd(n_sh)
    if depth > 3:
        S[:, 5:] &= rnd(n_sh, depth - 3) & rnd(n_sh, depth - 3) & rnd(n_sh, depth - 3)  # planes 3.. sparse: values repeat
    if depth == 64:
        S[:, 40:] |= rnd(n_sh, 26) & rnd(n_sh, 26)  # high planes set on a quarter of the columns
    S[:, 2:, 0, :4] = 0  # magnitude 0 on slot 0's first 256 columns (some with the sign bit)
    return A, Bw, F, S


@pytest.mark.parametrize("depth", [0, 1, 7, 20, 64])
@pytest.mark.parametrize("with_filter", [False, True])
def test_numpy_brute_force_equals_per_group_path(oracle, depth, with_filter):
    O = oracle
    rng = D.rng_for(7600, depth, int(with_filter))
    n_sh, n_a, n_b = 2, 3, 4
    A, Bw, F, S = _random_case(rng, n_sh, n_a, n_b, depth)
    Fx = F if with_filter else None
    dist, counts = M.numpy_expected(A, Bw, Fx, S, depth)
    a_bms = [[R.bitmap_of_words(O, A[s, i]) for i in range(n_a)] for s in range(n_sh)]
    b_bms = [[R.bitmap_of_words(O, Bw[s, j]) for j in range(n_b)] for s in range(n_sh)]
    f_bms = [R.bitmap_of_words(O, F[s]) for s in range(n_sh)] if with_filter else None
    pairs = [(0, 0), (1, 2), (n_a - 1, n_b - 1)]
    for (i, j), (dc, c) in M.slow_expected(O, a_bms, b_bms, f_bms, S, depth, pairs).items():
        assert (int(dist[i, j]), int(counts[i, j])) == (dc, c), (i, j)
    assert (dist > 0).all() and (dist < counts).all() if depth <= 7 else (dist > 0).all()
    d1, c1 = M.numpy_expected(A, None, Fx, S, depth)  # the one-field form: B absent
    for (i, _), (dc, c) in M.slow_expected(O, a_bms, None, f_bms, S, depth, [(i, 0) for i in range(n_a)]).items():
        assert (int(d1[i, 0]), int(c1[i, 0])) == (dc, c), i


def test_numpy_brute_force_by_hand():
    """one shard: -5 on column 3, +5 on column 4, 0 on column 5 (sign set, magnitude 0) and column 6 (no sign), -5 on column 70
    (outside the filter), sign / plane bits on column 7 (no exists bit)"""
    S = np.zeros((1, 5, 16, 1024), dtype=np.uint64)
    S[0, 0, 0, 0] = 0b1111000
    S[0, 0, 0, 1] = 1 << 6  # column 70
    S[0, 1, 0, 0] = (1 << 3) | (1 << 5) | (1 << 7)
    S[0, 1, 0, 1] = 1 << 6
    S[0, 2, 0, 0] = (1 << 3) | (1 << 4) | (1 << 7)  # plane 0
    S[0, 4, 0, 0] = (1 << 3) | (1 << 4) | (1 << 7)  # plane 2: |v| = 5
    S[0, 2, 0, 1] = S[0, 4, 0, 1] = 1 << 6
    A = np.zeros((1, 2, 16, 1024), dtype=np.uint64)
    A[0, 0, 0, 0] = 0b11111000
    A[0, 0, 0, 1] = 1 << 6
    A[0, 1, 0, 0] = (1 << 5) | (1 << 6)
    dist, counts = M.numpy_expected(A, None, None, S, 3)
    assert dist[:, 0].tolist() == [3, 1] and counts[:, 0].tolist() == [5, 2]  # {-5, 5, 0}; {0}
    F = np.zeros((1, 16, 1024), dtype=np.uint64)
    F[0, 0, 0] = ~np.uint64(0)
    dist, counts = M.numpy_expected(A, None, F, S, 3)
    assert dist[:, 0].tolist() == [3, 1] and counts[:, 0].tolist() == [4, 2]
    Bw = np.zeros((1, 2, 16, 1024), dtype=np.uint64)
    Bw[0, 0, 0, 0] = 1 << 3
    Bw[0, 1, 0, 1] = 1 << 6
    dist, counts = M.numpy_expected(A, Bw, None, S, 3)
    assert dist.tolist() == [[1, 1], [0, 0]] and counts.tolist() == [[1, 1], [0, 0]]
