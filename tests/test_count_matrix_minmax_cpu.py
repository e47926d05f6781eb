"""fbk_count_matrix_minmax without a device: the ABI is declared and bound, bad arguments are errors (not crashes), the path rule of
featurebase_amd/csrc/fbk_minmax_plan.h at its boundaries (the header compiled into a stand-alone checker), and the two ways the GPU
tests compute expected values — the numpy brute force ordered by (class, magnitude) and the reference's composition (the oracle's
intersect, fragment.min / fragment.max, ValCount.Smaller / Larger) — agree on random small fragments with sign and plane bits
outside exists.  Where the two are DEFINED to differ the data avoids it: the sign is cleared wherever the magnitude is 0 (the
reference counts such columns apart from +0), and at depth 64 plane 63 is clear inside exists (the reference's fold over the shards
compares wrapped int64 values); the by-hand cases cover both corners for the numpy model."""
import numpy as np
import pytest

import datagen as D
import minmax_ref as M


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


def test_signature_declared(lib):
    assert "fbk_count_matrix_minmax" in lib.SIGNATURES
    assert getattr(lib.load(), "fbk_count_matrix_minmax") is not None
    assert len(lib.SIGNATURES["fbk_count_matrix_minmax"][1]) == 18
    assert (lib.MINMAX_AUTO, lib.MINMAX_DESCENT, lib.MINMAX_SCATTER) == (0, 1, 2)


def test_null_and_bad_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    f = l.fbk_count_matrix_minmax
    mn, mx = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    c0, c1 = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    rows = np.zeros(4, dtype=np.uint32)
    r, o = rows.ctypes.data, (mn.ctypes.data, mx.ctypes.data, c0.ctypes.data, c1.ctypes.data)
    E = lib.FBK_E_INVALID
    assert f(None, None, None, 0, None, None, 1, None, None, None, None, 0, 0, 0, None, None, None, None) == E
    assert f(None, None, r, 1, None, None, 1, None, None, None, r, 20, 1, 0, *o) == E  # NULL ctx / a / bsi
    assert f(None, None, r, 1, None, None, 1, None, None, None, r, 20, 1, 0, o[0], o[1], o[2], None) == E  # one count pointer
    assert f(None, None, r, 1, None, None, 1, None, None, None, r, 20, 1, 0, o[0], o[1], None, o[3]) == E
    assert f(None, None, r, 1, None, None, 1, None, None, None, r, 20, 1, 3, *o) == E  # flags 3
    assert f(None, None, r, 1, None, None, 1, None, None, None, r, 65, 1, 0, *o) == E  # depth 65
    assert f(None, None, r, 4097, None, None, 1, None, None, None, r, 65, 1, 1, None, None, None, None) == E
    assert l.fbk_last_error(None) is not None
    assert not mn.any() and not mx.any() and not c0.any() and not c1.any()  # nothing was written


def test_the_path_rule_at_its_boundaries():
    AUTO, DESCENT, SCATTER = 0, 1, 2
    cells, cap = M.plan_constants()
    assert cells % 64 == 0 and cap % 64 == 0 and 64 <= cells <= cap <= 1024
    ask = lambda *qs: [g[0] for g in M.plan_check(["P %d %d %d" % q for q in qs])]
    # AUTO: the descent up to kMinmaxDescentCells groups, the scatter from the next one on, whatever the two sides are
    assert ask((cells, 1, AUTO), (1, cells, AUTO), (cells // 8, 8, AUTO), (1, 1, AUTO)) == [DESCENT] * 4
    assert ask((cells + 1, 1, AUTO), (1, cells + 1, AUTO), (cap, 1, AUTO) if cap > cells else (cap + 1, 1, AUTO), (4096, 4096, AUTO)) == [SCATTER] * 4
    # the pins: the descent up to the hard cap and an error above it, the scatter always
    assert ask((cap, 1, DESCENT), (cap // 64, 64, DESCENT), (1, 1, DESCENT)) == [DESCENT] * 3
    assert ask((cap + 1, 1, DESCENT), (33, 65, DESCENT), (4096, 4096, DESCENT)) == [0] * 3
    assert ask((1, 1, SCATTER), (cells, 1, SCATTER), (4096, 4096, SCATTER)) == [SCATTER] * 3
    assert ask((1, 1, 3), (1, 1, 4), (4096, 4096, 1 << 31)) == [0] * 3  # unknown flags
    # the descent's grid keeps the partials of a launch within kDescentBlocks blocks of 64 groups
    blocks = M.plan_check(["K"])[0][2]
    for ns, c in [(1, 1), (1, 64), (1, 65), (3, cap), (128, 64), (128, cap), (1 << 20, cap), (1 << 20, 1)]:
        tiles, grid = M.plan_check(["G %d %d" % (ns, c)])[0]
        assert tiles == -(-c // 64) and 1 <= grid and grid * tiles <= blocks and grid <= -(-ns * 1024 // 4)
        assert grid == min(-(-ns * 1024 // 4), blocks // tiles)
    # the densify chunk: 128 KiB per densified row of a shard in 2^30 bytes, the shards dealt evenly
    assert [g[0] for g in M.plan_check(["C 118 69", "C 119 69", "C 60 0", "C 0 5", "C 1 100000", "C 200 66"])] == [118, 60, 60, 0, 1, 100]


def _random_case(rng, n_sh, n_a, n_b, depth, slots=(0, 9)):
    """A / B / F about half the columns of two slots, exists a quarter, sign and planes everywhere (also outside exists); the
    planes from 3 on sparse, so that columns share values and the counts exceed 1; the sign cleared where the magnitude is 0"""
    def rnd(*shape):
        w = np.zeros(shape + (16, 1024), dtype=np.uint64)
        for sl in slots:
            w[..., sl, :] = rng.integers(0, 1 << 63, shape + (1024,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (1024,), dtype=np.uint64)
        return w

    A, Bw, F = rnd(n_sh, n_a), rnd(n_sh, n_b), rnd(n_sh)
    S = rnd(n_sh, depth + 2)
    S[:, 0] &= rnd(n_sh)
    if depth > 3:
        S[:, 5:] &= rnd(n_sh, depth - 3) & rnd(n_sh, depth - 3) & rnd(n_sh, depth - 3) & rnd(n_sh, depth - 3)
    if depth == 64:
        S[:, 40:65] |= rnd(n_sh, 25) & rnd(n_sh, 25)  # high planes set on a quarter of the columns
        S[:, 65] &= ~S[:, 0]                          # plane 63 only outside exists (the module's docstring)
    S[:, 2:, 0, :4] = 0  # magnitude 0 on slot 0's first 256 columns
    anymag = np.bitwise_or.reduce(S[:, 2:], axis=1) if depth else np.zeros_like(S[:, 0])
    S[:, 1] &= anymag | ~S[:, 0]  # no sign over magnitude 0 inside exists; outside exists it stays
    return A, Bw, F, S


@pytest.mark.parametrize("depth", [0, 1, 7, 20, 63, 64])
@pytest.mark.parametrize("with_filter", [False, True])
def test_numpy_brute_force_equals_the_reference_composition(oracle, B, depth, with_filter):
    O = oracle
    rng = D.rng_for(8100, depth, int(with_filter))
    n_sh, n_a, n_b = 2, 3, 4
    A, Bw, F, S = _random_case(rng, n_sh, n_a, n_b, depth)
    Fx = F if with_filter else None
    a_bms = [[M.bitmap_of_words(O, A[s, i]) for i in range(n_a)] for s in range(n_sh)]
    b_bms = [[M.bitmap_of_words(O, Bw[s, j]) for j in range(n_b)] for s in range(n_sh)]
    f_bms = [M.bitmap_of_words(O, F[s]) for s in range(n_sh)] if with_filter else None
    frags = [M.fragment_of_words(O, B, S[s]) for s in range(n_sh)]
    mins, maxs, cmin, cmax = M.numpy_expected(A, Bw, Fx, S, depth)
    pairs = [(i, j) for i in range(n_a) for j in range(n_b)]
    for (i, j), want in M.oracle_expected(O, B, a_bms, b_bms, f_bms, frags, depth, pairs).items():
        assert (int(mins[i, j]), int(maxs[i, j]), int(cmin[i, j]), int(cmax[i, j])) == want, (i, j)
    assert (cmin > 0).all() and (mins <= maxs).all()
    if depth <= 1:
        assert (cmin > 1).all() and (cmax > 1).all()
    if depth >= 7:
        assert (mins < 0).all() and (maxs > 0).all()
    m1 = M.numpy_expected(A, None, Fx, S, depth)  # the one-field form: B absent
    for (i, _), want in M.oracle_expected(O, B, a_bms, None, f_bms, frags, depth, [(i, 0) for i in range(n_a)]).items():
        assert tuple(int(x[i, 0]) for x in m1) == want, i


def test_numpy_brute_force_by_hand():
    """one shard, depth 3: -5 on column 3, +5 on column 4, 0 on column 5 (sign set, magnitude 0) and column 6 (no sign), -5 on
    column 70 (outside the filter), sign / plane bits on column 7 (no exists bit)"""
    S = np.zeros((1, 5, 16, 1024), dtype=np.uint64)
    S[0, 0, 0, 0] = 0b1111000
    S[0, 0, 0, 1] = 1 << 6  # column 70
    S[0, 1, 0, 0] = (1 << 3) | (1 << 5) | (1 << 7)
    S[0, 1, 0, 1] = 1 << 6
    S[0, 2, 0, 0] = (1 << 3) | (1 << 4) | (1 << 7)  # plane 0
    S[0, 4, 0, 0] = (1 << 3) | (1 << 4) | (1 << 7)  # plane 2: |v| = 5
    S[0, 2, 0, 1] = S[0, 4, 0, 1] = 1 << 6
    A = np.zeros((1, 4, 16, 1024), dtype=np.uint64)
    A[0, 0, 0, 0] = 0b11111000  # columns 3..7 and 70: {-5, 5, 0, 0, -5}
    A[0, 0, 0, 1] = 1 << 6
    A[0, 1, 0, 0] = (1 << 5) | (1 << 6)  # +0 and the sign over zero: min = max = 0, both columns counted
    A[0, 2, 0, 0] = 1 << 7  # only bits without exists: empty
    A[0, 3, 0, 0] = (1 << 4) | (1 << 5)  # {5, 0 (sign over zero)}
    mn, mx, c0, c1 = M.numpy_expected(A, None, None, S, 3)
    assert mn[:, 0].tolist() == [-5, 0, M.INT64_MAX, 0] and mx[:, 0].tolist() == [5, 0, M.INT64_MIN, 5]
    assert c0[:, 0].tolist() == [2, 2, 0, 1] and c1[:, 0].tolist() == [1, 2, 0, 1]
    F = np.zeros((1, 16, 1024), dtype=np.uint64)
    F[0, 0, 0] = ~np.uint64(0)  # column 70 is outside it
    mn, mx, c0, c1 = M.numpy_expected(A, None, F, S, 3)
    assert mn[:, 0].tolist() == [-5, 0, M.INT64_MAX, 0] and c0[:, 0].tolist() == [1, 2, 0, 1] and c1[:, 0].tolist() == [1, 2, 0, 1]
    Bw = np.zeros((1, 2, 16, 1024), dtype=np.uint64)
    Bw[0, 0, 0, 0] = 1 << 3
    Bw[0, 1, 0, 1] = 1 << 6
    mn, mx, c0, c1 = M.numpy_expected(A, Bw, None, S, 3)
    assert mn.tolist() == [[-5, -5]] + [[M.INT64_MAX] * 2] * 3 and mx.tolist() == [[-5, -5]] + [[M.INT64_MIN] * 2] * 3
    assert c0.tolist() == [[1, 1], [0, 0], [0, 0], [0, 0]] and c1.tolist() == c0.tolist()


def test_numpy_orders_65_bit_values_at_depth_64():
    """two shards, depth 64: +(2^63 + 1) in shard 0 (written as int64 it wraps to INT64_MIN + 1), +3 and -(2^64 - 1) in shard 1
    (written: +1).  By value the minimum is -(2^64 - 1) and the maximum 2^63 + 1; the wrapped int64 would say otherwise."""
    S = np.zeros((2, 66, 16, 1024), dtype=np.uint64)
    S[0, 0, 0, 0] = 1
    S[0, 2, 0, 0] = S[0, 65, 0, 0] = 1  # column 0: planes 0 and 63
    S[1, 0, 0, 0] = 0b110
    S[1, 2, 0, 0] = S[1, 3, 0, 0] = 0b010  # column 1: +3
    S[1, 1, 0, 0] = 0b100
    S[1, 2:, 0, 0] |= np.uint64(0b100)  # column 2: every plane, negative
    A = np.zeros((2, 2, 16, 1024), dtype=np.uint64)
    A[:, 0, 0, 0] = 0b111
    A[:, 1, 0, 0] = 0b011
    mn, mx, c0, c1 = M.numpy_expected(A, None, None, S, 64)
    assert mn[:, 0].tolist() == [1, 3] and mx[:, 0].tolist() == [M.INT64_MIN + 1, M.INT64_MIN + 1]
    assert c0[:, 0].tolist() == [1, 1] and c1[:, 0].tolist() == [1, 1]


def test_nineteen_shards_take_every_kernel_round_its_loop():
    """what tests/test_gpu_count_matrix_minmax.py's 19-shard cases rest on: k_minmax_scatter / _holders run min(ceil(ns * 1024 / 4),
    2048) blocks of four units, the descent descent_grid() blocks per tile"""
    n = M.MANY_SHARDS
    assert min(-(-n * 1024 // 4), 2048) * 4 == 8 * 1024 and n > 2 * 8  # the scatter: 8 shards a round, two whole rounds and a part
    grid = lambda cells: tuple(M.plan_check(["G %d %d" % (n, cells)])[0])  # noqa: E731  (tiles, unit blocks)
    assert grid(5 * 7) == (1, 2048) and grid(13 * 11) == (3, 682) and grid(70) == (2, 1024)
    assert (682 * 4) % 1024 != 0 and 682 % 64 != 0 and -(-n * 1024 // (682 * 4)) == 8  # steps of 2 or 3 shards, 8 rounds (the last a part)
    steps = {(r + 1) * 2728 // 1024 - r * 2728 // 1024 for r in range(7)}
    assert steps == {2, 3}
    cells, cap = M.plan_constants()
    assert 5 * 7 <= cells < 70 <= 13 * 11 <= cap < 33 * 65 and -(-65 // 64) == 2
    assert len(M.MANY_ROWS) == len(M.MANY_FRAG) == n and set(M.MANY_FRAG[:8]) == {0, 1, 2} and set(M.MANY_FRAG[8:]) == {3, 4}
    pairs = list(zip(M.MANY_ROWS, M.MANY_FRAG))
    assert len(set(pairs)) == n - 1 and pairs[18] == pairs[8]


def _fold(parts, keep):
    """per-shard results -> the call's over the shards `keep` (depth <= 63: the written int64 is the value)"""
    mn = np.min([parts[s][0] for s in keep], axis=0)
    mx = np.max([parts[s][1] for s in keep], axis=0)
    c0 = np.sum([np.where(parts[s][0] == mn, parts[s][2], 0) for s in keep], axis=0, dtype=np.uint64)
    c1 = np.sum([np.where(parts[s][1] == mx, parts[s][3], 0) for s in keep], axis=0, dtype=np.uint64)
    return mn, mx, c0, c1


@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("depth", [7, 20])
@pytest.mark.parametrize("shape", [(5, 7), (13, 11), (33, 65), (70, None)])
def test_nineteen_shard_cases_tell_a_shard_lost_beyond_the_first_round(shape, depth, with_filter):
    """a condition on the inputs of the GPU test, checked with the reference alone: the result over shards [0, 8) differs from the
    full one in the minimum and in the maximum of at least a quarter of the non-empty groups, and the result without any one of
    the shards 8 .. 18 differs from the full one in the counts"""
    n_a, n_b = shape
    A, Bw, F, S = M.many_shard_case(n_a, n_b, depth)
    one = {}  # the shards that read the same rows and fragment share a result
    for s in range(M.MANY_SHARDS):
        key = (M.MANY_ROWS[s], M.MANY_FRAG[s])
        if key not in one:
            a, b, f, sw = M.many_shard_words(A, Bw, F, S, [s])
            one[key] = M.numpy_expected(a, b, f if with_filter else None, sw, depth)
    parts = [one[(M.MANY_ROWS[s], M.MANY_FRAG[s])] for s in range(M.MANY_SHARDS)]
    every = list(range(M.MANY_SHARDS))
    full = _fold(parts, every)
    if shape == (5, 7):  # the fold of the per-shard results is the reference over all the words at once
        a, b, f, sw = M.many_shard_words(A, Bw, F, S)
        for x, y in zip(full, M.numpy_expected(a, b, f if with_filter else None, sw, depth)):
            assert x.dtype == y.dtype and np.array_equal(x, y)
    held = full[2] > 0
    assert held.sum() * 2 > held.size and (full[0][held] < 0).all() and (full[1][held] > 0).all()
    first = _fold(parts, every[:8])
    assert ((first[0] != full[0]) & held).sum() * 4 >= held.sum() and ((first[1] != full[1]) & held).sum() * 4 >= held.sum()
    for s in range(8, M.MANY_SHARDS):
        without = _fold(parts, [t for t in every if t != s])
        assert not (np.array_equal(without[2], full[2]) and np.array_equal(without[3], full[3])), ("shard", s)
    # the tie counts differ from group to group: a result written to another group's place shows
    assert np.unique(full[2][held]).size > 3 and np.unique(full[3][held]).size > 3
