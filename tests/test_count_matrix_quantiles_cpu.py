"""fbk_count_matrix_quantiles without a device: the ABI is declared and bound, bad arguments are errors (not crashes), the rules of
featurebase_amd/csrc/fbk_group_quantile_plan.h at their boundaries (the header compiled into a stand-alone checker), the numpy
model of the GPU tests (tests/gquant_ref.py) against an independent composition (pct_ref.quantiles on the values of A_i & B_j & F,
selected separately, with the rank from exact fractions), the rank rule by hand, and the order at depth 64."""
import math
from fractions import Fraction

import numpy as np
import pytest

import datagen as D
import gquant_ref as G
import pct_ref as P


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


def test_signature_declared(lib):
    assert "fbk_count_matrix_quantiles" in lib.SIGNATURES
    assert getattr(lib.load(), "fbk_count_matrix_quantiles") is not None
    assert len(lib.SIGNATURES["fbk_count_matrix_quantiles"][1]) == 20
    assert (lib.GQUANT_AUTO, lib.GQUANT_LDS, lib.GQUANT_GLOBAL) == (0, 1, 2)
    from featurebase_amd.roaring import Context

    assert callable(Context.count_matrix_quantiles)


def test_null_and_bad_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    f = l.fbk_count_matrix_quantiles
    vals, cnts, tot = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    rows = np.zeros(4, dtype=np.uint32)
    r, o = rows.ctypes.data, (vals.ctypes.data, cnts.ctypes.data, tot.ctypes.data)
    u32 = lambda *x: np.array(x, dtype=np.uint32)
    one, two = u32(1), u32(2)
    E = lib.FBK_E_INVALID

    def bad(what, *args):
        assert f(*args) == E
        assert what in l.fbk_last_error(None).decode(), (what, l.fbk_last_error(None))

    ok_q = (one.ctypes.data, two.ctypes.data, 1)  # the median
    head = (None, None, r, 1, None, None, 1, None, None, None, r, 20, 1)  # NULL ctx / a / bsi
    bad("NULL", *head, *ok_q, 0, *o)
    bad("NULL", None, None, None, 0, None, None, 1, None, None, None, None, 0, 0, None, None, 0, 0, None, None, None)
    bad("NULL", *head, *ok_q, 0, o[0], o[1], None)  # out_totals
    bad("NULL", *head, None, two.ctypes.data, 1, 0, *o)  # q_num
    bad("NULL", *head, one.ctypes.data, None, 1, 0, *o)  # q_den
    bad("NULL", *head, *ok_q, 0, None, o[1], o[2])  # out_values
    bad("NULL", *head, *ok_q, 0, o[0], None, o[2])  # out_counts
    zero, big, mx = u32(0), u32((1 << 20) + 1), u32(1 << 20)
    bad("num / den", *head, one.ctypes.data, zero.ctypes.data, 1, 0, *o)  # den == 0
    bad("num / den", *head, one.ctypes.data, big.ctypes.data, 1, 0, *o)  # den > 2^20
    bad("num / den", *head, two.ctypes.data, one.ctypes.data, 1, 0, *o)  # num > den
    bad("NULL", *head, mx.ctypes.data, mx.ctypes.data, 1, 0, *o)  # 2^20 / 2^20 is a request: the NULL context is what fails
    many = np.ones(17, dtype=np.uint32)
    bad("at most 16", *head, many.ctypes.data, many.ctypes.data, 17, 0, *o)
    bad("NULL", *head, many.ctypes.data, many.ctypes.data, 16, 0, *o)
    bad("unknown flags", *head, *ok_q, 3, *o)
    bad("unknown flags", *head, *ok_q, 1 << 31, *o)
    # n_a / n_b > 4096, bit_depth > 64, b == NULL with n_b != 1: behind the NULL checks (a device test shows their own messages)
    bad("NULL", None, None, r, 4097, None, None, 1, None, None, None, r, 65, 1, *ok_q, 0, *o)
    bad("NULL", None, None, r, 1, None, None, 2, None, None, None, r, 20, 1, *ok_q, 0, *o)
    assert not vals.any() and not cnts.any() and not tot.any()  # nothing was written


def test_the_plan_header_at_its_boundaries():
    AUTO, LDS, GLOBAL = 0, 1, 2
    k = G.plan_constants()
    dl, dg, cap, auto = k["lds_digit"], k["global_digit"], k["lds_cap"], k["auto_pairs"]
    assert 8 <= dl <= 12 and 8 <= dg <= 12 and k["max_den"] == 1 << 20 and k["max_requests"] == 16 and k["scratch_bound"] == 1 << 30
    # the LDS cap: 32-bit counters of every (group, request) pair in 64 KiB
    assert cap == (64 << 10) // (4 << dl) and 1 <= auto <= cap
    # passes per depth: ceil((depth + 1) / digit) up to depth 63, the 64-bit key at 63 and 64
    for d in {8, 11, dl, dg}:
        for depth in range(65):
            bits, passes = G.plan_check(["N %d %d" % (depth, d)])[0]
            assert bits == min(depth + 1, 64) and passes == -(-bits // d) and passes >= 1
            if depth <= 63:
                assert passes == -(-(depth + 1) // d)
        assert [G.plan_check(["N %d %d" % (x, d)])[0][1] for x in (0, d - 2, d - 1, d, 2 * d - 1, 2 * d)] == [1, 1, 1, 2, 2, 3]
        # the passes tile the key from the top in whole digits; the short digit comes last
        for depth in (0, d - 1, d, 20, 62, 63, 64):
            bits, passes = G.plan_check(["N %d %d" % (depth, d)])[0]
            cuts = G.plan_check(["B %d %d %d" % (depth, d, p) for p in range(passes)])
            assert cuts[0][0] + cuts[0][1] == bits and cuts[-1][0] == 0 and all(w == d for _, w in cuts[:-1]) and 1 <= cuts[-1][1] <= d
            assert all(cuts[p][0] == cuts[p + 1][0] + cuts[p + 1][1] for p in range(passes - 1))
    # the scratch: pairs * 2^digit * 8 bytes; 4096 x 4096 x 16 is far beyond the bound at either digit, and no 64-bit overflow
    ask = lambda *qs: [g[0] for g in G.plan_check(["S %d %d %d %d" % q for q in qs])]
    assert ask((4096, 4096, 16, 8), (4096, 4096, 16, 11), (4096, 4096, 0, 8)) == [4096 * 4096 * 16 * 2048, 4096 * 4096 * 16 * 16384, 4096 * 4096 * 2048]
    assert ask((4096, 4096, 16, dg))[0] > k["scratch_bound"]
    most = k["scratch_bound"] // (8 << dg)  # the most pairs a call takes
    assert ask((most, 1, 1, dg), (most // 16, 1, 16, dg), (most, 1, 0, dg))[0:3] == [k["scratch_bound"]] * 3 and ask((most + 1, 1, 1, dg))[0] > k["scratch_bound"]
    assert ask((5, 7, 3, dg), (5, 1, 0, dl)) == [105 * (8 << dg), 5 * (8 << dl)]
    # the path rule: AUTO by the pairs n_a * n_b * max(1, n_q); the LDS pin up to its cap, the GLOBAL pin always; unknown flags
    path = lambda *qs: [g[0] for g in G.plan_check(["P %d %d %d %d" % q for q in qs])]
    assert path((auto, 1, 1, AUTO), (1, auto, 0, AUTO), (1, 1, auto, AUTO) if auto <= 16 else (1, 1, 1, AUTO), (1, 1, 0, AUTO)) == [LDS] * 4
    assert path((auto + 1, 1, 1, AUTO), (1, auto + 1, 0, AUTO), (auto, 1, 2, AUTO), (4096, 4096, 16, AUTO)) == [GLOBAL] * 4
    assert path((cap, 1, 1, LDS), (1, cap, 0, LDS), (cap // 16, 1, 16, LDS), (1, 1, 16, LDS)) == [LDS] * 4
    assert path((cap + 1, 1, 1, LDS), (cap, 1, 2, LDS), (64, 64, 1, LDS), (4096, 4096, 16, LDS)) == [0] * 4
    assert path((1, 1, 0, GLOBAL), (cap, 1, 1, GLOBAL), (4096, 4096, 16, GLOBAL)) == [GLOBAL] * 3
    assert path((1, 1, 1, 3), (1, 1, 1, 4), (4096, 4096, 16, 1 << 31)) == [0] * 3
    # the densify chunk: the minmax scatter path's rule
    assert [g[0] for g in G.plan_check(["C 118 69", "C 119 69", "C 60 0", "C 0 5", "C 1 100000", "C 200 66"])] == [118, 60, 60, 0, 1, 100]


RANK_N = [1, 2, 4, 5, 100]
RANK_F = [(0, 1), (1, 2), (1, 4), (99, 100), (1, 1), (1, 1 << 20)]
# by hand: k = max(1, ceil(N * num / den)) - 1
RANK_BY_HAND = {
    1: [0, 0, 0, 0, 0, 0],
    2: [0, 0, 0, 1, 1, 0],
    4: [0, 1, 0, 3, 3, 0],
    5: [0, 2, 1, 4, 4, 0],
    100: [0, 49, 24, 98, 99, 0],
}


def test_the_rank_rule_by_hand():
    for n in RANK_N:
        assert [G.disc_rank(n, *f) for f in RANK_F] == RANK_BY_HAND[n], n
        assert [g[0] for g in G.plan_check(["R %d %d %d" % (n, *f) for f in RANK_F])] == RANK_BY_HAND[n], n
        for num, den in RANK_F:  # the definition in exact fractions
            assert G.disc_rank(n, num, den) == max(1, math.ceil(Fraction(n * num, den))) - 1
    # the largest arguments: N = 2^40 columns, den = 2^20: exact in 64 bits
    big = [(1 << 40, 1 << 20, 1 << 20), (1 << 40, (1 << 20) - 1, 1 << 20), ((1 << 40) - 1, 1, 1 << 20), ((1 << 40) - 1, 999983, 999984)]
    assert [g[0] for g in G.plan_check(["R %d %d %d" % b for b in big])] == [G.disc_rank(*b) for b in big]
    assert G.disc_rank(1 << 40, 1 << 20, 1 << 20) == (1 << 40) - 1 and G.disc_rank((1 << 40) - 1, 1, 1 << 20) == (1 << 20) - 1


def _rnd(rng, *shape):
    """words of two slots, about half the bits set"""
    w = np.zeros(shape + (16, 1024), dtype=np.uint64)
    for sl in (0, 9):
        w[..., sl, :] = rng.integers(0, 1 << 63, shape + (1024,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (1024,), dtype=np.uint64)
    return w


@pytest.mark.parametrize("depth", [0, 1, 7, 20, 63, 64])
@pytest.mark.parametrize("with_filter", [False, True])
def test_the_numpy_model_equals_an_independent_composition(depth, with_filter):
    rng = D.rng_for(9100, depth, int(with_filter))
    n_sh, n_a, n_b = 2, 3, 4
    A, Bw, F, S = _rnd(rng, n_sh, n_a), _rnd(rng, n_sh, n_b), _rnd(rng, n_sh), _rnd(rng, n_sh, depth + 2)
    S[:, 0] &= _rnd(rng, n_sh) & _rnd(rng, n_sh) & _rnd(rng, n_sh) & _rnd(rng, n_sh)
    if depth > 3:  # the planes from 3 on sparse: columns share values and the counts exceed 1
        S[:, 5:] &= _rnd(rng, n_sh, depth - 3) & _rnd(rng, n_sh, depth - 3) & _rnd(rng, n_sh, depth - 3) & _rnd(rng, n_sh, depth - 3)
    A[:, 2] &= _rnd(rng, n_sh) & _rnd(rng, n_sh) & _rnd(rng, n_sh) & _rnd(rng, n_sh) & _rnd(rng, n_sh)  # small groups
    A[1, 1] = 0
    fr = [(0, 1), (1, 2), (1, 4), (99, 100), (1, 1), (1, 1 << 20), (1, 2)]
    Fx = F if with_filter else None
    for Bx in (Bw, None):
        vals, cnts, totals = G.numpy_expected(A, Bx, Fx, S, depth, fr)
        assert vals.shape == (n_a, n_b if Bx is not None else 1, len(fr)) and totals.dtype == np.uint64 and vals.dtype == np.int64
        for i in range(n_a):
            for j in range(vals.shape[1]):
                sel = A[:, i] & (Bx[:, j] if Bx is not None else ~np.uint64(0))
                if with_filter:
                    sel = sel & F
                v = P.values(S, sel, depth)
                n = int(v.size)
                assert int(totals[i, j]) == n
                ranks = [max(1, math.ceil(Fraction(n * num, den))) - 1 for num, den in fr] if n else [0] * len(fr)
                ev, ec, _ = P.quantiles(v, ranks)
                assert vals[i, j].tolist() == ev.tolist() and cnts[i, j].tolist() == ec.tolist(), (i, j)
        assert (totals > 0).all() and (totals[2] < totals[0]).all()
        assert (vals[..., 0] <= vals[..., 4]).all() and (vals[..., 1] == vals[..., 6]).all()
        if depth <= 1:
            assert (cnts[:2] > 1).all()
        if depth >= 7:
            assert (vals[:2, :, 0] < 0).all() and (vals[:2, :, 4] > 0).all()


def test_the_model_by_hand():
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
    A[0, 0, 0, 0] = 0b11111000  # columns 3..7 and 70: sorted {-5, -5, 0, 0, 5}
    A[0, 0, 0, 1] = 1 << 6
    A[0, 1, 0, 0] = (1 << 5) | (1 << 6)  # +0 and the sign over zero
    A[0, 2, 0, 0] = 1 << 7  # only bits without exists: empty
    A[0, 3, 0, 0] = (1 << 4) | (1 << 5)  # {0 (sign over zero), 5}
    fr = [(0, 1), (1, 2), (1, 1), (2, 5), (3, 5)]
    v, c, t = G.numpy_expected(A, None, None, S, 3, fr)
    assert t[:, 0].tolist() == [5, 2, 0, 2]
    assert v[:, 0].tolist() == [[-5, 0, 5, -5, 0], [0] * 5, [0] * 5, [0, 0, 5, 0, 5]]
    assert c[:, 0].tolist() == [[2, 2, 1, 2, 2], [2] * 5, [0] * 5, [1, 1, 1, 1, 1]]
    F = np.zeros((1, 16, 1024), dtype=np.uint64)
    F[0, 0, 0] = ~np.uint64(0)  # column 70 is outside it
    v, c, t = G.numpy_expected(A, None, F, S, 3, fr)
    assert t[:, 0].tolist() == [4, 2, 0, 2] and v[0, 0].tolist() == [-5, 0, 5, 0, 0] and c[0, 0].tolist() == [1, 2, 1, 2, 2]


def test_the_order_at_depth_64_is_the_wrapped_int64_s():
    """two shards, depth 64, as fbk_bsi_quantiles: +(2^63 + 1) is written INT64_MIN + 1 and sorts FIRST, -(2^64 - 1) is written +1"""
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
    v, c, t = G.numpy_expected(A, None, None, S, 64, [(0, 1), (1, 2), (1, 1)])
    assert t[:, 0].tolist() == [3, 2]
    assert v[:, 0].tolist() == [[P.I64_MIN + 1, 1, 3], [P.I64_MIN + 1, P.I64_MIN + 1, 3]] and (c == 1).all()
    whole = P.quantiles(P.values(S, A[:, 0], 64), [0, 1, 2])
    assert whole[0].tolist() == [P.I64_MIN + 1, 1, 3]
