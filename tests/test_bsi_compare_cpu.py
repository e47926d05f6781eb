"""CPU checks of fbk_bsi_compare (no GPU): the ABI's shape, the host rules of featurebase_amd/csrc/fbk_compare_plan.h compiled into
a stand-alone program (tests/cpp/compare_plan_check.cpp, -fsanitize=address,undefined) against Python ints, and the two numpy
recurrences of tests/compare_ref.py — the arithmetic of the kernel's two instances — against the Python-int definition on random
fragments with junk outside exists and planted extreme columns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compare_ref as CR
import datagen as D
import moments_ref as M
from featurebase_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DEPTH_PAIRS = [(0, 0), (1, 1), (3, 7), (7, 3), (63, 64), (64, 64), (64, 0)]


@pytest.fixture(scope="module")
def checker():
    out = os.path.join(ROOT, "build", "compare_plan_check_san")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "compare_plan_check.cpp"), "-o", out])

    def run(lines):
        r = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"compare_plan_check exit {r.returncode}\n{r.stderr[-4000:]}"
        got = [l.split() for l in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got

    return run


def test_symbol_and_signature():
    lib = L.load()
    assert hasattr(lib, "fbk_bsi_compare")
    assert len(L.SIGNATURES["fbk_bsi_compare"][1]) == 16
    assert L.COMPARE_PATH_OFFSET == CR.PATH_OFFSET == 0x100
    assert (L.BSI_EQ, L.BSI_NEQ, L.BSI_LT, L.BSI_LTE, L.BSI_GT, L.BSI_GTE) == CR.OPS


def test_null_arguments_are_invalid():
    lib = L.load()
    rows = np.zeros(1, dtype=np.uint32)
    counts = np.zeros(1, dtype=np.uint64)
    h = C.c_void_p()
    fake = C.c_void_p(16)  # never dereferenced: a NULL argument is found first
    r, o, c = rows.ctypes.data, C.byref(h), counts.ctypes.data
    # without a device there is no context to enter: every call names ctx == NULL, alone and with the other NULLs the call rejects
    calls = [
        (None, fake, r, 1, 0, fake, r, 1, 0, L.BSI_LT, None, None, 1, 0, o, c),
        (None, None, r, 1, 0, fake, r, 1, 0, L.BSI_LT, None, None, 1, 0, o, c),  # x
        (None, fake, r, 1, 0, None, r, 1, 0, L.BSI_LT, None, None, 1, 0, o, c),  # y
        (None, fake, None, 1, 0, fake, None, 1, 0, L.BSI_LT, None, None, 1, 0, o, c),  # base rows
        (None, fake, r, 1, 0, fake, r, 1, 0, L.BSI_LT, fake, None, 1, 0, o, c),  # a filter without rows_f
        (None, fake, r, 1, 0, fake, r, 1, 0, L.BSI_LT, None, None, 1, 0, None, None),  # neither output
    ]
    for args in calls:
        assert lib.fbk_bsi_compare(*args) == L.FBK_E_INVALID
    assert h.value is None


def test_plan_rules_against_python_ints(checker):
    depths = [0, 1, 7, 63, 64]
    bases = [0, 1, -1, 1 << 40, -(1 << 40), I64_MIN, I64_MAX]
    grid = [(dx, dy, bx, by, fl) for dx in depths for dy in depths for bx in bases for by in bases for fl in (0, CR.PATH_OFFSET)]
    got = checker([f"P {dx} {dy} {bx} {by} {fl} {CR.LT}" for dx, dy, bx, by, fl in grid])
    ks = set()
    for (dx, dy, bx, by, fl), g in zip(grid, got):
        k = bx - by
        ks.add(k)
        general = k != 0 or fl != 0
        assert int(g[1]) == int(general) == int(CR.is_general(k, fl)), (dx, dy, bx, by, fl)
        want = max(dx, dy, abs(k).bit_length()) + 2 if general else max(dx, dy)
        assert int(g[0]) == want == CR.steps(dx, dy, k, fl), (dx, dy, bx, by, fl)
        assert g[6] == "".join(str((k >> i) & 1) for i in range(140)), (bx, by)
        # W bits hold both streams: |±mx + k| and |my| stay below 2^(W - 1)
        if general:
            assert ((1 << dx) - 1) + abs(k) < 1 << (want - 1) and (1 << dy) - 1 < 1 << (want - 1)
    assert (1 << 64) - 1 in ks and -((1 << 64) - 1) in ks and max(int(g[0]) for g in got) == 66
    # the operators: result = E & (((lt & take_lt) | (gt & take_gt)) ^ invert), against the truth table of the three outcomes
    rows = checker([f"P 1 1 0 0 0 {op}" for op in (0, 1, 2, 3, 4, 5, 6, 7, -1)])
    assert [int(r[5]) for r in rows] == [0, 1, 1, 1, 1, 1, 1, 0, 0]
    truth = {CR.EQ: (0, 1, 0), CR.NEQ: (1, 0, 1), CR.LT: (1, 0, 0), CR.LTE: (1, 1, 0), CR.GT: (0, 0, 1), CR.GTE: (0, 1, 1)}  # (x < y, x == y, x > y)
    for op, r in zip(range(9), rows):
        if op in truth:
            tl, tg, inv = int(r[2]), int(r[3]), int(r[4])
            assert tuple(((l & tl) | (g & tg)) ^ inv for l, g in ((1, 0), (0, 0), (0, 1))) == truth[op], op
    assert checker(["K"]) == [["64", str(1 << 27), str(CR.PATH_OFFSET)]]


def _fragment(rng, depth, n_cols, density=0.7):
    """[depth + 2, 16, 1024] words with values in the first n_cols columns; sign and plane bits set outside exists as well"""
    S = np.zeros((depth + 2, 1 << 20), dtype=bool)
    S[0, :n_cols] = rng.random(n_cols) < density
    S[1:, :n_cols] = rng.random((depth + 1, n_cols)) < 0.5
    if depth:  # small magnitudes too: a third of the columns use only the low planes
        S[2 + depth // 2:, : n_cols // 3] = False
    return np.packbits(S, axis=1, bitorder="little").view(np.uint64).reshape(depth + 2, 16, 1024)


def _plant(S, depth, col, value):
    """column `col` holds `value` ("-0": a set sign over magnitude 0)"""
    w, b = divmod(col, 64)
    bit = np.uint64(1) << np.uint64(b)
    S[:, 0, w] &= ~bit
    S[0, 0, w] |= bit
    neg = value == "-0" or (value != "-0" and value < 0)
    mag = 0 if value == "-0" else abs(value)
    assert mag < 1 << depth or mag == 0
    if neg:
        S[1, 0, w] |= bit
    for i in range(depth):
        if (mag >> i) & 1:
            S[2 + i, 0, w] |= bit


def _planted(dx, dy):
    """(x, y) pairs for the first columns: -0 against 0 and -0, the largest magnitudes of both signs against each other, equal
    magnitudes of opposite sign"""
    bx, by = (1 << dx) - 1, (1 << dy) - 1
    e = min(bx, by)
    return [("-0", 0), (0, "-0"), ("-0", "-0"), (bx, by), (-bx, by), (bx, -by), (-bx, -by), (e, -e), (-e, e), (e, e), (-e, -e), ("-0", by), ("-0", -by), (bx, "-0"), (-bx, "-0")]


def _as_int(v):
    return 0 if v == "-0" else v


def _case(dx, dy, seed):
    rng = D.rng_for(9800, dx, dy, seed)
    n_cols = 2500
    Sx, Sy = _fragment(rng, dx, n_cols), _fragment(rng, dy, n_cols)
    if dx == dy and dx:  # equal values are otherwise rare: copy y's planes and sign into a stretch of x
        Sx[1:, 0, 8:12] = Sy[1:, 0, 8:12]
    pairs = _planted(dx, dy)
    for c, (vx, vy) in enumerate(pairs):
        _plant(Sx, dx, c, vx)
        _plant(Sy, dy, c, vy)
    assert M.values_at(Sx, dx, range(len(pairs))) == [_as_int(p[0]) for p in pairs]
    assert M.values_at(Sy, dy, range(len(pairs))) == [_as_int(p[1]) for p in pairs]
    F = _fragment(rng, 0, n_cols, 0.8)[0]
    F[0, 0] |= np.uint64((1 << len(pairs)) - 1)  # the planted columns pass the filter
    return Sx, Sy, F, pairs


def _check(model, want, what):
    lt, gt, E = model
    wl, wg, wE = want
    for op in CR.OPS:
        assert (CR.combine(op, lt, gt, E) == CR.words_of_bits(CR.combine(op, wl, wg, wE))).all(), (what, op)


@pytest.mark.parametrize("dx,dy", DEPTH_PAIRS)
def test_sign_magnitude_recurrence_equals_the_definition(dx, dy):
    Sx, Sy, F, pairs = _case(dx, dy, 0)
    for filt in (None, F):
        want = CR.definition(Sx, dx, 0, Sy, dy, 0, filt)
        assert want[2].sum() > 500
        if dx and dy:
            assert want[0].sum() > 50 and want[1].sum() > 50
        if dx == dy:
            assert (want[2] & ~want[0] & ~want[1]).sum() > 3  # equal columns exist
        _check(CR.sign_magnitude(Sx, dx, Sy, dy, filt), want, (dx, dy, filt is not None))
        # a base on both sides changes nothing, at the int64 extremes too
        assert all((a == b).all() for a, b in zip(CR.definition(Sx, dx, I64_MIN, Sy, dy, I64_MIN, filt), want))
    # the planted columns, by hand: -0 == 0 == -0
    lt, gt, E = CR.definition(Sx, dx, 0, Sy, dy, 0, None)
    for c, (vx, vy) in enumerate(pairs):
        assert E[c] and (bool(lt[c]), bool(gt[c])) == (_as_int(vx) < _as_int(vy), _as_int(vx) > _as_int(vy)), (c, vx, vy)


@pytest.mark.parametrize("dx,dy", DEPTH_PAIRS)
def test_general_recurrence_equals_the_definition(dx, dy):
    Sx, Sy, F, _ = _case(dx, dy, 1)
    big = (1 << 64) - 1
    for k in (0, 1, -1, 1 << dx, -(1 << dy), big, -big):  # 2^depth: a carry through every plane
        bx, by = _split_bases(k)
        for filt in (None, F):
            want = CR.definition(Sx, dx, bx, Sy, dy, by, filt)
            _check(CR.general(Sx, dx, Sy, dy, k, filt), want, (dx, dy, k, filt is not None))
            if k == 0:
                _check(CR.sign_magnitude(Sx, dx, Sy, dy, filt), want, (dx, dy, "sm"))
                assert CR.steps(dx, dy, 0) == max(dx, dy) and CR.steps(dx, dy, 0, CR.PATH_OFFSET) == max(dx, dy) + 2


def _split_bases(k):
    """int64 bases with base_x - base_y == k"""
    if -(1 << 63) <= k < 1 << 63:
        return (k, 0)
    return (I64_MAX, I64_MAX - k) if k > 0 else (I64_MIN, I64_MIN - k)


def test_split_bases_are_int64():
    for k in (0, 1, -1, 1 << 63, -(1 << 63) - 1, (1 << 64) - 1, -((1 << 64) - 1)):
        bx, by = _split_bases(k)
        assert bx - by == k and I64_MIN <= bx <= I64_MAX and I64_MIN <= by <= I64_MAX


def test_one_step_fewer_is_wrong():
    """the + 2 of W = max(depth_x, depth_y, bitlen |k|) + 2 is needed: with W - 1 steps a planted column wraps"""
    # depth 1, k = 1: X = 1 + 1 = 2 does not fit two bits of two's complement (it reads as -2 < 0); depth 2, k = -3: X = -3 - 3 = -6
    # does not fit three (it reads as 2 > 0)
    for depth, vx, k, want in ((1, 1, 1, (False, True)), (2, -3, -3, (True, False))):
        Sx, Sy = np.zeros((depth + 2, 16, 1024), dtype=np.uint64), np.zeros((depth + 2, 16, 1024), dtype=np.uint64)
        _plant(Sx, depth, 0, vx)
        _plant(Sy, depth, 0, 0)
        W = CR.steps(depth, depth, k)
        assert W == depth + 2
        lt, gt, E = CR.general(Sx, depth, Sy, depth, k)
        assert (bool(R_bit(lt, 0)), bool(R_bit(gt, 0))) == want
        d = CR.definition(Sx, depth, k, Sy, depth, 0)
        assert (bool(d[0][0]), bool(d[1][0])) == want
        lt1, gt1, _ = CR.general(Sx, depth, Sy, depth, k, width=W - 1)
        assert (bool(R_bit(lt1, 0)), bool(R_bit(gt1, 0))) == want[::-1], "W - 1 steps would do"
    # depth 64 at k = ±(2^64 - 1): 66 steps, 65 are too few for the largest magnitudes
    S64x, S64y = np.zeros((66, 16, 1024), dtype=np.uint64), np.zeros((66, 16, 1024), dtype=np.uint64)
    big = (1 << 64) - 1
    _plant(S64x, 64, 0, big)
    _plant(S64y, 64, 0, 0)
    lt, gt, _ = CR.general(S64x, 64, S64y, 64, big)
    assert CR.steps(64, 64, big) == 66 and (R_bit(lt, 0), R_bit(gt, 0)) == (0, 1)
    lt1, gt1, _ = CR.general(S64x, 64, S64y, 64, big, width=65)
    assert (R_bit(lt1, 0), R_bit(gt1, 0)) != (0, 1)


def R_bit(words, col):
    return int((int(words[col >> 16, (col & 0xFFFF) >> 6]) >> (col & 63)) & 1)
