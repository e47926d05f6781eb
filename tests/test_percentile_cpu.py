"""fbk_bsi_quantiles / fbk_bsi_percentile without a device: the ABI is declared and bound, bad arguments are errors (not crashes), and
the replay from four order statistics (tests/pct_ref.py percentile_replay — what the device call does) equals the reference's search
loop restated (percentile_search — the yardstick of the GPU tests) on seeded inputs that take every exit of the loop, and on the
100-value data set of the Percentile block of tests/cpp/test_executor_api.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as D
import pct_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
FUNCS = ["fbk_bsi_quantiles", "fbk_bsi_percentile"]
NTHS = [0, 100, 50, 25, 75, 99, 1, 0.1, 99.9, 33.3]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


def test_signatures_declared_and_exported(lib):
    l = lib.load()
    for f in FUNCS:
        assert f in lib.SIGNATURES and getattr(l, f) is not None, f
    assert [len(lib.SIGNATURES[f][1]) for f in FUNCS] == [12, 13]
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for f in FUNCS:
        assert f" T {f}\n" in out, f
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "fbk.h")).read()
    assert "#define FBK_RANK_FROM_TOP (1ull << 63)" in hdr
    assert lib.RANK_FROM_TOP == P.RANK_FROM_TOP == 1 << 63
    from featurebase_amd.roaring import Context

    assert callable(Context.bsi_quantiles) and callable(Context.bsi_percentile)


def test_bad_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    tot = C.c_uint64(7)
    rows = np.zeros(4, dtype=np.uint32)
    ranks = np.zeros(1025, dtype=np.uint64)
    nth = np.full(257, 50.0)
    vals, cnts = np.zeros(1025, dtype=np.int64), np.zeros(1025, dtype=np.uint64)

    def err():
        return l.fbk_last_error(None).decode()

    def quant(depth=8, base=rows.ctypes.data, n_sh=1, rk=ranks.ctypes.data, n=3, ov=vals.ctypes.data, oc=cnts.ctypes.data, ot=C.byref(tot)):
        return l.fbk_bsi_quantiles(None, None, base, depth, None, None, n_sh, rk, n, ov, oc, ot)

    def pct(depth=8, base=rows.ctypes.data, n_sh=1, pn=nth.ctypes.data, n=3, ov=vals.ctypes.data, oc=cnts.ctypes.data, ot=C.byref(tot)):
        return l.fbk_bsi_percentile(None, None, base, depth, None, None, n_sh, 0, pn, n, ov, oc, ot)

    assert l.fbk_bsi_quantiles(None, None, None, 0, None, None, 0, None, 0, None, None, None) == lib.FBK_E_INVALID
    assert l.fbk_bsi_percentile(None, None, None, 0, None, None, 0, 0, None, 0, None, None, None) == lib.FBK_E_INVALID
    for call in (quant, pct):
        assert call(ot=None) == lib.FBK_E_INVALID and "NULL" in err()
        assert call(ov=None) == lib.FBK_E_INVALID and "NULL" in err()
        assert call(oc=None) == lib.FBK_E_INVALID and "NULL" in err()
        assert call(depth=65) == lib.FBK_E_INVALID and "bit depth" in err()
        assert call(base=None) == lib.FBK_E_INVALID and "NULL" in err()
        tot.value = 7
        assert call() == lib.FBK_E_INVALID and "NULL" in err()  # ctx == NULL; the total is reset before anything else
        assert tot.value == 0
        assert call(depth=64) == lib.FBK_E_INVALID
    assert quant(rk=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert quant(n=1025) == lib.FBK_E_INVALID and "1024" in err()
    assert quant(n=1024) == lib.FBK_E_INVALID and "NULL" in err()  # (the count is fine: the context is what is missing)
    assert pct(pn=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert pct(n=257) == lib.FBK_E_INVALID and "256" in err()
    assert pct(n=256) == lib.FBK_E_INVALID and "NULL" in err()
    for bad in (101.0, -0.5, float("nan"), float("inf")):
        one = np.array([50.0, bad, 10.0])
        assert pct(pn=one.ctypes.data) == lib.FBK_E_INVALID and "nth" in err(), bad


def _inputs(rng, kind, n):
    if kind == "ties":
        return rng.integers(-3, 4, n, dtype=np.int64)
    if kind == "full":
        return rng.integers(P.I64_MIN, P.I64_MAX, n, dtype=np.int64, endpoint=True)
    centre = int(rng.integers(-(1 << 40), 1 << 40))  # clustered: a few narrow clumps far apart
    clumps = centre + rng.integers(-5, 6, 3) * (1 << 30)
    return (clumps[rng.integers(0, 3, n)] + rng.integers(-50, 51, n)).astype(np.int64)


def _base_for(rng, kind):
    if kind == "full":
        return 0  # value + base has to stay inside int64
    return int(rng.choice([0, -1000, 12345, -(1 << 50), 1 << 50, int(rng.integers(-(1 << 20), 1 << 20))]))


def test_replay_from_four_order_statistics_equals_the_search_loop():
    rng = D.rng_for(9950)
    exits = {"min": 0, "max": 0, "balanced": 0, "bounds": 0}
    per_kind = {}
    cases = 0
    for kind in ("ties", "full", "clustered"):
        mine = dict.fromkeys(exits, 0)
        for _ in range(7000):
            n = int(rng.integers(1, 201))
            v = _inputs(rng, kind, n)
            base = _base_for(rng, kind)
            nth = float(rng.choice(NTHS)) if rng.random() < 0.6 else float(rng.uniform(0, 100))
            want = P.percentile_search(v, nth, base)
            got = P.replay_on(v, nth, base)
            assert got == want, (kind, n, nth, base, got, want)
            mine[want[2]] += 1
            cases += 1
        per_kind[kind] = mine
        for k, c in mine.items():
            exits[k] += c
    print("exits", exits, per_kind)
    assert cases >= 20000
    for k, c in exits.items():  # a condition on the inputs: every branch of the loop is exercised
        assert c >= 0.05 * cases, (k, c, cases)


def test_quantiles_yardstick_on_a_small_example():
    v = np.array([5, -2, 5, 0, 7, -2, 5], dtype=np.int64)
    T = P.RANK_FROM_TOP
    vals, cnts, n = P.quantiles(v, [0, 1, 2, 3, 6, 7, T | 0, T | 1, T | 6, T | 7, 3])
    assert n == 7
    assert vals.tolist() == [-2, -2, 0, 5, 7, 0, 7, 5, -2, 0, 5]
    assert cnts.tolist() == [2, 2, 1, 3, 1, 0, 1, 3, 2, 0, 3]
    assert P.percentile_search(np.zeros(0, dtype=np.int64), 50) is None and P.replay_on(np.zeros(0, dtype=np.int64), 50) is None
    assert P.midpoint(-7, -3) == -5 and P.midpoint(-7, 4) == -1 and P.midpoint(3, 5) == 4 and P.midpoint(P.I64_MIN, P.I64_MAX) == -1


def test_executor_api_percentile_block_expectations():
    """the data set of tests/cpp/test_executor_api.cpp (splitmix64 from seed 42: 100 values of +-uint32, a coin flip for "foo"): the
    program's `exec` is percentile_search; its `checker` (the reference test's getExpectedPercentile) agrees whenever the search
    ends balanced, which the program requires of at least 8 of its 16 cases"""
    M = (1 << 64) - 1
    seed = 42

    def rnd():
        nonlocal seed
        seed = (seed + 0x9E3779B97F4A7C15) & M
        z = seed
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    foo, rest = [], []
    for _ in range(100):
        num = rnd() & 0xFFFFFFFF
        if rnd() % 2 == 0:
            num = -num
        (foo if rnd() % 2 == 0 else rest).append(num)
    every = rest + foo
    assert len(every) == 100 and 20 < len(foo) < 80

    def checker(nums, nth):
        mn, mx = min(nums), max(nums)
        if nth == 0.0:
            return mn, True
        if nth == 100.0:
            return mx, True
        less, greater = P.desired(len(nums), nth)
        if less == 0:
            return mn, True
        if greater == 0:
            return mx, True
        while mn < mx:
            guess = P.midpoint(mx, mn)
            l, r = sum(v < guess for v in nums), sum(v > guess for v in nums)
            if l > less:
                mx = guess - 1
            elif r > greater:
                mn = guess + 1
            else:
                return guess, True
        return mn, False

    balanced = 0
    for nth in (0.0, 10.0, 25.0, 50.0, 75.0, 90.0, 99.0, 100.0):
        for nums in (foo, every):
            v = np.array(nums, dtype=np.int64)
            want = P.percentile_search(v, nth)
            assert P.replay_on(v, nth) == want and want[1] >= 1
            chk, bal = checker(nums, nth)
            if bal:
                assert want[0] == chk
                balanced += 1
    assert balanced >= 8
