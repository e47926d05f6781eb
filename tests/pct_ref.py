"""Expected values of fbk_bsi_quantiles and fbk_bsi_percentile for the tests.

* values(): the stored values of the columns of exists ∩ filter from dense planes (extract_ref.select / bsi_expected), stored zeros
  included: every such column takes part.
* quantiles(): order statistics by np.sort; `RANK_FROM_TOP | k` counts from the largest; a rank past the end is (0, 0).
* percentile_search(): the loop of executePercentile (executor.go:1404-1585) restated with Go's integer semantics (truncating / and
  %), counting the values < guess and > guess over the whole array in every iteration.  It is the yardstick, and reports which exit it
  took: "min", "max" (the early returns), "balanced" (the break) or "bounds" (lo < hi stopped holding).
* percentile_replay(): the same loop driven by four order statistics — "leftCount > desiredLess" holds exactly when s[L] < guess,
  "rightCount > desiredGreater" exactly when s[N-1-G] > guess — which is what the device call does.

Python floats are IEEE doubles, Python ints do not overflow; int64 range is asserted where Go would wrap."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

import extract_ref as X

RANK_FROM_TOP = 1 << 63
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def values(S: np.ndarray, F: Optional[np.ndarray], depth: int) -> np.ndarray:
    """S [n_shards, depth + 2, 16, 1024], F [n_shards, 16, 1024] or None -> int64 values of exists ∩ filter (shard, column order)"""
    if S.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    consider = S[:, 0] if F is None else S[:, 0] & F
    sh, pos, _ = X.select(consider, list(range(S.shape[0])))
    vals, pres = X.bsi_expected(S, depth, sh, pos)
    assert pres.all()
    return vals


def quantiles(vals: np.ndarray, ranks: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, int]:
    """(values int64, counts uint64, N) for the ranks (k, or RANK_FROM_TOP | k)"""
    s = np.sort(np.asarray(vals, dtype=np.int64))
    n = int(s.size)
    out_v, out_c = np.zeros(len(ranks), dtype=np.int64), np.zeros(len(ranks), dtype=np.uint64)
    for i, r in enumerate(ranks):
        r = int(r)
        k = r & ~RANK_FROM_TOP
        if k >= n:
            continue
        at = n - 1 - k if r & RANK_FROM_TOP else k
        out_v[i] = s[at]
        out_c[i] = np.searchsorted(s, s[at], side="right") - np.searchsorted(s, s[at], side="left")
    return out_v, out_c, n


def _tdiv(a: int, b: int) -> int:
    """Go's (and C's) integer division: truncates toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _tmod(a: int, b: int) -> int:
    return a - b * _tdiv(a, b)


def midpoint(lo: int, hi: int) -> int:
    """executor.go:1498"""
    return _tdiv(lo, 2) + _tdiv(hi, 2) + _tdiv(_tmod(lo, 2) + _tmod(hi, 2), 2)


def desired(n: int, nth: float) -> Tuple[int, int]:
    """desiredLess, desiredGreater (executor.go:1408-1409)"""
    less = float(n) * nth
    less = less / 100.0
    more = float(n) * (100 - nth)
    more = more / 100.0
    return int(less), int(more)


def percentile_search(vals: np.ndarray, nth: float, base: int = 0) -> Optional[Tuple[int, int, str]]:
    """(value + base, count, exit), or None for the median of nothing"""
    v = np.asarray(vals, dtype=np.int64)
    n = int(v.size)
    if n == 0:
        return None
    L, G = desired(n, nth)
    mn, mx = int(v.min()), int(v.max())
    assert I64_MIN <= mn + base and mx + base <= I64_MAX
    if G != 0 and L == 0:
        return mn + base, int((v == mn).sum()), "min"
    if G == 0:
        return mx + base, int((v == mx).sum()), "max"
    lo, hi = mn + base, mx + base
    guess = lo
    while lo < hi:
        guess = midpoint(lo, hi)
        g = guess - base  # in [mn, mx]: compared with the stored values, so that nothing leaves int64
        assert mn <= g <= mx
        if int((v < g).sum()) > L:
            hi = guess - 1
            continue
        if int((v > g).sum()) > G:
            lo = guess + 1
            continue
        return guess, 1, "balanced"
    return guess, 1, "bounds"


def percentile_replay(mn: int, mx: int, a: Optional[int], b: Optional[int], n: int, nth: float) -> Tuple[int, str]:
    """(value, exit) from mn = s[0], mx = s[N-1], a = s[L], b = s[N-1-G] (Base already added; a / b None where L / G is not below N)"""
    L, G = desired(n, nth)
    if G != 0 and L == 0:
        return mn, "min"
    if G == 0:
        return mx, "max"
    lo, hi, guess = mn, mx, mn
    while lo < hi:
        guess = midpoint(lo, hi)
        if a is not None and a < guess:
            hi = guess - 1
            continue
        if b is not None and b > guess:
            lo = guess + 1
            continue
        return guess, "balanced"
    return guess, "bounds"


def replay_on(vals: np.ndarray, nth: float, base: int = 0) -> Optional[Tuple[int, int, str]]:
    """percentile_replay fed from np.sort: the same triple as percentile_search"""
    s = np.sort(np.asarray(vals, dtype=np.int64))
    n = int(s.size)
    if n == 0:
        return None
    L, G = desired(n, nth)
    mn, mx = int(s[0]) + base, int(s[-1]) + base
    a = int(s[L]) + base if L < n else None
    b = int(s[n - 1 - G]) + base if G < n else None
    val, how = percentile_replay(mn, mx, a, b, n, nth)
    cnt = int((s == s[0]).sum()) if how == "min" else int((s == s[-1]).sum()) if how == "max" else 1
    return val, cnt, how
