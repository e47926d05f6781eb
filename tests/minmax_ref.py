"""Expected values of fbk_count_matrix_minmax (GroupBy with Min / Max of an int field per group) for the tests, two independent ways:

* numpy_expected: brute force from the bit words — every column of exists [∩ F] of every shard with its class (negative: sign set
  and magnitude != 0) and its magnitude as uint64, ordered by (class, magnitude) as mathematical integers, never by the wrapped
  int64; per group the smallest and the largest of its columns and how many columns hold each; an empty group is
  (INT64_MAX, INT64_MIN, 0, 0);
* oracle_expected: the reference's composition for sampled pairs — per shard the oracle's intersect A_i ∩ B_j [∩ F], then
  oracle/pybsi.py's bsi_min / bsi_max (fragment.min / fragment.max) over that filter, folded over the shards by ValCount.Smaller /
  Larger transcribed from executor.go:8446-8548.  That fold compares int64 values, so it is the mathematical order only while no
  selected magnitude reaches 2^63; and the reference counts a sign bit over magnitude 0 apart from +0.  Callers compare the two
  ways on data without either.

Rows are [16, 1024] uint64 words (slot, word); BSI fragments [depth + 2, 16, 1024] (exists, sign, planes)."""
from __future__ import annotations

import os
import subprocess
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from msum_ref import bits, bitmap_of_words, fragment_of_words  # noqa: F401  (re-exported for the tests)

INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_check(lines: Sequence[str]) -> List[List[int]]:
    """featurebase_amd/csrc/fbk_minmax_plan.h compiled into a stand-alone program (tests/cpp/minmax_plan_check.cpp,
    -fsanitize=address,undefined, run as a program the way the other test_*_plan_cpu.py run theirs): its answers to `lines`"""
    out = os.path.join(ROOT, "build", "minmax_plan_check_san")
    src = os.path.join(ROOT, "tests", "cpp", "minmax_plan_check.cpp")
    hdr = os.path.join(ROOT, "featurebase_amd", "csrc", "fbk_minmax_plan.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out])
    r = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"minmax_plan_check exit {r.returncode}\n{r.stderr[-4000:]}"
    got = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


def plan_constants() -> Tuple[int, int]:
    """(kMinmaxDescentCells, kMinmaxDescentMaxCells) as the library was built with them"""
    k = plan_check(["K"])[0]
    return k[0], k[1]


def numpy_expected(A: np.ndarray, Bw: Optional[np.ndarray], F: Optional[np.ndarray], S: np.ndarray, depth: int):
    """A [n_shards, n_a, 16, 1024], Bw [n_shards, n_b, 16, 1024] or None (one-field: n_b = 1), F [n_shards, 16, 1024] or None,
    S [n_shards, depth + 2, 16, 1024] -> (mins int64, maxs int64, min_counts uint64, max_counts uint64), all [n_a, n_b]"""
    n_sh, n_a = A.shape[:2]
    n_b = Bw.shape[1] if Bw is not None else 1
    mins = np.full((n_a, n_b), INT64_MAX, dtype=np.int64)
    maxs = np.full((n_a, n_b), INT64_MIN, dtype=np.int64)
    cmin, cmax = np.zeros((n_a, n_b), dtype=np.uint64), np.zeros((n_a, n_b), dtype=np.uint64)
    a_all, b_all, neg_all, mag_all = [], [], [], []
    for s in range(n_sh):
        g = bits(S[s, 0])
        if F is not None:
            g &= bits(F[s])
        cols = np.nonzero(g)[0]
        if cols.size == 0:
            continue
        mag = np.zeros(cols.size, dtype=np.uint64)
        for k in range(depth):
            mag |= bits(S[s, 2 + k])[cols].astype(np.uint64) << np.uint64(k)
        a_all.append(bits(A[s])[:, cols])
        b_all.append(bits(Bw[s])[:, cols] if Bw is not None else np.ones((1, cols.size), dtype=bool))
        neg_all.append(bits(S[s, 1])[cols] & (mag != 0))
        mag_all.append(mag)
    if not mag_all:
        return mins, maxs, cmin, cmax
    a, b = np.concatenate(a_all, axis=1), np.concatenate(b_all, axis=1)
    neg, mag = np.concatenate(neg_all), np.concatenate(mag_all)
    # the rank of every column's value among the distinct values, ascending: the negatives by falling magnitude, then the others
    cls, sub = (~neg).astype(np.uint8), np.where(neg, ~mag, mag)
    order = np.lexsort((sub, cls))
    step = (cls[order][1:] != cls[order][:-1]) | (sub[order][1:] != sub[order][:-1])
    rank = np.empty(mag.size, dtype=np.int64)
    rank[order] = np.concatenate([[0], np.cumsum(step)])
    n_ranks = int(rank.max()) + 1
    value = np.zeros(n_ranks, dtype=np.uint64)
    value[rank] = np.where(neg, ~mag + np.uint64(1), mag)  # int64 with wrap-around
    value = value.view(np.int64)
    for i in range(n_a):
        ci = np.nonzero(a[i])[0]
        if ci.size == 0:
            continue
        bi, ri = b[:, ci], rank[ci]
        lo = np.where(bi, ri, n_ranks).min(axis=1)
        hi = np.where(bi, ri, -1).max(axis=1)
        some = hi >= 0
        mins[i, some], maxs[i, some] = value[lo[some]], value[hi[some]]
        cmin[i] = np.where(some, (bi & (ri == lo[:, None])).sum(axis=1), 0)
        cmax[i] = np.where(some, (bi & (ri == hi[:, None])).sum(axis=1), 0)
    return mins, maxs, cmin, cmax


def smaller(a: Tuple[int, int], b: Tuple[int, int]) -> Tuple[int, int]:
    """ValCount.Smaller (executor.go:8446-8468) on (Val, Count)"""
    if a[1] == 0 or (b[0] < a[0] and b[1] > 0):
        return b
    return (a[0], a[1] + (b[1] if a[0] == b[0] else 0))


def larger(a: Tuple[int, int], b: Tuple[int, int]) -> Tuple[int, int]:
    """ValCount.Larger (executor.go:8526-8548)"""
    if a[1] == 0 or (b[0] > a[0] and b[1] > 0):
        return b
    return (a[0], a[1] + (b[1] if a[0] == b[0] else 0))


def oracle_expected(O, B, a_bms: Sequence[Sequence], b_bms: Optional[Sequence[Sequence]], f_bms: Optional[Sequence], frags: Sequence, depth: int,
                    pairs: Sequence[Tuple[int, int]]) -> Dict[Tuple[int, int], Tuple[int, int, int, int]]:
    """The reference's composition for the given (i, j) pairs: a_bms[s][i] / b_bms[s][j] / f_bms[s] oracle OBitmaps (None: no
    container anywhere in that row), frags[s] a pybsi.Fragment.  b_bms None: the one-field form (j = 0).
    Returns {(i, j): (min, max, min_count, max_count)}, an empty group as the sentinels."""
    out = {}
    for (i, j) in pairs:
        mn, mx = (0, 0), (0, 0)
        for s in range(len(frags)):
            x = a_bms[s][i]
            if x is None:
                continue
            if b_bms is not None:
                y = b_bms[s][j]
                if y is None:
                    continue
                x = x.intersect(y)
            if f_bms is not None:
                if f_bms[s] is None:
                    continue
                x = x.intersect(f_bms[s])
            mn = smaller(mn, B.bsi_min(frags[s], x, depth))
            mx = larger(mx, B.bsi_max(frags[s], x, depth))
        out[(i, j)] = (mn[0] if mn[1] else INT64_MAX, mx[0] if mx[1] else INT64_MIN, mn[1], mx[1])
    return out
