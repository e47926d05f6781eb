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


# ---- a call of 19 shards over 5 stored ones (tests/test_gpu_count_matrix_minmax.py: launches that go round their loops) -----------
# Shard s reads the set-field and filter rows of stored shard MANY_ROWS[s] and the fragment MANY_FRAG[s].  Fragments 0 .. 2 lack
# their top 3, 2, 1 planes and serve the first 8 shards only (one round of the grid of k_minmax_scatter / _holders and of a one-tile
# k_minmax_descent); fragments 3 and 4 have every plane and serve shards 8 .. 18 in ten different pairings with the stored rows (shard
# 18 repeats shard 8).  So the extremes of a group lie beyond the first round, and a shard that a later round skipped or read twice
# shows in the values or, where another shard holds the same extreme, in the counts.
MANY_SHARDS, MANY_STORED = 19, 5
MANY_ROWS = [s % MANY_STORED for s in range(MANY_SHARDS)]
MANY_FRAG = [0, 1, 2, 0, 1, 2, 0, 1] + [3, 4] * 5 + [3]


def many_shard_case(n_a: int, n_b: Optional[int], depth: int):
    """the stored words (A [5, n_a, 16, 1024], Bw [5, n_b, 16, 1024] or None with n_b None: the one-field form, F [5, 16, 1024],
    S [5, depth + 2, 16, 1024]): random rows, exists one column in 128, sign and plane bits also outside exists"""
    import datagen as D

    rng = D.rng_for(8950, n_a, n_b or 0, depth)

    def rnd(shape, ands=0):
        w = rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
        for _ in range(ands):
            w &= rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
        return w

    A = rnd((MANY_STORED, n_a, 16, 1024))
    Bw = rnd((MANY_STORED, n_b, 16, 1024)) if n_b else None
    F = rnd((MANY_STORED, 16, 1024))
    S = rnd((MANY_STORED, depth + 2, 16, 1024))
    S[:, 0] &= rnd((MANY_STORED, 16, 1024), 6)
    A[0, 0, 3] = 0  # an empty container in a row
    for k in range(3):
        S[k, 2 + depth - (3 - k):] = 0
    # fragments 3 and 4: a column whose top 9 planes are all set gets every plane set (about 16 columns of a fragment's 8192).  The
    # largest magnitude then sits on several columns of every later shard, and a group's tie count takes part from each of them
    top = min(9, depth)
    S[3:, 2:2 + depth - top] |= np.bitwise_and.reduce(S[3:, 2 + depth - top:2 + depth], axis=1)[:, None]
    return A, Bw, F, S


def many_shard_lists(n_a: int, n_b: Optional[int], depth: int):
    """(rows_a [19, n_a], rows_b [19, n_b] or None, rows_f [19], base_rows [19]) into dense uploads of many_shard_case's words"""
    rows, frag = np.array(MANY_ROWS, dtype=np.uint32), np.array(MANY_FRAG, dtype=np.uint32)
    ra = rows[:, None] * np.uint32(n_a) + np.arange(n_a, dtype=np.uint32)[None, :]
    rb = rows[:, None] * np.uint32(n_b) + np.arange(n_b, dtype=np.uint32)[None, :] if n_b else None
    return ra, rb, rows.copy(), frag * np.uint32(depth + 2)


def many_shard_words(A, Bw, F, S, shards: Optional[Sequence[int]] = None):
    """the words the given shards of the call read (all 19: None), as numpy_expected takes them"""
    sh = list(range(MANY_SHARDS)) if shards is None else list(shards)
    r, f = [MANY_ROWS[s] for s in sh], [MANY_FRAG[s] for s in sh]
    return A[r], (Bw[r] if Bw is not None else None), F[r], S[f]


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
