"""Expected values of fbk_count_matrix_quantiles (GroupBy with a percentile of an int field per group) for the tests: the numpy model.

* disc_rank(): SQL's PERCENTILE_DISC(num / den) over N values as an ascending rank, max(1, ceil(N * num / den)) - 1, in Python
  integers.
* numpy_expected(): per group the values of pct_ref.values (the columns of exists ∩ F, stored zeros included, sign over magnitude 0
  the value 0, int64 wrap-around) restricted to the group's columns A_i ∩ B_j, sorted as int64, the value at the rank of every
  request and the number of the group's columns holding exactly it.  An empty group is (0, 0) with total 0.
* plan_check(): featurebase_amd/csrc/fbk_group_quantile_plan.h compiled into a stand-alone program (tests/cpp/gquant_plan_check.cpp).

Rows are [16, 1024] uint64 words (slot, word); BSI fragments [depth + 2, 16, 1024] (exists, sign, planes)."""
from __future__ import annotations

import os
import subprocess
from typing import List, Optional, Sequence, Tuple

import numpy as np

import pct_ref as P
from msum_ref import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_check(lines: Sequence[str]) -> List[List[int]]:
    """the plan header's answers to `lines` (-fsanitize=address,undefined, run as a program like the other *_plan_check)"""
    out = os.path.join(ROOT, "build", "gquant_plan_check_san")
    src = os.path.join(ROOT, "tests", "cpp", "gquant_plan_check.cpp")
    hdr = os.path.join(ROOT, "featurebase_amd", "csrc", "fbk_group_quantile_plan.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out])
    r = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"gquant_plan_check exit {r.returncode}\n{r.stderr[-4000:]}"
    got = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


def plan_constants() -> dict:
    """the constants the library was built with"""
    k = plan_check(["K"])[0]
    return dict(zip(("lds_digit", "global_digit", "lds_cap", "auto_pairs", "scratch_bound", "max_den", "max_requests"), k))


def disc_rank(n: int, num: int, den: int) -> int:
    assert n >= 1 and 1 <= den and 0 <= num <= den
    return max(1, -(-(n * num) // den)) - 1


def numpy_expected(A: np.ndarray, Bw: Optional[np.ndarray], F: Optional[np.ndarray], S: np.ndarray, depth: int,
                   fractions: Sequence[Tuple[int, int]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A [n_shards, n_a, 16, 1024], Bw [n_shards, n_b, 16, 1024] or None (one-field: n_b = 1), F [n_shards, 16, 1024] or None,
    S [n_shards, depth + 2, 16, 1024], fractions [(num, den)] -> (values int64 [n_a, n_b, n_q], counts uint64 [n_a, n_b, n_q],
    totals uint64 [n_a, n_b])"""
    n_sh, n_a = A.shape[:2]
    n_b = Bw.shape[1] if Bw is not None else 1
    n_q = len(fractions)
    vals, cnts = np.zeros((n_a, n_b, n_q), dtype=np.int64), np.zeros((n_a, n_b, n_q), dtype=np.uint64)
    totals = np.zeros((n_a, n_b), dtype=np.uint64)
    v = P.values(S, F, depth)  # (shard, column) order
    a_all, b_all = [], []
    for s in range(n_sh):
        g = bits(S[s, 0])
        if F is not None:
            g &= bits(F[s])
        cols = np.nonzero(g)[0]
        a_all.append(bits(A[s])[:, cols])
        b_all.append(bits(Bw[s])[:, cols] if Bw is not None else np.ones((1, cols.size), dtype=bool))
    a, b = np.concatenate(a_all, axis=1), np.concatenate(b_all, axis=1)
    assert a.shape[1] == v.size
    for i in range(n_a):
        ci = np.nonzero(a[i])[0]
        if ci.size == 0:
            continue
        vi, bi = v[ci], b[:, ci]
        for j in range(n_b):
            s = np.sort(vi[bi[j]])
            n = int(s.size)
            totals[i, j] = n
            for q, (num, den) in enumerate(fractions if n else ()):
                x = s[disc_rank(n, int(num), int(den))]
                vals[i, j, q] = x
                cnts[i, j, q] = np.searchsorted(s, x, side="right") - np.searchsorted(s, x, side="left")
    return vals, cnts, totals
