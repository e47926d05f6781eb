"""Expected values of fbk_count_matrix_distinct (GroupBy with aggregate=Count(Distinct(field))) for the tests, two independent ways:

* numpy_expected: brute force from the bit words — per shard the columns of exists [∩ F], their signed int64 values and their
  A / B membership; per group the union of the value sets over the shards, from membership products per value;
* slow_expected: per group and shard the oracle's intersect A_i ∩ B_j [∩ F], then the value of every column of that set that
  exists, read bit by bit from the planes in Python integers; the distinct count of the union of those value sets.

Rows are [16, 1024] uint64 words (slot, word); BSI fragments [depth + 2, 16, 1024] (exists, sign, planes)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from msum_ref import bits


def values_of(S: np.ndarray, depth: int, cols: np.ndarray) -> np.ndarray:
    """[depth + 2, 16, 1024] -> int64 values of the columns given: sign ? -magnitude : magnitude, wrapping"""
    mag = np.zeros(cols.size, dtype=np.uint64)
    for k in range(depth):
        mag |= bits(S[2 + k])[cols].astype(np.uint64) << np.uint64(k)
    neg = bits(S[1])[cols]
    return np.where(neg, ~mag + np.uint64(1), mag).view(np.int64)


def numpy_expected(A: np.ndarray, Bw: Optional[np.ndarray], F: Optional[np.ndarray], S: np.ndarray, depth: int) -> Tuple[np.ndarray, np.ndarray]:
    """A [n_shards, n_a, 16, 1024], Bw [n_shards, n_b, 16, 1024] or None (one-field: n_b = 1), F [n_shards, 16, 1024] or None,
    S [n_shards, depth + 2, 16, 1024] -> (distinct uint64 [n_a, n_b], counts uint64 [n_a, n_b]).
    The columns of all shards side by side; a value held by one column adds that column's A x B membership, a value held by
    several adds (their membership products > 0): the union over the shards."""
    n_sh, n_a = A.shape[:2]
    n_b = Bw.shape[1] if Bw is not None else 1
    counts = np.zeros((n_a, n_b), dtype=np.uint64)
    a_all, b_all, v_all = [], [], []
    for s in range(n_sh):
        g = bits(S[s, 0])
        if F is not None:
            g &= bits(F[s])
        cols = np.nonzero(g)[0]
        if cols.size == 0:
            continue
        a = bits(A[s])[:, cols].astype(np.float64)
        b = bits(Bw[s])[:, cols].astype(np.float64) if Bw is not None else np.ones((1, cols.size))
        counts += np.rint(a @ b.T).astype(np.uint64)  # exact: at most 2^20 per shard
        a_all.append(a)
        b_all.append(b)
        v_all.append(values_of(S[s], depth, cols))
    if not v_all:
        return np.zeros((n_a, n_b), dtype=np.uint64), counts
    a, b, v = np.concatenate(a_all, axis=1), np.concatenate(b_all, axis=1), np.concatenate(v_all)
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    single = cnt[inv] == 1
    dist = np.rint(a[:, single] @ b[:, single].T).astype(np.uint64)
    multi = np.nonzero(~single)[0]
    multi = multi[np.argsort(inv[multi], kind="stable")]
    _, starts = np.unique(inv[multi], return_index=True)
    for lo, hi in zip(starts, list(starts[1:]) + [multi.size]):
        cv = multi[lo:hi]
        dist += (a[:, cv] @ b[:, cv].T > 0).astype(np.uint64)
    return dist, counts


def slow_expected(O, a_bms: Sequence[Sequence], b_bms: Optional[Sequence[Sequence]], f_bms: Optional[Sequence], S: np.ndarray, depth: int,
                  pairs: Sequence[Tuple[int, int]]) -> Dict[Tuple[int, int], Tuple[int, int]]:
    """a_bms[s][i] / b_bms[s][j] / f_bms[s] oracle OBitmaps (None: no container in that row), S as numpy_expected.  b_bms None:
    the one-field form (j = 0).  Returns {(i, j): (distinct, count)}."""
    out = {}
    for (i, j) in pairs:
        seen, cnt = set(), 0
        for s in range(S.shape[0]):
            x = a_bms[s][i]
            if x is not None and b_bms is not None:
                x = x.intersect(b_bms[s][j]) if b_bms[s][j] is not None else None
            if x is not None and f_bms is not None:
                x = x.intersect(f_bms[s]) if f_bms[s] is not None else None
            if x is None:
                continue
            for c in x.slice():
                sl, wd, bt = c >> 16, (c >> 6) & 1023, c & 63
                if not (int(S[s, 0, sl, wd]) >> bt) & 1:
                    continue
                mag = sum(((int(S[s, 2 + k, sl, wd]) >> bt) & 1) << k for k in range(depth))
                v = -mag if (int(S[s, 1, sl, wd]) >> bt) & 1 else mag
                seen.add(((v + (1 << 63)) % (1 << 64)) - (1 << 63))  # int64 wrap-around
                cnt += 1
        out[(i, j)] = (len(seen), cnt)
    return out
