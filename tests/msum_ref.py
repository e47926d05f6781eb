"""Expected values of fbk_count_matrix_sum (GroupBy with aggregate=Sum) for the tests, two independent ways:

* oracle_expected: the reference's composition — per shard and pair the filter X = A_i ∩ B_j [∩ F] (oracle intersect), then
  the oracle's BSI Sum over that filter (executeSumCountShard), summed over the shards in uint64 wrap-around;
* numpy_expected: brute force from the bit words — the signed value of every column of exists [∩ F] as uint64, the pair sums
  as integer matrix products over those columns, 16 bits of the value at a time (exact), wrapped to 64 bits.

Rows are [16, 1024] uint64 words (slot, word); BSI fragments [depth + 2, 16, 1024] (exists, sign, planes)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MASK64 = (1 << 64) - 1


def bits(words: np.ndarray) -> np.ndarray:
    """[..., 16, 1024] uint64 -> [..., 2^20] bool, column c = slot * 65536 + word * 64 + bit"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    lead = w.shape[:-2]
    return np.unpackbits(w.view(np.uint8).reshape(*lead, -1), bitorder="little").reshape(*lead, 1 << 20).astype(bool)


def words_of_bitmap(bm) -> np.ndarray:
    """oracle OBitmap (container keys: slot = key & 15) or None -> [16, 1024] uint64"""
    w = np.zeros((16, 1024), dtype=np.uint64)
    if bm is not None:
        for k, c in bm.items():
            if c.n:
                w[k & 15] = c.words()
    return w


def words_of_row(row) -> np.ndarray:
    """{key: oracle container} (slot = key & 15) -> [16, 1024] uint64"""
    w = np.zeros((16, 1024), dtype=np.uint64)
    for k, c in row.items():
        if c.n:
            w[k & 15] = c.words()
    return w


def numpy_expected(A: np.ndarray, Bw: Optional[np.ndarray], F: Optional[np.ndarray], S: np.ndarray, depth: int) -> Tuple[np.ndarray, np.ndarray]:
    """A [n_shards, n_a, 16, 1024], Bw [n_shards, n_b, 16, 1024] or None (one-field: n_b = 1), F [n_shards, 16, 1024] or None,
    S [n_shards, depth + 2, 16, 1024] -> (sums int64 [n_a, n_b], counts uint64 [n_a, n_b])"""
    n_sh, n_a = A.shape[:2]
    n_b = Bw.shape[1] if Bw is not None else 1
    sums = np.zeros((n_a, n_b), dtype=np.uint64)
    counts = np.zeros((n_a, n_b), dtype=np.uint64)
    for s in range(n_sh):
        g = bits(S[s, 0])
        if F is not None:
            g &= bits(F[s])
        cols = np.nonzero(g)[0]
        if cols.size == 0:
            continue
        a = bits(A[s])[:, cols].astype(np.int64)
        b = bits(Bw[s])[:, cols].astype(np.int64) if Bw is not None else np.ones((1, cols.size), dtype=np.int64)
        mag = np.zeros(cols.size, dtype=np.uint64)
        for k in range(depth):
            mag |= bits(S[s, 2 + k])[cols].astype(np.uint64) << np.uint64(k)
        neg = bits(S[s, 1])[cols]
        val = np.where(neg, ~mag + np.uint64(1), mag)
        counts += (a @ b.T).astype(np.uint64)
        for q in range(4):
            vq = ((val >> np.uint64(16 * q)) & np.uint64(0xFFFF)).astype(np.int64)
            part = (a @ (b * vq).T).astype(np.uint64)  # exact: at most 2^20 * 65535 per pair
            sums += part << np.uint64(16 * q)
    return sums.view(np.int64), counts


def oracle_expected(O, B, a_bms: Sequence[Sequence], b_bms: Optional[Sequence[Sequence]], f_bms: Optional[Sequence], frags: Sequence,
                    pairs: Sequence[Tuple[int, int]]) -> Dict[Tuple[int, int], Tuple[int, int]]:
    """The reference's composition for the given (i, j) pairs: a_bms[s][i] / b_bms[s][j] / f_bms[s] oracle OBitmaps (None: no
    container anywhere in that row), frags[s] a pybsi.Fragment.  b_bms None: the one-field form (j = 0).
    Returns {(i, j): (sum as int64, count)}."""
    out = {}
    for (i, j) in pairs:
        tot, cnt = 0, 0
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
            sm, c = B.bsi_sum(frags[s], x, True)
            tot = (tot + sm) & MASK64
            cnt += c
        out[(i, j)] = (tot - (1 << 64) if tot >> 63 else tot, cnt)
    return out


def bitmap_of_words(O, w: np.ndarray):
    """[16, 1024] uint64 -> oracle OBitmap of bitmap containers (None when empty)"""
    items = [(sl, O.OContainer.bitmap(w[sl])) for sl in range(16) if w[sl].any()]
    return O.OBitmap.from_containers(items) if items else None


def fragment_of_words(O, B, S: np.ndarray):
    """[depth + 2, 16, 1024] -> pybsi.Fragment"""
    return B.Fragment([bitmap_of_words(O, S[r]) for r in range(S.shape[0])])
