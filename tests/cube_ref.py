"""Expected values of fbk_count_cube (GroupBy over three fields) for the tests, two independent ways:

* numpy_expected: brute force from the bit words — popcount(P_p & A_i & B_j & F) per shard, summed over the shards;
* oracle_expected: the reference's composition for three levels — rows[0] ∩= filter, rows[1] ∩= rows[0],
  rows[2].intersectionCount(rows[1]) with the oracle's bitmaps, the per-shard counts added up.

and `chunk`, the densify chunk of a call as include/fbk.h documents it.  Rows are [16, 1024] uint64 words (slot, word)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

PT = 8  # k_cube_mfma's P rows per block (a leading field of at most 4 rows runs the 4-row form)


def numpy_expected(P: np.ndarray, A: np.ndarray, B: np.ndarray, F: Optional[np.ndarray]) -> np.ndarray:
    """P [n_shards, n_p, 16, 1024], A [n_shards, n_a, 16, 1024], B [n_shards, n_b, 16, 1024], F [n_shards, 16, 1024] or None
    -> uint64 [n_p, n_a, n_b].  Slots in which one of the operands has no bit at all are skipped (they count nothing)."""
    n_sh, n_p = P.shape[:2]
    n_a, n_b = A.shape[1], B.shape[1]
    out = np.zeros((n_p, n_a, n_b), dtype=np.uint64)
    for s in range(n_sh):
        live = [sl for sl in range(16) if P[s, :, sl].any() and A[s, :, sl].any() and B[s, :, sl].any() and (F is None or F[s, sl].any())]
        if not live:
            continue
        p = P[s][:, live]
        if F is not None:
            p = p & F[s][live]
        pa = p[:, None] & A[s][:, live][None]  # [n_p, n_a, slots, 1024]
        for j in range(n_b):
            out[:, :, j] += np.bitwise_count(pa & B[s, j][live]).sum(axis=(2, 3), dtype=np.uint64)
    return out


def oracle_expected(p_bms: Sequence[Sequence], a_bms: Sequence[Sequence], b_bms: Sequence[Sequence], f_bms: Optional[Sequence],
                    triples: Sequence[Tuple[int, int, int]]) -> Dict[Tuple[int, int, int], int]:
    """x_bms[s][r]: oracle OBitmaps (None: no container anywhere in that row), f_bms[s] likewise or f_bms None: no filter."""
    out = {}
    for (p, i, j) in triples:
        n = 0
        for s in range(len(p_bms)):
            r0, r1, r2 = p_bms[s][p], a_bms[s][i], b_bms[s][j]
            if r0 is None or r1 is None or r2 is None:
                continue
            if f_bms is not None:
                if f_bms[s] is None:
                    continue
                r0 = r0.intersect(f_bms[s])
            r1 = r1.intersect(r0)
            n += r2.intersection_count(r1)
        out[(p, i, j)] = n
    return out


def sample_triples(rng, n_p: int, n_a: int, n_b: int, k: int = 4):
    """k triples, always with the two corners"""
    t = {(0, 0, 0), (n_p - 1, n_a - 1, n_b - 1)}
    while len(t) < min(k, n_p * n_a * n_b):
        t.add((int(rng.integers(0, n_p)), int(rng.integers(0, n_a)), int(rng.integers(0, n_b))))
    return sorted(t)


def chunk(n_shards: int, n_p: int, n_a: int, n_b: int, p_dense: bool, a_dense: bool, b_dense: bool, f_dense: bool = True) -> int:
    """the densify chunk of a call (include/fbk.h, fbk_count_cube); f_dense = True also stands for "no filter" """
    per = 8 * n_p * n_a * n_b
    per += (1 << 17) * ((0 if p_dense else n_p) + (0 if a_dense else n_a) + (0 if b_dense else n_b) + (0 if f_dense else 1))
    most = max(1, min(n_shards, (1 << 30) // per))
    passes = -(-n_shards // most)
    return -(-n_shards // passes)
