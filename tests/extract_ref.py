"""Expected values of fbk_extract_* (Extract(Limit(filter, limit=, offset=), Rows(f1), ...)) for the tests, two independent ways:

* the numpy brute force (select / bsi_expected / rows_expected): unpack the filter's words, list its columns shard by shard, cut
  the list by offset / limit, then gather values and memberships column by column.  No cleverness: it is the yardstick;
* the reference's own procedure through the oracle's row algebra (oracle_bsi / oracle_rows, executor.go:4747, :4845-4877,
  :4969-5026): filter.Columns() and a map from column to slot, then per bit plane / per row of the field one Intersect with the
  filter and an OR / append per column of the result.

Rows are [16, 1024] uint64 words (slot, word); BSI fragments [depth + 2, 16, 1024] (exists, sign, planes)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from msum_ref import bitmap_of_words, bits

U64 = (1 << 64) - 1


def select(F: np.ndarray, shard_ids: Sequence[int], offset: int = 0, limit: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """F [n_shards, 16, 1024] -> (shard index, position in the shard, column id) of the selected columns, all ascending"""
    sh, pos = [], []
    for s in range(F.shape[0]):
        p = np.nonzero(bits(F[s]))[0]
        sh.append(np.full(p.size, s, dtype=np.int64))
        pos.append(p.astype(np.int64))
    sh = np.concatenate(sh) if sh else np.zeros(0, dtype=np.int64)
    pos = np.concatenate(pos) if pos else np.zeros(0, dtype=np.int64)
    lo = min(offset, sh.size)
    hi = sh.size if limit is None else min(sh.size, lo + limit)
    sh, pos = sh[lo:hi], pos[lo:hi]
    ids = np.asarray(shard_ids, dtype=np.uint64)
    cols = ids[sh] * np.uint64(1 << 20) + pos.astype(np.uint64) if sh.size else np.zeros(0, dtype=np.uint64)
    return sh, pos, cols


def bsi_expected(S: np.ndarray, depth: int, sh: np.ndarray, pos: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """S [n_shards, depth + 2, 16, 1024] -> (values int64[n]: sign ? -magnitude : magnitude, wrapping, 0 where absent; present bool[n])"""
    vals, pres = np.zeros(sh.size, dtype=np.int64), np.zeros(sh.size, dtype=bool)
    for s in np.unique(sh):
        k = np.nonzero(sh == s)[0]
        b = bits(S[s])[:, pos[k]]
        mag = np.zeros(k.size, dtype=np.uint64)
        for p in range(depth):
            mag |= b[2 + p].astype(np.uint64) << np.uint64(p)
        v = np.where(b[1], ~mag + np.uint64(1), mag).view(np.int64)
        pres[k] = b[0]
        vals[k] = np.where(b[0], v, 0)
    return vals, pres


def rows_expected(A: np.ndarray, sh: np.ndarray, pos: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """A [n_shards, n_a, 16, 1024] -> CSR (offsets uint64[n + 1], items uint32[m]): per column the rows that hold it, ascending"""
    n_a = A.shape[1]
    member = np.zeros((sh.size, n_a), dtype=bool)
    for s in np.unique(sh):
        k = np.nonzero(sh == s)[0]
        for i in range(n_a):
            member[k, i] = bits(A[s, i])[pos[k]]
    offs = np.zeros(sh.size + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(member.sum(axis=1))
    return offs, np.nonzero(member)[1].astype(np.uint32)


def csr_lists(offs: np.ndarray, items: np.ndarray) -> List[List[int]]:
    return [items[int(offs[k]):int(offs[k + 1])].tolist() for k in range(offs.size - 1)]


# ---- the reference's procedure, on the oracle's rows (one shard at a time, no limit) -----------------------------------------
def _columns(bm) -> List[int]:
    return sorted(bm.slice()) if bm is not None else []


def oracle_bsi(O, F: np.ndarray, S: np.ndarray, depth: int) -> Tuple[List[int], List[Optional[int]]]:
    """one shard: (positions of the filter, per position the stored value or None): exists ∩ filter, sign ∩ exists ∩ filter, then
    per plane Intersect + an OR of 2^i per column (executor.go:4969-5026)"""
    f = bitmap_of_words(O, F)
    cols = _columns(f)
    slot = {c: k for k, c in enumerate(cols)}
    ex = bitmap_of_words(O, S[0])
    if f is None or ex is None:
        return cols, [None] * len(cols)
    exf = ex.intersect(f)
    present = set(_columns(exf))
    mag = [0] * len(cols)
    for p in range(depth):
        pl = bitmap_of_words(O, S[2 + p])
        if pl is None:
            continue
        for c in _columns(pl.intersect(exf)):
            mag[slot[c]] |= 1 << p
    sg = bitmap_of_words(O, S[1])
    neg = set(_columns(sg.intersect(exf))) if sg is not None else set()
    out: List[Optional[int]] = []
    for k, c in enumerate(cols):
        if c not in present:
            out.append(None)
            continue
        v = (-mag[k] if c in neg else mag[k]) & U64
        out.append(v - (1 << 64) if v >> 63 else v)
    return cols, out


def oracle_rows(O, F: np.ndarray, A: np.ndarray) -> Tuple[List[int], List[List[int]]]:
    """one shard: (positions of the filter, per position the rows holding it): per row Intersect + Columns() + the map
    (executor.go:4845-4877)"""
    f = bitmap_of_words(O, F)
    cols = _columns(f)
    slot = {c: k for k, c in enumerate(cols)}
    out: List[List[int]] = [[] for _ in cols]
    for i in range(A.shape[0]):
        r = bitmap_of_words(O, A[i])
        if r is None or f is None:
            continue
        for c in _columns(r.intersect(f)):
            out[slot[c]].append(i)
    return cols, out
