"""Expected values of fbk_bsi_sort (Sort(filter, field=, sort-desc=, limit=, offset=) by an int field) for the tests, two independent
ways:

* brute(): numpy on top of extract_ref.select / bsi_expected — list the columns of exists ∩ filter shard by shard with their values,
  drop the zero magnitudes (the reference's behaviour) unless keep_zero, np.lexsort((column, value)) with the value key reversed
  for descending, then offset and limit.  Equal values come in ascending column id: the order fbk.h fixes.  It is the yardstick;
* reference_sort(): the reference's own procedure on the oracle's row algebra (fragment.go:2907-2969, executor.go:9574-9608,
  :9367-9383): consider = exists ∩ filter, pos = consider − sign, neg = consider − pos, per plane from the top one Intersect and a
  dict update per column, the dict's records appended (negatives first), a stable sort by RowKV.Compare, a pairwise merge of the
  shards' lists, then cut().  The reference's order of EQUAL values is unspecified (Go map iteration, and Merge takes the other
  shard first on a tie), so the two are compared where the values are distinct, or after canon() ordered each run of equal values
  by column.

Rows are [16, 1024] uint64 words (slot, word); BSI fragments [depth + 2, 16, 1024] (exists, sign, planes)."""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np

import extract_ref as X
from msum_ref import bitmap_of_words

U64 = (1 << 64) - 1


def _order_key(vals: np.ndarray, desc: bool) -> np.ndarray:
    return ~vals if desc else vals  # ~v = -v - 1 reverses int64 order without overflow


def brute(S: np.ndarray, F: Optional[np.ndarray], shard_ids: Sequence[int], depth: int, desc: bool = False, keep_zero: bool = False, offset: int = 0,
          limit: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """S [n_shards, depth + 2, 16, 1024], F [n_shards, 16, 1024] or None -> (columns uint64[n], values int64[n], total)"""
    return order(*records(S, F, shard_ids, depth), desc, keep_zero, offset, limit)


def records(S: np.ndarray, F: Optional[np.ndarray], shard_ids: Sequence[int], depth: int) -> Tuple[np.ndarray, np.ndarray]:
    """brute()'s first half: (columns uint64, values int64) of exists ∩ filter in ascending column order, stored zeros included"""
    if S.shape[0] == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    consider = S[:, 0] if F is None else S[:, 0] & F
    sh, pos, cols = X.select(consider, shard_ids)
    vals, pres = X.bsi_expected(S, depth, sh, pos)
    assert pres.all()
    return cols, vals


def order(cols: np.ndarray, vals: np.ndarray, desc: bool = False, keep_zero: bool = False, offset: int = 0,
          limit: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """brute()'s second half, for callers that order one list of records several ways"""
    if not keep_zero:
        cols, vals = cols[vals != 0], vals[vals != 0]  # value 0 <=> magnitude 0 (the negation of a non-zero magnitude below 2^64 is not 0)
    order = np.lexsort((cols, _order_key(vals, desc)))
    cols, vals = cols[order], vals[order]
    lo = min(offset, cols.size)
    hi = cols.size if limit is None else min(cols.size, lo + limit)
    return cols[lo:hi], vals[lo:hi], int(order.size)


def canon(cols: np.ndarray, vals: np.ndarray, desc: bool) -> Tuple[np.ndarray, np.ndarray]:
    """a list sorted by value: every run of equal values ordered by column"""
    k = _order_key(vals, desc)
    assert (np.diff(k) >= 0).all(), "not sorted by value"
    order = np.lexsort((cols, k))
    return cols[order], vals[order]


# ---- the reference's procedure, on the oracle's rows ----------------------------------------------------------------------------
def _compare(a, b, desc: bool) -> bool:
    """RowKV.Compare for int64 values (fragment.go:2895-2899)"""
    return desc != (a[1] < b[1])


def _flatten(O, out: list, S: np.ndarray, filt, depth: int, sign: int, col0: int) -> None:
    """flattenRowValues (fragment.go:2943-2969); the map is walked in insertion order (Go: unspecified)"""
    m = {}
    if filt is None:
        return
    for i in range(depth - 1, -1, -1):
        row = bitmap_of_words(O, S[2 + i])
        if row is None:
            continue
        for v in sorted(row.intersect(filt).slice()):
            m[v] = m.get(v, 0) | (1 << i)
    for k, v in m.items():
        w = (v * sign) & U64  # int64 arithmetic wraps
        out.append((col0 + k, w - (1 << 64) if w >> 63 else w))


def sort_shard(O, S: np.ndarray, F: Optional[np.ndarray], shard_id: int, depth: int, desc: bool) -> List[Tuple[int, int]]:
    """sortBsiData (fragment.go:2907-2941): the shard's (column, value) records, sorted"""
    consider = bitmap_of_words(O, S[0])
    if consider is not None and F is not None:
        f = bitmap_of_words(O, F)
        consider = consider.intersect(f) if f is not None else None
    if consider is None:
        return []
    sign = bitmap_of_words(O, S[1])
    pos = consider.difference(sign) if sign is not None else consider
    neg = consider.difference(pos)
    recs: List[Tuple[int, int]] = []
    _flatten(O, recs, S, neg if neg.count() else None, depth, -1, shard_id << 20)
    _flatten(O, recs, S, pos if pos.count() else None, depth, 1, shard_id << 20)
    less = lambda a, b: _compare(a, b, desc)
    return sorted(recs, key=functools.cmp_to_key(lambda a, b: -1 if less(a, b) else (1 if less(b, a) else 0)))  # sort.SliceStable


def merge(s: List[Tuple[int, int]], o: List[Tuple[int, int]], desc: bool) -> List[Tuple[int, int]]:
    """SortedRow.Merge (executor.go:9574-9608)"""
    out, i, j = [], 0, 0
    while i < len(s) and j < len(o):
        if _compare(s[i], o[j], desc):
            out.append(s[i])
            i += 1
        else:
            out.append(o[j])
            j += 1
    return out + s[i:] + o[j:]


def reference_sort(O, S: np.ndarray, F: Optional[np.ndarray], shard_ids: Sequence[int], depth: int, desc: bool) -> Tuple[np.ndarray, np.ndarray]:
    """the merged list of all shards before offset / limit: (columns, values)"""
    acc: List[Tuple[int, int]] = []
    for s in range(S.shape[0]):
        part = sort_shard(O, S[s], None if F is None else F[s], int(shard_ids[s]), depth, desc)
        acc = part if s == 0 else merge(acc, part, desc)
    return np.array([c for c, _ in acc], dtype=np.uint64), np.array([v for _, v in acc], dtype=np.int64)


def cut(cols: np.ndarray, vals: np.ndarray, offset: int, limit: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
    """executor.go:9367-9383 (offset within the list)"""
    cols, vals = cols[offset:], vals[offset:]
    if limit is not None and limit < cols.size:
        cols, vals = cols[:limit], vals[:limit]
    return cols, vals
