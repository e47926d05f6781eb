"""Expected result of fbk_bsi_distinct_rows for the tests: Distinct(filter, field=) of an int field as SignedRow{Neg, Pos}
(executeDistinctShardBSI, executor.go:2034-2153; the union over shards, :1190-1196).

* distinct_rows(): from (columns, stored values, base, optional filter columns) to {sign: {shard: sorted positions}}: a column takes
  part when it is in the filter (every column without one); v = stored + base; v >= 0 sets position v of "pos", v < 0 position -v of
  "neg" (:2123-2130); shard = position >> 20.  Python ints: nothing wraps; a v outside int64 is an error, as in the call.
* from_planes(): the same from dense planes [n_shards, depth + 2, 16, 1024] and a dense filter (pct_ref.values gives the stored values
  of exists ∩ filter, stored zeros included).
* row_positions(): the positions a downloaded fbk row holds, from its containers and their keys (shard * 16 + slot)."""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SHARD_BITS = 20


def distinct_rows(columns: Iterable[int], stored: Iterable[int], base: int = 0, filter_columns: Optional[Iterable[int]] = None) -> Dict[str, Dict[int, np.ndarray]]:
    keep = None if filter_columns is None else set(int(c) for c in filter_columns)
    sets = {"pos": set(), "neg": set()}
    for c, s in zip(columns, stored):
        if keep is not None and int(c) not in keep:
            continue
        v = int(s) + int(base)
        if not I64_MIN <= v <= I64_MAX:
            raise OverflowError("stored + base is outside int64")
        sets["pos" if v >= 0 else "neg"].add(v if v >= 0 else -v)
    out: Dict[str, Dict[int, np.ndarray]] = {}
    for sign, vals in sets.items():
        by_shard: Dict[int, list] = {}
        for p in sorted(vals):
            by_shard.setdefault(p >> SHARD_BITS, []).append(p)
        out[sign] = {sh: np.array(ps, dtype=np.uint64) for sh, ps in by_shard.items()}
    return out


def from_values(vals: np.ndarray, base: int = 0) -> Dict[str, Dict[int, np.ndarray]]:
    """distinct_rows() of stored values that all take part (vectorised: the GPU tests' larger inputs)"""
    u = np.unique(np.asarray(vals, dtype=np.int64))
    if u.size and not (I64_MIN <= int(u[0]) + base and int(u[-1]) + base <= I64_MAX):
        raise OverflowError("stored + base is outside int64")
    v = u + np.int64(base) if u.size else u
    pos = v[v >= 0].astype(np.uint64)
    neg = np.sort((np.uint64(0) - v[v < 0].astype(np.uint64)))
    out = {}
    for sign, p in (("pos", pos), ("neg", neg)):
        sh = p >> np.uint64(SHARD_BITS)
        out[sign] = {int(s): p[sh == s] for s in np.unique(sh)}
    return out


def from_planes(S: np.ndarray, F: Optional[np.ndarray], depth: int, base: int = 0) -> Dict[str, Dict[int, np.ndarray]]:
    import pct_ref as P

    return from_values(P.values(S, F, depth), base)


def row_positions(row) -> np.ndarray:
    """sorted positions (uint64) of a downloaded row {key: Container}; key = shard * 16 + slot"""
    parts = []
    for key in sorted(row):
        bits = np.unpackbits(row[key].words().view(np.uint8), bitorder="little")
        parts.append(np.nonzero(bits)[0].astype(np.uint64) + (np.uint64(key) << np.uint64(16)))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
