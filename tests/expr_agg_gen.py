"""Worlds and the numpy model for fbk_expr_bsi_agg / fbk_query_expr_bsi (shared by tests/test_expr_agg_cpu.py and
tests/test_gpu_expr_agg.py): expr_gen.World plus a second BSI fragment "W" per shard, so that a tree can filter on V and aggregate W,
or V itself.

W's bit depth is expr_gen.DEPTHS shifted by one (an iteration whose V has depth 0 has a W of depth 1, and so on round the list).
For certain it holds, in every world: slot NIL_SLOT without a single value in any shard (the exists container is nil there while the
existence row of batch "B", and so most filters, is not); slot FULL_SLOT of shard 0 with a value in every column (a full exists
container, dense random planes: their sum wraps uint64 at depth 63 / 64); RUN_SLOT with a stretch of equal values (run containers
among the planes); a few hundred scattered values (arrays).  Signs per shard: with two or more shards, shard 0 is all negative and
shard 1 all positive (a third is mixed); a one-shard world takes the three in turn (it // 3).  Magnitude 0 carries no sign bit, as
setValue never writes one.

The model: a field's values per shard as (columns, magnitudes uint64, negative bool); Sum / Min / Max over the columns of
model_tree & exists with the reference's rules (fragment.sum / min / max, fragment.go:724-853): Sum wraps in uint64; Min is minus
the largest magnitude among the negatives if there is one, else the smallest magnitude; Max the largest magnitude among the
non-negatives if there is one, else minus the smallest; the count is the number of columns holding that value; (0, 0) for nothing."""
from typing import List, Tuple

import numpy as np

import datagen as D
import expr_gen as G

SUM, MIN, MAX = 0, 1, 2  # FBK_AGG_* (include/fbk.h)
AGGS = (SUM, MIN, MAX)
NIL_SLOT, FULL_SLOT, RUN_SLOT = 9, 5, 2


def bitmap_of_words(words: np.ndarray):
    """[16, 1024] uint64 -> oracle bitmap with Container.optimize() applied (None when empty)"""
    from oracle import pyoracle as O

    items = []
    for slot in range(16):
        if words[slot].any():
            items.append((slot, O.optimize(O.OContainer.bitmap(words[slot]))))
    return O.OBitmap.from_containers(items) if items else None


def words_of_columns(cols: np.ndarray) -> np.ndarray:
    bits = np.zeros(1 << 20, dtype=np.uint8)
    bits[cols] = 1
    return np.packbits(bits, bitorder="little").view(np.uint64).reshape(16, 1024)


def to_int64(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


class Field:
    """an int field of a world: per shard (columns int64[n], magnitudes uint64[n], negative bool[n]), its oracle fragments"""

    def __init__(self, name: str, depth: int, data: List[Tuple[np.ndarray, np.ndarray, np.ndarray]]):
        from oracle import pybsi

        self.name, self.depth, self.data = name, depth, data
        self.base = [s * (depth + 2) for s in range(len(data))]
        self.frags = []
        for cols, mag, neg in data:
            rows = [cols, cols[neg]] + [cols[((mag >> np.uint64(i)) & np.uint64(1)).astype(bool)] for i in range(depth)]
            self.frags.append(pybsi.Fragment([bitmap_of_words(words_of_columns(r)) if r.size else None for r in rows]))

    def aggregate(self, agg: int, filt: np.ndarray) -> Tuple[List[int], List[int]]:
        """filt [n_shards, 16, 1024] -> (values, counts) per shard"""
        vals, counts = [], []
        for s, (cols, mag, neg) in enumerate(self.data):
            bits = np.unpackbits(np.ascontiguousarray(filt[s]).reshape(-1).view(np.uint8), bitorder="little")
            keep = bits[cols].astype(bool)
            m, n = [int(x) for x in mag[keep]], neg[keep]
            if not m:
                v, c = 0, 0
            elif agg == SUM:
                v, c = to_int64(sum(-x if sg else x for x, sg in zip(m, n))), len(m)
            else:
                decides = [x for x, sg in zip(m, n) if bool(sg) == (agg == MIN)]  # negatives decide a minimum, the others a maximum
                if decides:
                    best = max(decides)
                    v, c = to_int64(-best if agg == MIN else best), decides.count(best)
                else:
                    best = min(m)
                    v, c = to_int64(best if agg == MIN else -best), m.count(best)
            vals.append(v)
            counts.append(c)
        return vals, counts


def sign_mode(it: int, n_shards: int, s: int) -> str:
    if n_shards == 1:
        return ["negative", "positive", "mixed"][(it // 3) % 3]
    return ["negative", "positive", "mixed"][s]


class World(G.World):
    def __init__(self, it: int):
        super().__init__(it)
        rng = D.rng_for(9200, it)
        self.wdepth = G.DEPTHS[(it + 1) % len(G.DEPTHS)]
        lim = np.uint64((1 << min(self.wdepth, 63)) - 1)
        data = []
        for s in range(self.n_shards):
            scattered = rng.choice(1 << 20, size=300, replace=False).astype(np.int64)
            run = (RUN_SLOT << 16) + 700 + np.arange(3000, dtype=np.int64)
            cols = [scattered, run]
            mags = [rng.integers(0, 1 << 64, size=300, dtype=np.uint64, endpoint=False) & lim, np.full(3000, rng.integers(0, 1 << 64, dtype=np.uint64) & lim, dtype=np.uint64)]
            if s == 0:
                cols.append((FULL_SLOT << 16) + np.arange(65536, dtype=np.int64))
                mags.append(rng.integers(0, 1 << 64, size=65536, dtype=np.uint64, endpoint=False) & lim)
            c, m = np.concatenate(cols), np.concatenate(mags)
            c, first = np.unique(c, return_index=True)
            m = m[first]
            keep = (c >> 16) != NIL_SLOT
            c, m = c[keep], m[keep]
            mode = sign_mode(it, self.n_shards, s)
            neg = np.ones(c.size, bool) if mode == "negative" else np.zeros(c.size, bool) if mode == "positive" else rng.random(c.size) < 0.4
            data.append((c, m, neg & (m != 0)))
        self.fields = {"W": Field("W", self.wdepth, data)}
        vdata = []
        for s in range(self.n_shards):  # V as expr_gen made it, in the same form
            cols = np.asarray(sorted(self.values[s]), dtype=np.int64)
            vals = [self.values[s][int(c)] for c in cols]
            vdata.append((cols, np.asarray([abs(v) for v in vals], dtype=np.uint64), np.asarray([v < 0 for v in vals], dtype=bool)))
        v = Field.__new__(Field)
        v.name, v.depth, v.data, v.base, v.frags = "V", self.depth, vdata, list(self.base), self.frags
        self.fields["V"] = v
        self.agg_field = "V" if it % 4 == 3 else "W"  # what this iteration's tree is aggregated over

    def exists_words(self, field: str) -> np.ndarray:
        return np.stack([words_of_columns(cols) for cols, _, _ in self.fields[field].data])

    def model_agg(self, agg: int, tree, field: str) -> Tuple[List[int], List[int]]:
        return self.fields[field].aggregate(agg, self.model(tree))
