"""Case generator of the structural fuzz of the calls that read densified operands (tests/test_gpu_fuzz_ops.py runs the cases on
the GPU, tests/test_fuzz_ops_cpu.py checks the generator and the references against each other without one).  No GPU in here.

A fuzz case is a POOL of rows and row lists into it.  The pool is datagen.random_row rows of every container archetype (missing
slots, wholly empty rows), a few special rows (two anchors without missing slots, one-container rows cut out of anchor 0, an empty
row, an all-ones row) and, in the odd iterations, BSI fragments built from values (many ties; planes that encode as runs, arrays or
nothing).  Its words are W [n_rows, 16, 1024]; the GPU test uploads the pool twice, encoded and dense, and every operand draws
which of the two it reads (case.enc), so one expectation covers every dense / encoded combination.  Row lists are arbitrary:
base_rows anywhere (exists, sign and planes are arbitrary rows, with bits outside exists), repeated and overlapping fragments,
filter rows inside the field's own fragment, repeats inside rows_a.

Expectations gather from W and go to the references (sort_ref, pct_ref, extract_ref, msum_ref, mdist_ref, distinct_rows_ref,
minmax_ref, moments_ref, cube_ref).

The operators groupby_minmax, moments and groupby_cube came after the first six.  groupby_minmax has groupby_sum's operands.  moments
adds a second field y: arbitrary rows at a depth of its own, absent in one iteration of the six, and in another x's own fragment
moved by 1 .. depth_x + 1 rows (MOMENTS_Y).  groupby_cube adds a leading field P of 1 .. 9 rows (both forms of its kernel) and cuts
A or B down to CUBE_CELLS cells.  Each has a stream of its own and draws what only it needs after the draws every operator makes,
so the cases of the first six are what they were before (tests/test_fuzz_ops_cpu.py).

The discrete structure choices come from the iteration number (PLAN), so six iterations cover them for every seed.  Nothing is
rejected: a case that would break a documented precondition or a budget of the references is constructed so that it does not:
  * shard 0 of every case but the empty one reads an anchor as exists and a filter row that is the anchor itself, a one-container
    cut of it or the all-ones row: exists ∩ filter is not empty whatever the seed; the empty case filters by the empty row;
  * fbk_bsi_distinct_rows makes one 2^17-byte output row per 2^20 positions that hold a value: arbitrary planes go up to depth 26
    (at most 2 * (2^6 + 1) rows), deeper fields (up to 40) read fragments built from values only; |base| < 2^40;
  * the GroupBy references hold one float64 per (group row, column of exists ∩ filter): without a filter n_a, n_b <= 12 and at most 4
    shards; 65 .. 130 rows (a second 64-row tile) come with one-container filter rows (<= 2^16 columns a shard) and at most 3 shards.

The short-chunk cases (short_*) are deterministic: the smallest shard count whose documented chunk arithmetic (include/fbk.h,
restated in chunk_extract / chunk_msum / chunk_mdist) leaves a shorter last chunk, row lists that repeat a few fragments and rows of a
small pool, one dense operand among the encoded ones, a sparse filter.  Their expectations are evaluated on the filter's columns only
(sparse_*: bit gathers from W), a second implementation the CPU test compares with the dense references on the fuzz cases."""
from __future__ import annotations

import os
from functools import cached_property
from typing import List, Optional, Sequence, Tuple

import numpy as np

import cube_ref as CU
import datagen as D
import distinct_rows_ref as DR
import extract_ref as X
import mdist_ref as MD
import minmax_ref as MM
import moments_ref as MO
import msum_ref as MS
import pct_ref as P
import sort_ref as SR

ITERS = int(os.environ.get("FBK_FUZZ_ITERS", "6"))
OPS = ("sort", "extract", "quantiles", "groupby_sum", "groupby_distinct", "distinct_rows", "groupby_minmax", "moments", "groupby_cube")
NEW_OPS = OPS[6:]  # added after the first six: whatever they draw, they draw after the draws every operator makes
STREAM = {op: 7400 + k for k, op in enumerate(OPS)}
TOP = P.RANK_FROM_TOP
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# the structure of iteration it (it % 6): filter present; two-field GroupBy; empty selection; the filter row lies inside the field's
# fragment; every operand from one batch (None: each operand draws); fragments built from values; 65 .. 130 group rows
PLAN = [
    dict(filter=True, two_field=True, empty=False, alias=True, one_batch=None, vb=False, big=False),
    dict(filter=False, two_field=False, empty=False, alias=False, one_batch=None, vb=True, big=False),
    dict(filter=True, two_field=True, empty=True, alias=False, one_batch=None, vb=False, big=False),
    dict(filter=True, two_field=False, empty=False, alias=False, one_batch="encoded", vb=True, big=True),
    dict(filter=False, two_field=True, empty=False, alias=False, one_batch=None, vb=False, big=False),
    dict(filter=True, two_field=True, empty=False, alias=False, one_batch="dense", vb=True, big=True),
]
# fbk_bsi_moments' second field in iteration it (it % 6): a fragment of its own; absent (the one-field form); x's fragment moved
# by 1 .. depth_x + 1 rows, so that the two fields share rows (y's exists is x's sign or one of x's planes)
MOMENTS_Y = ["own", "own", "own", "absent", "overlap", "own"]
CUBE_CELLS = 2000  # n_p * n_a * n_b of a groupby_cube case at most


def kind_of(c) -> str:
    """the datagen.KINDS archetype of an oracle container, from its encoding and content (a one-value array counts as `single`)"""
    from oracle import pyoracle as O

    if c.n == 1:
        return "single"
    if c.typ == O.ARRAY:
        return "empty_array" if c.n == 0 else "array_small" if c.n < 64 else "array_big" if c.n < 4096 else "array_dense_runs"
    if c.typ == O.BITMAP:
        return "bitmap_sparse" if c.n <= 300 else "bitmap_as_array_range" if c.n < 8192 else "bitmap_dense"
    runs = len(c.data())
    return "run_full" if c.n == 65536 else "run_split" if (runs == 2 and c.n == 65535) else "run_few" if runs <= 32 else "run_many"


class Pool:
    def __init__(self, rng, frag_values: Sequence[dict] = (), depth: int = 0):
        from oracle import pyoracle as O
        from oracle import pybsi as B

        self.p_missing = float(rng.choice([0.0, 0.15, 0.6, 0.95]))
        n_main = int(rng.integers(70, 101))
        rows = [D.random_row(rng, 0, 0.0) for _ in range(2)]  # the anchors
        rows += [D.random_row(rng, 0, self.p_missing) if rng.random() > 0.05 else {} for _ in range(n_main - 2)]
        full_slots = [s for s in range(16) if rows[0][s].n > 0]
        self.cuts = list(range(len(rows), len(rows) + 3))  # one container of anchor 0 each
        rows += [{int(s): rows[0][int(s)]} for s in rng.choice(full_slots, size=3)]
        self.empty = len(rows)
        rows.append({})
        self.full = len(rows)
        rows.append({s: O.OContainer.run([(0, 65535)]) for s in range(16)})
        self.n_plain = len(rows)  # base_rows of arbitrary fragments lie in [0, n_plain - depth - 2]
        self.frag_base: List[int] = []
        self.frag_filter: Optional[int] = None
        for k, vals in enumerate(frag_values):
            fr = B.bsi_fragment_from_values(vals, depth)
            self.frag_base.append(len(rows))
            rows += [{kk & 15: c for kk, c in bm.items() if c.n} if bm is not None else {} for bm in fr.rows]
            if k == 0:  # a filter that meets fragment 0: some of its columns, as arrays
                cols = sorted(vals)[:: max(1, len(vals) // 400)]
                self.frag_filter = len(rows)
                rows.append({sl: O.OContainer.array([c & 0xFFFF for c in cols if c >> 16 == sl]) for sl in sorted({c >> 16 for c in cols})})
        self.rows = rows
        self.kinds = [{kind_of(c) for c in r.values()} for r in rows]
        self.W = np.zeros((len(rows), 16, 1024), dtype=np.uint64)
        for r, row in enumerate(rows):
            for k, c in row.items():
                self.W[r, k & 15] = c.words()

    def fbk_rows(self):
        return [D.to_fbk_row(r) for r in self.rows]


def _frag_values(rng, depth: int, n_frag: int, max_cols: int = 3000) -> List[dict]:
    """{column: value} per fragment: uniform values, few distinct small ones, values clustered around one (tests/test_gpu_fuzz_struct.py)"""
    lim = (1 << min(depth, 63)) - 1
    out = []
    for _ in range(n_frag):
        ncol = min(max_cols, int(rng.choice([3, 200, 3000])))
        span = int(rng.choice([1 << 20, 1 << 16, 70000]))
        cols = rng.choice(span, size=ncol, replace=False)
        kind = int(rng.integers(0, 3))
        if kind == 0:
            mag = [int(rng.integers(0, lim + 1)) if lim < (1 << 62) else int(rng.integers(0, 1 << 62)) * 2 + int(rng.integers(0, 2)) for _ in cols]
        elif kind == 1:
            mag = [min(lim, int(v)) for v in rng.integers(0, 7, size=ncol)]
        else:
            c0 = int(rng.integers(0, lim + 1)) if lim < (1 << 62) else int(rng.integers(0, 1 << 62))
            mag = [min(lim, max(0, c0 + int(d))) for d in rng.integers(-50, 50, size=ncol)]
        sign = np.where(rng.random(ncol) < rng.choice([0.0, 0.4, 1.0]), -1, 1)
        out.append({int(c): int(m) * int(g) for c, m, g in zip(cols, mag, sign)})
    return out


class Case:
    """One fuzz case of operator `op`, iteration `it`.  Row lists index pool.W; enc[name] says whether the operand (bsi, filter, a,
    b; y of moments; p of groupby_cube) reads the encoded upload of the pool (else the dense one).  features: what PLAN made of it."""

    def __init__(self, op: str, it: int):
        assert op in OPS
        self.op, self.it = op, it
        plan = dict(PLAN[it % len(PLAN)])
        rng = self.rng = D.rng_for(STREAM[op], it)
        groupby = op.startswith("groupby")
        if op == "extract":
            plan["filter"] = True  # the filter is the selection
        max_depth = 63 if op == "distinct_rows" else 64
        if op == "distinct_rows":
            max_depth = 40 if plan["vb"] else 26
        self.depth = depth = int(rng.integers(0, max_depth + 1))
        deep = op == "distinct_rows" and depth > 26  # fragments built from values only, of at most 200 columns (output rows) each
        n_sh_max = 6
        if groupby and not plan["filter"]:
            n_sh_max = 4
        if groupby and plan["big"]:
            n_sh_max = 3
        self.n_sh = n_sh = int(rng.integers(1, n_sh_max + 1))
        first = int(rng.choice([0, 0, 1 << 12, 1 << 31, (1 << 44) - 64]))
        self.shard_ids = (first + np.cumsum(rng.integers(1, 5, n_sh)) - 1).astype(np.uint64)
        fv = _frag_values(rng, depth, int(rng.integers(1, 4)), 200 if deep else 3000) if plan["vb"] else []
        pool = self.pool = Pool(rng, fv, depth)
        W = self.W = pool.W
        n_rows = W.shape[0]

        # the field: arbitrary fragments (repeats and overlaps allowed), some of them built from values
        hi = pool.n_plain - depth - 2
        base = rng.integers(0, hi + 1, n_sh)
        if rng.random() < 0.3:
            base[:] = base[0]  # every shard the same fragment
        for s in range(n_sh):
            if pool.frag_base and (deep or rng.random() < 0.5):
                base[s] = pool.frag_base[int(rng.integers(0, len(pool.frag_base)))]
        # the filter: arbitrary rows; inside the field's own fragment (alias); one-container rows (big); the empty row (empty)
        rows_f = rng.integers(0, n_rows, n_sh)
        if rng.random() < 0.25:
            rows_f[:] = rows_f[0]
        if plan["alias"]:
            rows_f = base + rng.integers(0, depth + 2, n_sh)
        if plan["big"]:
            rows_f = rng.choice(pool.cuts, size=n_sh)
        # shard 0: not empty by construction
        if deep:
            base[0], rows_f[0] = pool.frag_base[0], pool.frag_filter
        else:
            base[0] = 0
            rows_f[0] = 0 if plan["alias"] else pool.cuts[0] if plan["big"] else int(rng.choice([pool.full, pool.cuts[1], 0]))
        if plan["empty"]:
            rows_f[:] = pool.empty
        self.base_rows = base.astype(np.uint32)
        self.rows_f = rows_f.astype(np.uint32) if plan["filter"] else None

        # set fields: repeats inside a shard's list; the all-ones row at one index of A (and of B)
        def width(big):
            return int(rng.integers(65, 131)) if big else int(rng.integers(1, 13 if (groupby and not plan["filter"]) else 41))

        big_a = plan["big"] and (not groupby or not plan["two_field"])
        self.n_a, self.n_b = width(big_a), width(plan["big"] and not big_a)
        self.rows_a = rng.integers(0, n_rows, (n_sh, self.n_a)).astype(np.uint32)
        if self.n_a > 2:
            self.rows_a[:, 1] = self.rows_a[:, 0]
        self.i_full = int(rng.integers(0, self.n_a))
        self.rows_a[:, self.i_full] = pool.full
        self.rows_b = None
        if groupby and plan["two_field"]:
            self.rows_b = rng.integers(0, n_rows, (n_sh, self.n_b)).astype(np.uint32)
            self.j_full = int(rng.integers(0, self.n_b))
            self.rows_b[:, self.j_full] = pool.full
        else:
            self.n_b, self.j_full = 1, 0

        names = ("bsi", "filter", "a", "b")
        if plan["one_batch"]:
            self.enc = {k: plan["one_batch"] == "encoded" for k in names}
        else:
            self.enc = {k: bool(rng.random() < 0.5) for k in names}
        self.features = {"filter": plan["filter"], "no_filter": not plan["filter"], "two_field": self.rows_b is not None,
                         "one_field": self.rows_b is None, "empty": plan["empty"], "alias_filter": plan["alias"], "one_batch": bool(plan["one_batch"]),
                         "value_fragments": bool(pool.frag_base), "big_tile": plan["big"]}
        self.depth_y, self.base_rows_y, self.n_p, self.rows_p, self.p_full = 0, None, 0, None, 0
        if op in NEW_OPS:
            for k in {"moments": ("y",), "groupby_cube": ("p",)}.get(op, ()):
                self.enc[k] = plan["one_batch"] == "encoded" if plan["one_batch"] else bool(rng.random() < 0.5)
        if op == "moments":
            self._second_field(MOMENTS_Y[it % len(PLAN)])
        if op == "groupby_cube":
            self._leading_field()

    def _second_field(self, how: str):
        """y of fbk_bsi_moments: arbitrary rows of the pool at a depth of its own; shard 0 reads x's exists (anchor 0) as its own, so
        exists_x ∩ exists_y ∩ filter is not empty there (`overlap`: anchor 1, one row on)"""
        rng, pool, depth = self.rng, self.pool, self.depth
        dy = int(rng.integers(0, 65))
        if how == "overlap":
            dy = min(dy, pool.n_plain - depth - 3)  # both fragments, moved by up to depth + 1 rows, fit the plain rows
        by = rng.integers(0, pool.n_plain - dy - 2 + 1, self.n_sh)
        by[0] = 0
        if how == "overlap":
            bx = self.base_rows.astype(np.int64)
            assert not pool.frag_base and self.rows_f is None  # (nothing else depends on where x lies)
            by = bx + rng.integers(1, depth + 2, self.n_sh)
            by[0] = 1
            over = np.maximum(0, by + dy + 2 - pool.n_plain)  # <= bx: move both down
            bx, by = bx - over, by - over
            assert (bx >= 0).all() and bx[0] == 0
            self.base_rows = bx.astype(np.uint32)
        self.depth_y, self.base_rows_y = (dy, by.astype(np.uint32)) if how != "absent" else (0, None)
        ov = self.base_rows_y is not None and bool(((self.base_rows_y > self.base_rows) & (self.base_rows_y <= self.base_rows + depth + 1)).all())
        self.features.update(one_field_y=how == "absent", y_overlaps_x=how == "overlap" and ov)

    def _leading_field(self):
        """P of fbk_count_cube: 1 .. 4 rows (the kernel's 4-row form) in the even iterations, 5 .. 9 (the 8-row form) in the odd
        ones, the all-ones row at one index; A or B lose rows until the cube has at most CUBE_CELLS cells (a side of more than 64
        rows keeps them); the one-field iterations give B the all-ones row alone"""
        rng, pool, n_sh = self.rng, self.pool, self.n_sh
        self.n_p = n_p = int(rng.integers(1, 5)) if self.it % 2 == 0 else int(rng.integers(5, 10))
        self.rows_p = rng.integers(0, self.W.shape[0], (n_sh, n_p)).astype(np.uint32)
        self.p_full = int(rng.integers(0, n_p))
        self.rows_p[:, self.p_full] = pool.full
        if self.rows_b is None:
            self.rows_b = np.full((n_sh, 1), pool.full, dtype=np.uint32)
        n_a, n_b = self.n_a, self.n_b
        if n_p * n_a * n_b > CUBE_CELLS:
            if n_a > 64 or (n_b <= 64 and n_b >= n_a):
                n_b = max(1, CUBE_CELLS // (n_p * n_a))
            else:
                n_a = max(1, CUBE_CELLS // (n_p * n_b))
        assert n_p * n_a * n_b <= CUBE_CELLS
        self.n_a, self.n_b, self.i_full, self.j_full = n_a, n_b, self.i_full % n_a, self.j_full % n_b
        self.rows_a, self.rows_b = np.ascontiguousarray(self.rows_a[:, :n_a]), np.ascontiguousarray(self.rows_b[:, :n_b])
        self.rows_a[:, self.i_full], self.rows_b[:, self.j_full] = pool.full, pool.full

    def __repr__(self):
        more = f", depth_y={self.depth_y}" if self.op == "moments" else f", n_p={self.n_p}" if self.op == "groupby_cube" else ""
        return f"Case({self.op}, it={self.it}, depth={self.depth}, n_sh={self.n_sh}, n_a={self.n_a}, n_b={self.n_b}{more}, enc={self.enc}, {self.features})"

    # -- what the case reads ---------------------------------------------------------------------
    def rows_read_encoded(self) -> set:
        out = set()
        if self.enc["bsi"] and self.op != "groupby_cube":
            out |= set((self.base_rows[:, None] + np.arange(self.depth + 2)).reshape(-1).tolist())
        if self.enc["filter"] and self.rows_f is not None:
            out |= set(self.rows_f.tolist())
        if self.enc["a"] and self.op in ("sort", "extract", "groupby_sum", "groupby_distinct", "groupby_minmax", "groupby_cube"):
            out |= set(self.rows_a.reshape(-1).tolist())
        if self.enc["b"] and self.rows_b is not None:
            out |= set(self.rows_b.reshape(-1).tolist())
        if self.enc.get("y") and self.base_rows_y is not None:
            out |= set((self.base_rows_y[:, None] + np.arange(self.depth_y + 2)).reshape(-1).tolist())
        if self.enc.get("p") and self.rows_p is not None:
            out |= set(self.rows_p.reshape(-1).tolist())
        return out

    # -- gathered operands and the references -----------------------------------------------------
    @cached_property
    def S(self) -> np.ndarray:
        return self.W[self.base_rows[:, None].astype(np.int64) + np.arange(self.depth + 2)]

    @cached_property
    def F(self) -> Optional[np.ndarray]:
        return None if self.rows_f is None else self.W[self.rows_f]

    @cached_property
    def A(self) -> np.ndarray:
        return self.W[self.rows_a]

    @cached_property
    def Bw(self) -> Optional[np.ndarray]:
        return None if self.rows_b is None else self.W[self.rows_b]

    @cached_property
    def Sy(self) -> Optional[np.ndarray]:
        return None if self.base_rows_y is None else self.W[self.base_rows_y[:, None].astype(np.int64) + np.arange(self.depth_y + 2)]

    @cached_property
    def Pw(self) -> np.ndarray:
        return self.W[self.rows_p]

    @cached_property
    def records(self) -> Tuple[np.ndarray, np.ndarray]:
        """(columns, values) of exists ∩ filter, ascending columns (sort_ref.records)"""
        return SR.records(self.S, self.F, self.shard_ids, self.depth)

    @cached_property
    def values(self) -> np.ndarray:
        return P.values(self.S, self.F, self.depth)

    @cached_property
    def total(self) -> int:
        """the participating set: |exists ∩ filter| over the shards (Extract and the cube: the filter's columns; moments: y's exists too)"""
        if self.op == "groupby_cube" and self.F is None:
            return self.n_sh << 20
        w = self.F if self.op in ("extract", "groupby_cube") else (self.S[:, 0] if self.F is None else self.S[:, 0] & self.F)
        if self.Sy is not None:
            w = w & self.Sy[:, 0]
        return int(np.bitwise_count(w).sum())

    def sort_expected(self, desc, keep_zero, offset, limit):
        return SR.order(*self.records, desc, keep_zero, offset, limit)

    def locate(self, cols: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """columns -> (shard index, position)"""
        c = np.asarray(cols, dtype=np.uint64)
        return np.searchsorted(self.shard_ids, c >> np.uint64(20)).astype(np.int64), (c & np.uint64(0xFFFFF)).astype(np.int64)

    def percentile_base(self) -> int:
        """a random Base with minimum + Base and maximum + Base inside int64"""
        v = self.values
        mn, mx = (int(v.min()), int(v.max())) if v.size else (0, 0)
        lo, hi = max(I64_MIN - mn, -(1 << 62)), min(I64_MAX - mx, 1 << 62)
        return int(self.rng.integers(lo, hi + 1)) if self.rng.random() < 0.7 else 0

    def pick_cut(self, total: int, none_ok: bool):
        opts = [0, 1, int(self.rng.integers(0, total + 2)), max(total - 1, 0), total, total + 1] + ([None] if none_ok else [])
        return opts[int(self.rng.integers(0, len(opts)))]

    def msum_expected(self):
        return MS.numpy_expected(self.A, self.Bw, self.F, self.S, self.depth)

    def mdist_expected(self):
        return MD.numpy_expected(self.A, self.Bw, self.F, self.S, self.depth)

    def distinct_rows_expected(self, base: int):
        return DR.from_planes(self.S, self.F, self.depth, base)

    def minmax_expected(self):
        """(mins, maxs, min_counts, max_counts)"""
        return MM.numpy_expected(self.A, self.Bw, self.F, self.S, self.depth)

    def group_counts(self) -> np.ndarray:
        """msum_expected()[1], the columns of every group, without the sums: per shard a float64 product of the member matrices
        (exact: a count is at most 2^20).  tests/test_fuzz_ops_cpu.py holds it against msum_ref on the default cases."""
        out = np.zeros((self.n_a, self.n_b), dtype=np.uint64)
        for s in range(self.n_sh):
            g = MS.bits(self.S[s, 0])
            if self.F is not None:
                g &= MS.bits(self.F[s])
            cols = np.nonzero(g)[0]
            a = MS.bits(self.A[s])[:, cols].astype(np.float64)
            b = MS.bits(self.Bw[s])[:, cols].astype(np.float64) if self.Bw is not None else np.ones((1, cols.size))
            out += (a @ b.T).astype(np.uint64)
        return out

    def moments_expected(self) -> MO.Moments:
        return MO.expected(self.S, self.depth, self.Sy, self.depth_y, self.F)

    def cube_expected(self) -> np.ndarray:
        return CU.numpy_expected(self.Pw, self.A, self.Bw, self.F)

    @cached_property
    def selected_magnitudes(self) -> Tuple[np.ndarray, np.ndarray]:
        """(magnitude uint64, sign bit) of every column of exists ∩ filter"""
        sets = [self.base_rows] + ([self.rows_f] if self.rows_f is not None else [])
        return sparse_magnitudes(self.W, self.base_rows, self.depth, *sparse_columns(self.W, sets))[:2]


def cases(op: str, iters: int = ITERS):
    return [Case(op, it) for it in range(iters)]


# ---- the chunk arithmetic of include/fbk.h --------------------------------------------------------------------------------------
def _even(shards: int, most: int) -> int:
    passes = -(-shards // most)
    return -(-shards // passes)


def chunk_extract(shards: int, rows_per_shard: int) -> int:
    """fbk_extract_*, fbk_bsi_sort, _quantiles, _percentile, _distinct_rows: 2^28 bytes of scratch, R = the rows densified per shard"""
    per = (1 << 17) * rows_per_shard
    assert 0 < per <= 1 << 28
    return _even(shards, max(1, min(shards, (1 << 28) // per)))


def chunk_msum(shards: int, n_a: int, n_b: int, depth: int, rows_densified: int) -> int:
    per = -(-depth // 7) * (1 << 20) + 16 * n_a * n_b + (1 << 17) * rows_densified
    return _even(shards, max(1, min(shards, (1 << 30) // per)))


def chunk_mdist(shards: int, rows_densified: int) -> int:
    return _even(shards, max(1, min(shards, (1 << 30) // ((1 << 17) * rows_densified))))


def split(shards: int, chunk: int) -> List[int]:
    return [min(chunk, shards - s0) for s0 in range(0, shards, chunk)]


def smallest_uneven(chunk_of) -> int:
    """the smallest shard count that chunk_of(shards) deals into at least two chunks with a shorter last one"""
    n = 1
    while True:
        parts = split(n, chunk_of(n))
        if len(parts) >= 2 and parts[-1] < parts[0]:
            return n
        n += 1


# ---- evaluation on the filter's columns only ------------------------------------------------------------------------------------
def bit_at(W: np.ndarray, rows: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """bit pos[k] of row rows[k] (broadcast) of W"""
    pos = np.asarray(pos, dtype=np.int64)
    w = W[rows, pos >> 16, (pos >> 6) & 1023]
    return ((w >> (pos & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def sparse_columns(W: np.ndarray, row_sets: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """(shard index, position) of the columns in the AND of the rows row_sets[k][s] of every shard s, ascending"""
    cache, sh, pos = {}, [], []
    n_sh = len(row_sets[0])
    for s in range(n_sh):
        key = tuple(int(r[s]) for r in row_sets)
        if key not in cache:
            w = W[key[0]]
            for r in key[1:]:
                w = w & W[r]
            cache[key] = np.nonzero(MS.bits(w))[0].astype(np.int64) if w.any() else np.zeros(0, dtype=np.int64)
        pos.append(cache[key])
        sh.append(np.full(cache[key].size, s, dtype=np.int64))
    return np.concatenate(sh), np.concatenate(pos)


def sparse_values(W: np.ndarray, base_rows: np.ndarray, depth: int, sh: np.ndarray, pos: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(values int64: sign ? -magnitude : magnitude, wrapping, 0 where absent; present) of the columns (sh, pos)"""
    b = np.asarray(base_rows, dtype=np.int64)[sh]
    mag = np.zeros(sh.size, dtype=np.uint64)
    for p in range(depth):
        mag |= bit_at(W, b + 2 + p, pos).astype(np.uint64) << np.uint64(p)
    pres = bit_at(W, b, pos)
    v = np.where(bit_at(W, b + 1, pos), ~mag + np.uint64(1), mag).view(np.int64)
    return np.where(pres, v, 0), pres


def sparse_magnitudes(W: np.ndarray, base_rows: np.ndarray, depth: int, sh: np.ndarray, pos: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(magnitude uint64, sign bit, present) of the columns (sh, pos): the value is -magnitude where the sign bit is set, up to
    65 bits at depth 64"""
    b = np.asarray(base_rows, dtype=np.int64)[sh]
    mag = np.zeros(sh.size, dtype=np.uint64)
    for p in range(depth):
        mag |= bit_at(W, b + 2 + p, pos).astype(np.uint64) << np.uint64(p)
    return mag, bit_at(W, b + 1, pos), bit_at(W, b, pos)


def sparse_ints(W: np.ndarray, base_rows: np.ndarray, depth: int, sh: np.ndarray, pos: np.ndarray) -> Tuple[List[int], np.ndarray]:
    """(values as Python ints: sign ? -magnitude : magnitude, not wrapped; present) of the columns (sh, pos)"""
    mag, sign, pres = sparse_magnitudes(W, base_rows, depth, sh, pos)
    return [-m if s else m for m, s in zip(mag.tolist(), sign.tolist())], pres


def minmax_of(mag: np.ndarray, sign: np.ndarray) -> Tuple[int, int, int, int]:
    """(min, max, columns at the min, columns at the max) of the values sign ? -mag : mag, compared as Python ints and written as
    int64 with wrap-around; nothing: (INT64_MAX, INT64_MIN, 0, 0)"""
    if mag.size == 0:
        return I64_MAX, I64_MIN, 0, 0
    neg = sign & (mag != 0)
    vals = [-int(mag[neg].max()), -int(mag[neg].min())] if neg.any() else []  # the extremes of either sign
    vals += [int(mag[~neg].min()), int(mag[~neg].max())] if not neg.all() else []
    lo, hi = min(vals), max(vals)
    count = lambda v: int(((mag == np.uint64(abs(v))) & (neg == (v < 0))).sum())  # noqa: E731
    wrap = lambda v: ((v + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)  # noqa: E731
    return wrap(lo), wrap(hi), count(lo), count(hi)


def sparse_rows(W: np.ndarray, rows_a: np.ndarray, sh: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """member [n, n_a]: column k lies in row rows_a[sh[k], i]"""
    ra = np.asarray(rows_a, dtype=np.int64)
    return np.stack([bit_at(W, ra[sh, i], pos) for i in range(ra.shape[1])], axis=1) if sh.size else np.zeros((0, ra.shape[1]), dtype=bool)


def csr_of(member: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    offs = np.zeros(member.shape[0] + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(member.sum(axis=1))
    return offs, np.nonzero(member)[1].astype(np.uint32)


def sparse_groupby(W, rows_a, rows_b, base_rows, rows_f, depth) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(sums int64, counts uint64, distinct uint64), each [n_a, n_b], over exists ∩ filter [∩ A_i ∩ B_j]"""
    sets = [base_rows] + ([rows_f] if rows_f is not None else [])
    sh, pos = sparse_columns(W, sets)
    val, _ = sparse_values(W, base_rows, depth, sh, pos)
    a = sparse_rows(W, rows_a, sh, pos)
    b = sparse_rows(W, rows_b, sh, pos) if rows_b is not None else np.ones((sh.size, 1), dtype=bool)
    n_a, n_b = a.shape[1], b.shape[1]
    sums, counts, dist = np.zeros((n_a, n_b), dtype=np.uint64), np.zeros((n_a, n_b), dtype=np.uint64), np.zeros((n_a, n_b), dtype=np.uint64)
    for i in range(n_a):
        for j in range(n_b):
            v = val[a[:, i] & b[:, j]]
            counts[i, j], dist[i, j] = v.size, np.unique(v).size
            sums[i, j] = np.add.reduce(v.view(np.uint64), dtype=np.uint64) if v.size else 0
    return sums.view(np.int64), counts, dist


def _minmax_groups(mag, sign, a, b):
    """minmax_of per group: (mins int64, maxs int64, min_counts uint64, max_counts uint64), each [n_a, n_b]"""
    n_a, n_b = a.shape[1], b.shape[1]
    out = (np.zeros((n_a, n_b), dtype=np.int64), np.zeros((n_a, n_b), dtype=np.int64), np.zeros((n_a, n_b), dtype=np.uint64), np.zeros((n_a, n_b), dtype=np.uint64))
    for i in range(n_a):
        mi, si, bi = mag[a[:, i]], sign[a[:, i]], b[a[:, i]]
        for j in range(n_b):
            for o, v in zip(out, minmax_of(mi[bi[:, j]], si[bi[:, j]])):
                o[i, j] = v
    return out


def sparse_minmax(W, rows_a, rows_b, base_rows, rows_f, depth):
    """sparse_groupby's gather, the minimum and the maximum of every group and the columns that hold them"""
    sh, pos = sparse_columns(W, [base_rows] + ([rows_f] if rows_f is not None else []))
    mag, sign, _ = sparse_magnitudes(W, base_rows, depth, sh, pos)
    a = sparse_rows(W, rows_a, sh, pos)
    b = sparse_rows(W, rows_b, sh, pos) if rows_b is not None else np.ones((sh.size, 1), dtype=bool)
    return _minmax_groups(mag, sign, a, b)


def sparse_cube(W, rows_p, rows_a, rows_b, rows_f, triples) -> List[int]:
    """the count of P_p ∩ A_i ∩ B_j [∩ F] over the shards for the given triples: Python's popcount of the words as one integer"""
    out = []
    for (p, i, j) in triples:
        n = 0
        for s in range(rows_p.shape[0]):
            w = W[rows_p[s, p]] & W[rows_a[s, i]] & W[rows_b[s, j]]
            if rows_f is not None:
                w = w & W[rows_f[s]]
            n += bin(int.from_bytes(w.tobytes(), "little")).count("1")
        out.append(n)
    return out


# ---- the short-chunk cases --------------------------------------------------------------------------------------------------------
def _encode_rows(W: np.ndarray):
    """[n, 16, 1024] words -> fbk rows in the encodings Container.optimize() picks (datagen.fbk_container_of_vals: numpy only)"""
    out = []
    for r in range(W.shape[0]):
        row = {}
        for sl in range(16):
            if W[r, sl].any():
                row[sl] = D.fbk_container_of_vals(np.nonzero(np.unpackbits(W[r, sl].view(np.uint8), bitorder="little"))[0].astype(np.int64))
        out.append(row)
    return out


class ShortCase:
    """A deterministic call whose densify walk ends in a shorter chunk.  Pools are small: fragments `frag` (two of depth + 2 rows),
    filter rows `filt` (four; row 2 is empty, row 3 is read by the last chunk only), set-field rows `arow`; the row lists repeat them irregularly.  dense[name]: the
    operand reads a dense upload of its pool (the others an encoded one).  A second field y (fbk_bsi_moments) reads the fragments
    too, a leading field P (fbk_count_cube) the set-field rows."""

    def __init__(self, name: str):
        self.name = name
        rng = self.rng = D.rng_for(7490, SHORT_STREAM.index(name))
        spec = SHORT[name]
        self.depth = depth = spec["depth"]
        self.n_a, self.n_b, self.n_p = spec.get("n_a", 1), spec.get("n_b", 1), spec.get("n_p", 0)
        self.dense = {k: k in spec["dense"] for k in ("bsi", "filter", "a", "b") + (("y",) if "y" in spec else ()) + (("p",) if self.n_p else ())}
        self.chunk_of = spec["chunk_of"]
        self.n_sh = n_sh = smallest_uneven(self.chunk_of)
        self.chunks = split(n_sh, self.chunk_of(n_sh))
        rnd = lambda shape, ands=0: np.bitwise_and.reduce(rng.integers(0, 1 << 63, (ands + 1,) + tuple(shape), dtype=np.uint64) * 2 + rng.integers(0, 2, (ands + 1,) + tuple(shape), dtype=np.uint64), axis=0)  # noqa: E731
        # every row lives in words 100..101 of slot 3 (sparse bits: arrays), a run in slot 7, one word in slot 12
        def rows(n, ands):
            w = np.zeros((n, 16, 1024), dtype=np.uint64)
            w[:, 3, 100:102] = rnd((n, 2), ands)
            w[:, 7, 16:20] = rnd((n, 1), 6) | np.uint64(0x00FFFF00)
            w[:, 12, 1023] = rnd((n,), ands)
            return w
        frag = rows(2 * (depth + 2), 0)
        frag = frag.reshape(2, depth + 2, 16, 1024)
        frag[:, 2 + min(depth, spec.get("planes", 64)):] = 0  # the planes above stay empty: small magnitudes
        self.Wfrag = frag.reshape(-1, 16, 1024)
        filt = rows(4, 1)
        filt[2] = 0
        self.Wfilt = filt
        self.Warow = rows(min(max(self.n_a, self.n_b) + 3, 67), 0)  # (row lists wrap around it)
        self.base_rows = (rng.integers(0, 2, n_sh) * (depth + 2)).astype(np.uint32)
        self.rows_f = rng.integers(0, 3, n_sh).astype(np.uint32)
        self.rows_f[[0, n_sh - 1]] = [0, 1]  # the first and the last shard hold selected columns
        self.rows_f[self.chunks[0]] = 1  # ... and the first shard of the second chunk
        self.rows_f[self.chunks[0] + 1:n_sh - 1:5] = 3  # a row no shard of the first chunk reads: a union over the shards needs it
        c0 = self.chunks[0]  # the second chunk starts with another fragment and other rows than the first
        self.base_rows[c0] = (depth + 2) - self.base_rows[0]
        shift = rng.integers(0, 3, n_sh)
        shift[c0] = (shift[0] + 1) % 3
        self.rows_a = ((np.arange(self.n_a)[None, :] + shift[:, None]) % self.Warow.shape[0]).astype(np.uint32)
        self.rows_b = ((np.arange(self.n_b)[None, :] + 2 - shift[:, None]) % self.Warow.shape[0]).astype(np.uint32)
        self.shard_ids = (np.arange(n_sh, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 12))
        # the operands of the calls added later, drawn last: a second field y that reads the other fragment of the pool in some
        # shards (the first of either chunk among them) and x's own in others (shard 1 among them); a leading field P
        self.base_rows_y = None
        if "y" in spec:
            other = rng.integers(0, 2, n_sh)
            other[[0, 1, c0]] = [1, 0, 1]
            self.base_rows_y = np.where(other == 1, (depth + 2) - self.base_rows.astype(np.int64), self.base_rows).astype(np.uint32)
        self.rows_p = ((np.arange(self.n_p)[None, :] + 1 + 2 * shift[:, None]) % self.Warow.shape[0]).astype(np.uint32) if self.n_p else None

    def uploads(self):
        """{operand: (words, encoded rows or None for a dense upload)}"""
        pools = {"bsi": self.Wfrag, "filter": self.Wfilt, "a": self.Warow, "b": self.Warow}
        pools.update({"y": self.Wfrag} if "y" in self.dense else {}, **({"p": self.Warow} if self.n_p else {}))
        return {k: (w, None if self.dense[k] else _encode_rows(w)) for k, w in pools.items()}

    # expectations, on the columns of exists ∩ filter (Extract: of the filter) only
    @cached_property
    def filter_columns(self):
        return sparse_columns(self.Wfilt, [self.rows_f])

    @cached_property
    def records(self):
        """(columns, values) of exists ∩ filter"""
        sh, pos = self.filter_columns
        val, pres = sparse_values(self.Wfrag, self.base_rows, self.depth, sh, pos)
        return self.shard_ids[sh[pres]] * np.uint64(1 << 20) + pos[pres].astype(np.uint64), val[pres]

    def groupby(self, minmax: bool = False):
        """sparse_groupby over separate pools: the filter's columns first, then exists -> (sums, counts, distinct); minmax: the
        same gather -> (mins, maxs, min_counts, max_counts)"""
        sh, pos = self.filter_columns
        val, pres = sparse_values(self.Wfrag, self.base_rows, self.depth, sh, pos)
        sh, pos, val = sh[pres], pos[pres], val[pres]
        a, b = sparse_rows(self.Warow, self.rows_a, sh, pos), sparse_rows(self.Warow, self.rows_b, sh, pos)
        if minmax:
            mag, sign, _ = sparse_magnitudes(self.Wfrag, self.base_rows, self.depth, sh, pos)
            return _minmax_groups(mag, sign, a, b)
        out = [np.zeros((self.n_a, self.n_b), dtype=np.uint64) for _ in range(3)]
        for i in range(self.n_a):
            for j in range(self.n_b):
                v = val[a[:, i] & b[:, j]]
                out[0][i, j] = np.add.reduce(v.view(np.uint64), dtype=np.uint64) if v.size else 0
                out[1][i, j], out[2][i, j] = v.size, np.unique(v).size
        return out[0].view(np.int64), out[1], out[2]

    def moments(self, one_field: bool = False) -> MO.Moments:
        """moments_ref.brute over the filter's columns that both fields hold (one_field: that x holds)"""
        sh, pos = self.filter_columns
        xs, px = sparse_ints(self.Wfrag, self.base_rows, self.depth, sh, pos)
        if one_field:
            return MO.brute([x for x, p in zip(xs, px) if p], None)
        ys, py = sparse_ints(self.Wfrag, self.base_rows_y, self.depth, sh, pos)
        both = px & py
        return MO.brute([x for x, p in zip(xs, both) if p], [y for y, p in zip(ys, both) if p])

    def cube(self) -> np.ndarray:
        """uint64 [n_p, n_a, n_b]: the filter's columns counted by the rows of P, A and B that hold them"""
        sh, pos = self.filter_columns
        p, a, b = (sparse_rows(self.Warow, r, sh, pos).astype(np.int64) for r in (self.rows_p, self.rows_a, self.rows_b))
        return np.stack([(a * p[:, k:k + 1]).T @ b for k in range(self.n_p)]).astype(np.uint64)


# R of the sort-family calls and of fbk_extract_bsi: bit_depth + 2 field rows (+ 1 for an encoded filter)
SHORT = {
    "sort": dict(depth=64, dense={"filter"}, chunk_of=lambda n: chunk_extract(n, 66)),
    "sort_dense_field": dict(depth=20, dense={"bsi"}, chunk_of=lambda n: chunk_extract(n, 1)),
    "sort_all_encoded": dict(depth=64, dense=set(), chunk_of=lambda n: chunk_extract(n, 67)),
    "quantiles": dict(depth=64, dense={"filter"}, chunk_of=lambda n: chunk_extract(n, 66)),
    "distinct_rows": dict(depth=63, planes=24, dense={"filter"}, chunk_of=lambda n: chunk_extract(n, 65)),
    "extract_open": dict(depth=0, dense={"bsi"}, chunk_of=lambda n: chunk_extract(n, 1)),
    "extract_bsi": dict(depth=64, dense={"filter"}, chunk_of=lambda n: chunk_extract(n, 66)),
    "extract_rows": dict(depth=0, n_a=1024, dense={"filter", "bsi"}, chunk_of=lambda n: chunk_extract(n, 1024)),
    "groupby_sum": dict(depth=64, dense={"a"}, chunk_of=lambda n: chunk_msum(n, 1, 1, 64, 1 + 1 + 66)),
    "groupby_distinct": dict(depth=64, n_b=61, dense={"a"}, chunk_of=lambda n: chunk_mdist(n, 61 + 1 + 66)),
    # fbk_count_matrix_minmax: fbk_count_matrix_distinct's arithmetic; fbk_bsi_moments: R = the rows of x, of y and the filter's;
    # fbk_count_cube: the partial cube of a shard counts too (cube_ref.chunk), here 8 * 3 * 61 * 66 bytes beside 128 rows
    "groupby_minmax": dict(depth=64, planes=63, n_b=61, dense={"a"}, chunk_of=lambda n: chunk_mdist(n, 61 + 1 + 66)),
    "moments": dict(depth=64, y=True, dense=set(), chunk_of=lambda n: chunk_mdist(n, 66 + 66 + 1)),
    "moments_dense_y": dict(depth=64, y=True, dense={"y"}, chunk_of=lambda n: chunk_mdist(n, 66 + 1)),
    "groupby_cube": dict(depth=0, n_p=3, n_a=61, n_b=66, dense={"p"}, chunk_of=lambda n: CU.chunk(n, 3, 61, 66, True, False, False, False)),
}
# the stream of a case is its place in this list: the first ten in the order they had when they were all there was
SHORT_STREAM = ["distinct_rows", "extract_bsi", "extract_open", "extract_rows", "groupby_distinct", "groupby_sum", "quantiles", "sort", "sort_all_encoded",
                "sort_dense_field", "groupby_minmax", "moments", "moments_dense_y", "groupby_cube"]
