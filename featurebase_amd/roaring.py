"""Host-side driver of the fbk C ABI, named after the reference types it stands in for.

    Container  ~ roaring.Container          (roaring/container_stash.go:46-53)
    Batch      ~ a set of fragment.row()s   (fragment.go:283-333), device resident
    Plan       ~ one (query, node) batch of per-shard map calls (executor.go:6742)
    Context    ~ one GPU

This is test/bench plumbing over ctypes; all arithmetic happens in libfbk.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import lib as L

SLOTS = 16
BITMAP_WORDS = 1024


DESC_DTYPE = np.dtype(
    [("key", "<u8"), ("off", "<u8"), ("row", "<u4"), ("len", "<u4"), ("n", "<i4"), ("type", "u1"), ("pad", "u1", (3,))]
)  # == fbk_container_desc (include/fbk.h), 32 bytes


@dataclass
class Container:
    """One roaring container in its wire encoding (roaring.go:53-58)."""

    typ: int  # L.TYPE_ARRAY / TYPE_BITMAP / TYPE_RUN
    data: np.ndarray  # array: uint16[n]; bitmap: uint64[1024]; run: uint16[runs, 2] (start, last)
    n: int = -1  # cardinality, -1 = unknown (device recounts)

    @staticmethod
    def array(values: Iterable[int]) -> "Container":
        a = np.asarray(list(values) if not isinstance(values, np.ndarray) else values, dtype=np.uint16)
        return Container(L.TYPE_ARRAY, a, int(a.size))

    @staticmethod
    def bitmap(words: np.ndarray, n: int = -1) -> "Container":
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if w.size < BITMAP_WORDS:  # tests write short literals, like the reference's do
            w = np.concatenate([w, np.zeros(BITMAP_WORDS - w.size, dtype=np.uint64)])
        assert w.size == BITMAP_WORDS
        return Container(L.TYPE_BITMAP, w, n)

    @staticmethod
    def run(intervals: Iterable[Tuple[int, int]], n: int = -1) -> "Container":
        r = np.asarray(list(intervals), dtype=np.uint16).reshape(-1, 2)
        if n < 0:
            n = int((r[:, 1].astype(np.int64) - r[:, 0].astype(np.int64) + 1).sum()) if r.size else 0
        return Container(L.TYPE_RUN, r, n)

    @property
    def length(self) -> int:
        if self.typ == L.TYPE_ARRAY:
            return int(self.data.size)
        if self.typ == L.TYPE_RUN:
            return int(self.data.shape[0])
        return BITMAP_WORDS

    def payload(self) -> bytes:
        return np.ascontiguousarray(self.data).tobytes()

    def words(self) -> np.ndarray:
        """Bit content as uint64[1024] (representation independent, cf. BitwiseEqual
        roaring.go:6857-6922)."""
        if self.typ == L.TYPE_BITMAP:
            return self.data.copy()
        bits = np.zeros(65536, dtype=np.uint8)
        if self.typ == L.TYPE_ARRAY:
            bits[self.data.astype(np.int64)] = 1
        else:
            for s, l in self.data.astype(np.int64):
                bits[s : l + 1] = 1
        return np.packbits(bits, bitorder="little").view(np.uint64)


Row = Dict[int, Container]  # container key -> container; slot = key & 15


class Batch:
    def __init__(self, ctx: "Context", handle: int):
        self.ctx = ctx
        self.h = C.c_void_p(handle)
        self.owned = True  # False once handed to the device fragment cache

    def info(self) -> Tuple[int, int, int]:
        nr, nc, pb = C.c_uint32(), C.c_uint64(), C.c_uint64()
        L.check(self.ctx.lib.fbk_batch_info(self.ctx.h, self.h, C.byref(nr), C.byref(nc), C.byref(pb)))
        return nr.value, nc.value, pb.value

    @property
    def n_rows(self) -> int:
        return self.info()[0]

    def memory(self) -> Tuple[int, int, int]:
        """(arena bytes, heavy-row shadow bytes, shadow state 0 / 1 / 2) — fbk_batch_memory"""
        a, sh, st = C.c_uint64(), C.c_uint64(), C.c_int32()
        L.check(self.ctx.lib.fbk_batch_memory(self.ctx.h, self.h, C.byref(a), C.byref(sh), C.byref(st)))
        return a.value, sh.value, st.value

    def compact(self) -> int:
        """fbk_batch_compact: the containers into a right-sized arena; returns the arena bytes afterwards"""
        a = C.c_uint64()
        L.check(self.ctx.lib.fbk_batch_compact(self.ctx.h, self.h, C.byref(a)))
        return a.value

    def count(self, rows: Sequence[int]) -> np.ndarray:
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        out = np.zeros(r.size, dtype=np.uint64)
        L.check(self.ctx.lib.fbk_count(self.ctx.h, self.h, r.ctypes.data, r.size, out.ctypes.data))
        return out

    def download_flat(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """(descs, payload, n_rows): the batch in the flattened layout fbk_batch_upload takes — descs a
        structured array with the fields of fbk_container_desc, payload uint8."""
        n_rows, nc, pb = self.info()
        descs = np.zeros(max(nc, 1), dtype=DESC_DTYPE)
        payload = np.zeros(max(pb, 1), dtype=np.uint8)
        L.check(self.ctx.lib.fbk_batch_download(self.ctx.h, self.h, descs.ctypes.data_as(C.POINTER(L.ContainerDesc)), nc, payload.ctypes.data, pb))
        return descs[:nc], payload, n_rows

    def download(self) -> List[Row]:
        n_rows, nc, pb = self.info()
        descs = (L.ContainerDesc * max(nc, 1))()
        payload = np.zeros(max(pb, 1), dtype=np.uint8)
        L.check(self.ctx.lib.fbk_batch_download(self.ctx.h, self.h, descs, nc, payload.ctypes.data, pb))
        rows: List[Row] = [dict() for _ in range(n_rows)]
        for i in range(nc):
            d = descs[i]
            if d.type == L.TYPE_ARRAY:
                data = payload[d.off : d.off + 2 * d.len].view(np.uint16).copy()
            elif d.type == L.TYPE_RUN:
                data = payload[d.off : d.off + 4 * d.len].view(np.uint16).reshape(-1, 2).copy()
            else:
                data = payload[d.off : d.off + 8192].view(np.uint64).copy()
            rows[d.row][int(d.key)] = Container(int(d.type), data, int(d.n))
        return rows

    def to_roaring(self) -> bytes:
        """The batch in the Pilosa roaring format (Bitmap.WriteTo, roaring.go:1730)."""
        n = C.c_uint64()
        L.check(self.ctx.lib.fbk_batch_roaring_size(self.ctx.h, self.h, C.byref(n)))
        buf = np.zeros(max(n.value, 1), dtype=np.uint8)
        got = C.c_uint64()
        L.check(self.ctx.lib.fbk_batch_download_roaring(self.ctx.h, self.h, buf.ctypes.data, n.value, C.byref(got)))
        return buf[: got.value].tobytes()

    def free(self) -> None:
        if self.h and self.owned:
            L.check(self.ctx.lib.fbk_batch_free(self.ctx.h, self.h))
        self.h = C.c_void_p(None)


class Plan:
    def __init__(self, ctx: "Context", handle: int, n_pairs: int):
        self.ctx, self.h, self.n_pairs = ctx, C.c_void_p(handle), n_pairs

    def intersection_count(self) -> None:
        L.check(self.ctx.lib.fbk_plan_intersection_count(self.ctx.h, self.h))

    def intersection_count_total(self, device_ptr: int = 0) -> None:
        """Counts + per-node total in one launch (executeCount's mapFn + reduceFn)."""
        L.check(self.ctx.lib.fbk_plan_intersection_count_total(self.ctx.h, self.h, C.c_void_p(device_ptr or None)))

    def intersection_count_accumulate(self, device_ptr: int) -> None:
        """Counts + per-node reduce by accumulation into a zeroed uint64 at device_ptr (one launch)."""
        L.check(self.ctx.lib.fbk_plan_intersection_count_accumulate(self.ctx.h, self.h, C.c_void_p(device_ptr)))

    def setop(self, op: int, flags: int = 0) -> None:
        L.check(self.ctx.lib.fbk_plan_setop(self.ctx.h, self.h, op, flags))

    def total(self, device_ptr: int = 0) -> None:
        L.check(self.ctx.lib.fbk_plan_total(self.ctx.h, self.h, C.c_void_p(device_ptr or None)))

    def read(self, want_total: bool = False):
        counts = np.zeros(self.n_pairs, dtype=np.uint64)
        tot = C.c_uint64()
        L.check(
            self.ctx.lib.fbk_plan_read(
                self.ctx.h, self.h, counts.ctypes.data, C.cast(C.byref(tot), C.c_void_p) if want_total else None
            )
        )
        return (counts, tot.value) if want_total else counts

    def output(self) -> Batch:
        """Borrowed handle of the plan's set-op output (do not free)."""
        h = C.c_void_p()
        L.check(self.ctx.lib.fbk_plan_output(self.ctx.h, self.h, C.byref(h)))
        return Batch(self.ctx, h.value)

    def detach_output(self) -> Batch:
        """The plan's set-op output handed to the caller, who frees it; the plan's next setop makes a fresh one."""
        h = C.c_void_p()
        L.check(self.ctx.lib.fbk_plan_detach_output(self.ctx.h, self.h, C.byref(h)))
        return Batch(self.ctx, h.value)

    def free(self) -> None:
        if self.h:
            L.check(self.ctx.lib.fbk_plan_free(self.ctx.h, self.h))
            self.h = C.c_void_p(None)


class Query:
    """A prepared query (fbk_query_*): row lists and result buffers resident, every run launch-only."""

    def __init__(self, ctx: "Context", handle: int, kind: str, shape: Tuple[int, ...]):
        self.ctx, self.h, self.kind, self.shape = ctx, C.c_void_p(handle), kind, shape

    def run(self, device_ptr: int = 0, accumulate: bool = False) -> None:
        L.check(self.ctx.lib.fbk_query_run(self.ctx.h, self.h, C.c_void_p(device_ptr or None), L.QUERY_ACCUMULATE if accumulate else 0))

    def result_ptr(self) -> Tuple[int, int]:
        """(device pointer, bytes) of the query's own result buffer"""
        p, n = C.c_void_p(), C.c_uint64()
        L.check(self.ctx.lib.fbk_query_result(self.ctx.h, self.h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def read(self, per_shard: bool = False):
        if self.kind == "count_matrix":
            n_shards, n_a, n_b = self.shape
            tot = np.zeros((n_a, n_b), dtype=np.uint64)
            ps = np.zeros((n_shards, n_a, n_b), dtype=np.uint64) if per_shard else None
            L.check(self.ctx.lib.fbk_query_read(self.ctx.h, self.h, tot.ctypes.data, ps.ctypes.data if ps is not None else None))
            return (tot, ps) if per_shard else tot
        if self.kind == "count_matrix_sum":  # (sums [n_a, n_b] int64, counts [n_a, n_b] uint64)
            _, n_a, n_b = self.shape
            sums, counts = np.zeros((n_a, n_b), dtype=np.int64), np.zeros((n_a, n_b), dtype=np.uint64)
            L.check(self.ctx.lib.fbk_query_read(self.ctx.h, self.h, sums.ctypes.data, counts.ctypes.data))
            return sums, counts
        if self.kind in ("fold", "rows"):  # counts per group / cardinalities of the result rows
            out = np.zeros(self.shape[0], dtype=np.uint64)
            L.check(self.ctx.lib.fbk_query_read(self.ctx.h, self.h, out.ctypes.data, None))
            return out
        if self.kind == "topn":  # (row indexes, counts) of the results
            cap = self.shape[0]
            idx, cnt = np.zeros(1 + cap, dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint64)
            L.check(self.ctx.lib.fbk_query_read(self.ctx.h, self.h, idx.ctypes.data, cnt.ctypes.data))
            r = int(idx[0])
            return idx[1 : 1 + r].copy(), cnt[:r].copy()
        sums, counts = np.zeros(self.shape[0], dtype=np.int64), np.zeros(self.shape[0], dtype=np.uint64)
        L.check(self.ctx.lib.fbk_query_read(self.ctx.h, self.h, sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def output(self) -> "Batch":
        """The output batch of the last run (row-valued queries): BORROWED — do not free, valid until the next run."""
        h = C.c_void_p()
        L.check(self.ctx.lib.fbk_query_output(self.ctx.h, self.h, C.byref(h)))
        b = Batch(self.ctx, h.value)
        b.owned = False  # free() on the wrapper is a no-op: the query owns the batch
        return b

    def free(self) -> None:
        if self.h:
            L.check(self.ctx.lib.fbk_query_free(self.ctx.h, self.h))
            self.h = C.c_void_p(None)


class Extract:
    """The selected columns of Extract(filter, ...) (fbk_extract_*): fixed once by Context.extract, then one call per field.
    Keep the filter batch alive while the handle is, and close() it before the context."""

    def __init__(self, ctx: "Context", handle: int, n: int, n_shards: int, keep):
        self.ctx, self.h, self.n, self.n_shards, self._keep = ctx, C.c_void_p(handle), n, n_shards, keep

    def span(self) -> Tuple[int, int]:
        """(first, count): the shards (positions in the call's shard list) that hold a selected column"""
        a, b = C.c_uint32(), C.c_uint32()
        L.check(self.ctx.lib.fbk_extract_span(self.ctx.h, self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def columns(self) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.uint64)
        L.check(self.ctx.lib.fbk_extract_columns(self.ctx.h, self.h, out.ctypes.data))
        return out

    def bsi(self, batch: Batch, base_rows, bit_depth: int) -> Tuple[np.ndarray, np.ndarray]:
        """Int field: (values int64[n] — sign applied, Base not added, 0 where absent —, present bool[n])"""
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        assert base.size == self.n_shards
        vals, pres = np.zeros(self.n, dtype=np.int64), np.zeros(self.n, dtype=np.uint8)
        L.check(self.ctx.lib.fbk_extract_bsi(self.ctx.h, self.h, batch.h, base.ctypes.data, bit_depth, vals.ctypes.data, pres.ctypes.data))
        return vals, pres.astype(bool)

    def rows(self, batch: Batch, rows_a, cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Set field, rows_a [n_shards, n_a]: CSR (offsets uint64[n + 1], items uint32[m]): the items of column k are the
        indices i (ascending) of the rows that hold it.  One retry with the reported size when `cap` items were too few."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(self.n_shards, -1)
        offs, m = np.zeros(self.n + 1, dtype=np.uint64), C.c_uint64()
        cap = max(self.n, 1) if cap is None else cap
        for _ in range(2):
            items = np.zeros(max(cap, 1), dtype=np.uint32)
            rc = self.ctx.lib.fbk_extract_rows(self.ctx.h, self.h, batch.h, ra.ctypes.data, ra.shape[1], offs.ctypes.data, items.ctypes.data, cap, C.byref(m))
            if rc != L.FBK_E_CAPACITY:
                break
            cap = int(m.value)
        L.check(rc)
        return offs, items[: m.value].copy()

    def close(self) -> None:
        if self.h:
            L.check(self.ctx.lib.fbk_extract_free(self.ctx.h, self.h))
            self.h = C.c_void_p(None)

    def __enter__(self) -> "Extract":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class ExprLeaf:
    """One leaf of a bitmap call tree (fbk_expr_leaf): a row per shard of `batch`, or a BSI predicate over the shard's fragment."""

    def __init__(self, batch: Optional["Batch"], rows, kind: int = L.EXPR_ROW, op: int = 0, bit_depth: int = 0, lo: int = 0, hi: int = 0):
        self.batch, self.kind, self.op, self.bit_depth, self.lo, self.hi = batch, kind, op, bit_depth, lo, hi
        self.rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)


def row_leaf(batch: "Batch", rows) -> ExprLeaf:
    """rows[s] = ordinal of shard s's row in batch"""
    return ExprLeaf(batch, rows)


def bsi_leaf(batch: "Batch", base_rows, op: int, bit_depth: int, predicate: int) -> ExprLeaf:
    """Row(v op predicate): base_rows[s] = base row of shard s's BSI fragment (the row Context.bsi_range gives)"""
    return ExprLeaf(batch, base_rows, L.EXPR_BSI, op, bit_depth, predicate, 0)


def between_leaf(batch: "Batch", base_rows, bit_depth: int, lo: int, hi: int) -> ExprLeaf:
    """Row(lo <= v <= hi) (the row Context.bsi_range_between gives)"""
    return ExprLeaf(batch, base_rows, L.EXPR_BETWEEN, 0, bit_depth, lo, hi)


_EXPR_OPS = {"and": L.EXPR_AND, "or": L.EXPR_OR, "xor": L.EXPR_XOR, "andnot": L.EXPR_ANDNOT, "not": L.EXPR_ANDNOT}


def compile_expr(tree) -> Tuple[List[ExprLeaf], np.ndarray]:
    """A nested tuple such as ("and", ("or", leaf, leaf), ("andnot", exists, leaf), bsi_leaf) -> (leaves, postfix program) for
    Context.expr_count / expr_eval / query_expr.  An operator folds its operands left to right (("andnot", a, b, c) = a minus b minus c);
    ("not", exists, x) is ("andnot", exists, x), the way executeNotShard evaluates Not(x).  A leaf used twice is listed once."""
    leaves: List[ExprLeaf] = []
    index: dict = {}
    prog: List[int] = []

    def walk(t) -> None:
        if isinstance(t, ExprLeaf):
            if id(t) not in index:
                index[id(t)] = len(leaves)
                leaves.append(t)
            prog.append((L.EXPR_PUSH << 24) | index[id(t)])
            return
        name, args = t[0], t[1:]
        if name not in _EXPR_OPS or not args or (name == "not" and len(args) != 2):
            raise ValueError(f"compile_expr: bad node {name!r} with {len(args)} operands")
        walk(args[0])
        for a in args[1:]:
            walk(a)
            prog.append(_EXPR_OPS[name] << 24)

    walk(tree)
    return leaves, np.asarray(prog, dtype=np.uint32)


class GroupSelect:
    """having / sort / offset / limit of a GroupBy (fbk_groupby_select, include/fbk.h).
    sort: a reference-style string ("count desc, sum asc": getSorter, executor.go:3130-3162) or a list of (subject, desc) pairs;
    a term whose subject already occurred is dropped (it can never decide).  having: a reference-style condition string
    ("count > 5", "-5 < sum < 27", "sum >< [1, 9]") or (subject, op, lo[, hi]) with op one of OPS.  path: None, "device" or "host"."""

    SUBJECTS = {"count": L.GROUPSEL_COUNT, "sum": L.GROUPSEL_AGG, "aggregate": L.GROUPSEL_AGG}
    OPS = {"==": L.HAVING_EQ, "!=": L.HAVING_NEQ, "<": L.HAVING_LT, "<=": L.HAVING_LTE, ">": L.HAVING_GT, ">=": L.HAVING_GTE, "><": L.HAVING_BETWEEN,
           "<x<=": L.HAVING_BTWN_LT_LTE, "<=x<": L.HAVING_BTWN_LTE_LT, "<x<": L.HAVING_BTWN_LT_LT, "<=x<=": L.HAVING_BETWEEN}

    @staticmethod
    def parse_sort(spec: str) -> List[Tuple[int, bool]]:
        """getSorter's rules: terms split on commas, `count` | `sum` | `aggregate`, then `asc` | `desc` (default desc).  Raises
        ValueError with the reference's message."""
        terms = []
        for term in spec.split(","):
            term = term.strip()
            parts = term.split()
            if not parts:
                raise ValueError(f"invalid sorting directive: '{term}'")
            if parts[0] not in GroupSelect.SUBJECTS:
                raise ValueError(f"sorting is only supported on count, aggregate, or sum, not '{parts[0]}'")
            if len(parts) == 1:
                desc = True
            elif len(parts) > 2:
                raise ValueError(f"parsing sort directive: '{term}': too many elements")
            elif parts[1] in ("asc", "desc"):
                desc = parts[1] == "desc"
            else:
                raise ValueError(f"unknown sort direction '{parts[1]}'")
            terms.append((GroupSelect.SUBJECTS[parts[0]], desc))
        return terms

    @staticmethod
    def parse_condition(text: str) -> Tuple[int, int, int, int]:
        """Condition(count|sum <op> v), Condition(lo < sum <= hi), Condition(sum >< [lo, hi]) -> (subject, op, lo, hi)"""
        import re

        num, subj = r"(-?\d+)", r"(count|sum)"
        t = text.strip()
        m = re.fullmatch(rf"{num}\s*(<=?)\s*{subj}\s*(<=?)\s*{num}", t)
        if m:
            return GroupSelect.SUBJECTS[m.group(3)], GroupSelect.OPS[f"{m.group(2)}x{m.group(4)}"], int(m.group(1)), int(m.group(5))
        m = re.fullmatch(rf"{subj}\s*><\s*\[\s*{num}\s*,\s*{num}\s*\]", t)
        if m:
            return GroupSelect.SUBJECTS[m.group(1)], L.HAVING_BETWEEN, int(m.group(2)), int(m.group(3))
        m = re.fullmatch(rf"{subj}\s*(==|!=|<=|>=|<|>)\s*{num}", t)
        if m:
            return GroupSelect.SUBJECTS[m.group(1)], GroupSelect.OPS[m.group(2)], int(m.group(3)), 0
        raise ValueError(f"Condition() only supports count or sum against integers: '{text}'")

    def __init__(self, sort=None, having=None, offset: int = 0, limit: Optional[int] = None, path: Optional[str] = None):
        terms = self.parse_sort(sort) if isinstance(sort, str) else [(self.SUBJECTS.get(s, s), bool(d)) for s, d in (sort or [])]
        self.sort = []
        for s, d in terms:
            if all(s != s0 for s0, _ in self.sort):
                self.sort.append((s, d))
        if isinstance(having, str):
            having = self.parse_condition(having)
        elif having is not None:
            subject, op, lo = having[0], having[1], having[2]
            having = (self.SUBJECTS.get(subject, subject), self.OPS.get(op, op), int(lo), int(having[3]) if len(having) > 3 else 0)
        if having is not None and having[0] == L.GROUPSEL_COUNT:
            two = having[1] >= L.HAVING_BETWEEN
            if having[2] < 0 or (two and having[3] < 0):
                having = (L.GROUPSEL_COUNT, L.HAVING_BETWEEN, 1, 0)  # a negative literal in a count condition matches nothing (executor.go:3792-3795)
        self.having, self.offset, self.limit = having, int(offset), limit
        self.flags = {None: 0, "device": L.GROUPSEL_DEVICE, "host": L.GROUPSEL_HOST}[path]

    def struct(self) -> "L.GroupbySelect":
        s = L.GroupbySelect()
        s.flags, s.n_sort = self.flags, len(self.sort)
        for t, (subject, desc) in enumerate(self.sort[:2]):
            s.sort[t].subject, s.sort[t].desc = subject, int(desc)
        if self.having is not None:
            s.having_subject, s.having_op = self.having[0], self.having[1]
            wrap = lambda v: v - (1 << 64) if v >= (1 << 63) else v  # (a count bound is read as uint64)
            s.having_lo, s.having_hi = wrap(self.having[2]), wrap(self.having[3])
        s.offset, s.limit = self.offset, (1 << 64) - 1 if self.limit is None else self.limit
        return s


class Moments(NamedTuple):
    """Result of Context.bsi_moments: n and the five sums over the selected columns, Python ints (the sums signed, modulo 2^128)."""

    n: int
    sum_x: int
    sum_y: int
    sum_xx: int
    sum_yy: int
    sum_xy: int


def moments_shift(m: Moments, base_x: int, base_y: int = 0) -> Moments:
    """The moments of x + base_x and y + base_y from the raw ones (the four identities of include/fbk.h), in Python ints."""
    return Moments(
        m.n,
        m.sum_x + m.n * base_x,
        m.sum_y + m.n * base_y,
        m.sum_xx + 2 * base_x * m.sum_x + m.n * base_x * base_x,
        m.sum_yy + 2 * base_y * m.sum_y + m.n * base_y * base_y,
        m.sum_xy + base_y * m.sum_x + base_x * m.sum_y + m.n * base_x * base_y,
    )


def moments_var(m: Moments) -> Optional[int]:
    """SQL VAR(x) as the reference returns it: the population variance as a decimal of scale 6, truncated toward zero
    (aggregateVar.Eval, pql.FromFloat64WithScale).  n·Σx² − (Σx)² is exact; one division by n² in double.  None when n == 0:
    the reference then converts NaN to int64, which Go leaves unspecified."""
    if m.n == 0:
        return None
    return int(float(m.n * m.sum_xx - m.sum_x * m.sum_x) / float(m.n * m.n) * 1e6)


def moments_corr(m: Moments) -> Optional[int]:
    """SQL CORR(x, y) as the reference returns it: the expression of aggregateCorr.Eval in double, in its order of operations,
    from the moments converted to double; a decimal of scale 6, truncated toward zero.  None when n == 0 or when
    n·Σx² − (Σx)² or its y counterpart is zero (a constant column): the reference then converts NaN or Inf to int64, which Go
    leaves unspecified."""
    if m.n == 0:
        return None
    n, sx, sy, sxy, sxx, syy = float(m.n), float(m.sum_x), float(m.sum_y), float(m.sum_xy), float(m.sum_xx), float(m.sum_yy)
    under = (n * sxx - sx * sx) * (n * syy - sy * sy)
    if not under > 0 or math.isinf(under):
        return None
    return int((n * sxy - sx * sy) / math.sqrt(under) * 1e6)


class Context:
    """One GPU.  Fails loudly when libfbk.so is missing or no gfx950 device is visible."""

    def __init__(self, device: int = 0, _handle: Optional[int] = None, _borrowed: bool = False):
        self.lib = L.load()
        self.borrowed = _borrowed  # a group member: closed by the group
        if _handle is not None:
            self.h = C.c_void_p(_handle)
            return
        h = C.c_void_p()
        L.check(self.lib.fbk_open(device, 0, C.byref(h)))
        self.h = h

    def close(self) -> None:
        if self.h and not self.borrowed:
            L.check(self.lib.fbk_close(self.h))
        self.h = C.c_void_p(None)

    def fork(self) -> "Context":
        """A second context on the same device (own stream / lock / pool) for another calling
        thread; shares the fragment cache with this one (fbk_ctx_fork)."""
        h = C.c_void_p()
        L.check(self.lib.fbk_ctx_fork(self.h, C.byref(h)))
        return Context(_handle=h.value)

    def set_option(self, name: str, value: int) -> None:
        L.check(self.lib.fbk_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        L.check(self.lib.fbk_get_option(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def last_error(self) -> Tuple[int, str]:
        """(status code, message) of the last failing call on THIS context (fbk_last_error_r)."""
        buf = C.create_string_buffer(512)
        code = C.c_int32()
        L.check(self.lib.fbk_last_error_r(self.h, buf, 512, C.byref(code)))
        return int(code.value), buf.value.decode()

    def set_stream(self, hip_stream: int) -> None:
        L.check(self.lib.fbk_set_stream(self.h, C.c_void_p(hip_stream or None)))

    # ---- one process per GPU: the exchange issued by the library (fbk_comm_*) -------------------
    def comm_unique_id(self) -> bytes:
        """rank 0: the 128 bytes every rank passes to comm_init (hand them over with whatever channel the host has)"""
        buf = (C.c_uint8 * L.COMM_ID_BYTES)()
        L.check(self.lib.fbk_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, uid: bytes, n_ranks: int, rank: int) -> None:
        """collective: returns when every rank has called it"""
        assert len(uid) == L.COMM_ID_BYTES
        buf = (C.c_uint8 * L.COMM_ID_BYTES).from_buffer_copy(uid)
        L.check(self.lib.fbk_comm_init(self.h, buf, n_ranks, rank))

    def comm_all_reduce(self, device_ptr: int, n_words: int) -> None:
        """asynchronous in-place sum of n_words uint64 over the ranks: after what the context's stream holds, on the
        communicator's stream; the words must not be touched before comm_fence()"""
        L.check(self.lib.fbk_comm_all_reduce_u64(self.h, C.c_void_p(device_ptr), n_words))

    def comm_fence(self) -> None:
        L.check(self.lib.fbk_comm_fence(self.h))

    def comm_close(self) -> None:
        L.check(self.lib.fbk_comm_close(self.h))

    def synchronize(self) -> None:
        L.check(self.lib.fbk_synchronize(self.h))

    # -- residency ------------------------------------------------------------------
    def upload(self, rows: Sequence[Row]) -> Batch:
        """rows[i] maps container key -> Container (what fragment.row() yields)."""
        n_desc = sum(len(r) for r in rows)
        descs = (L.ContainerDesc * max(n_desc, 1))()
        chunks: List[bytes] = []
        off = 0
        i = 0
        for ri, row in enumerate(rows):
            for key, c in row.items():
                d = descs[i]
                d.key, d.off, d.row, d.len, d.n, d.type = key, off, ri, c.length, c.n, c.typ
                b = c.payload()
                chunks.append(b)
                off += len(b)
                i += 1
        payload = b"".join(chunks) or b"\0"
        h = C.c_void_p()
        L.check(self.lib.fbk_batch_upload(self.h, descs, n_desc, len(rows), payload, off, C.byref(h)))
        return Batch(self, h.value)

    def upload_flat(self, descs: np.ndarray, payload: np.ndarray, n_rows: int) -> Batch:
        """The flattened form directly: `descs` a structured array laid out as fbk_container_desc
        (32 bytes per record), `payload` the bytes its offsets point into."""
        d = np.ascontiguousarray(descs)
        assert d.dtype.itemsize == C.sizeof(L.ContainerDesc)
        pay = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        h = C.c_void_p()
        L.check(
            self.lib.fbk_batch_upload(
                self.h, C.cast(d.ctypes.data, C.POINTER(L.ContainerDesc)), d.size, n_rows, pay.ctypes.data, pay.size, C.byref(h)
            )
        )
        return Batch(self, h.value)

    def upload_roaring(self, data: bytes) -> Tuple[Batch, np.ndarray]:
        """A serialised roaring bitmap (Pilosa or official format) -> (batch, row ids): batch row
        i holds the containers with key >> 4 == row_ids[i] (Bitmap.UnmarshalBinary, roaring.go:1945)."""
        n = C.c_uint32()
        h = C.c_void_p()
        cap = max(len(data) // 2, 1)  # every container takes at least 2 payload bytes
        ids = np.zeros(cap, dtype=np.uint64)
        L.check(self.lib.fbk_batch_upload_roaring(self.h, data, len(data), C.byref(h), ids.ctypes.data, cap, C.byref(n)))
        return Batch(self, h.value), ids[: n.value].copy()

    def rbf_find_root(self, file_bytes: bytes, name: str) -> int:
        pg = C.c_uint32()
        L.check(self.lib.fbk_rbf_find_root(file_bytes, len(file_bytes), name.encode(), C.byref(pg)))
        return pg.value

    def upload_rbf(self, file_bytes: bytes, root_pgno: int) -> Tuple[Batch, np.ndarray]:
        """One bitmap b-tree of an RBF file image -> (batch, row ids) (rbf/tx.go ContainerIterator)."""
        n = C.c_uint32()
        h = C.c_void_p()
        cap = max(len(file_bytes) // 20, 1)  # a leaf cell takes at least 18 + 2 bytes
        ids = np.zeros(cap, dtype=np.uint64)
        L.check(self.lib.fbk_batch_upload_rbf(self.h, file_bytes, len(file_bytes), root_pgno, C.byref(h), ids.ctypes.data, cap, C.byref(n)))
        return Batch(self, h.value), ids[: n.value].copy()

    def upload_dense_device(self, device_ptr: int, n_rows: int) -> Batch:
        """n_rows dense rows (16 x 1024 uint64 each) that already sit in this device's memory at device_ptr
        (fbk_batch_upload_dense accepts a device source: the copy is device to device)."""
        h = C.c_void_p()
        L.check(self.lib.fbk_batch_upload_dense(self.h, C.c_void_p(device_ptr), n_rows, C.byref(h)))
        return Batch(self, h.value)

    def upload_dense(self, words: np.ndarray) -> Batch:
        w = np.ascontiguousarray(words, dtype=np.uint64)
        assert w.size % (SLOTS * BITMAP_WORDS) == 0
        n_rows = w.size // (SLOTS * BITMAP_WORDS)
        h = C.c_void_p()
        L.check(self.lib.fbk_batch_upload_dense(self.h, w.ctypes.data, n_rows, C.byref(h)))
        return Batch(self, h.value)

    # -- one-shot ops -----------------------------------------------------------------
    # -- device fragment cache ------------------------------------------------------------
    def cache_put(self, key: str, version: int, batch: Batch, row_ids) -> None:
        """The cache takes ownership of `batch` (do not free it)."""
        ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
        L.check(self.lib.fbk_cache_put(self.h, key.encode(), version, batch.h, ids.ctypes.data, ids.size))
        batch.owned = False

    def cache_get(self, key: str, version: int) -> Optional[Tuple[Batch, np.ndarray]]:
        """Pinned (batch, row ids) or None on a miss; call cache_release(batch) when done."""
        h, ids, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        rc = self.lib.fbk_cache_get(self.h, key.encode(), version, C.byref(h), C.byref(ids), C.byref(n))
        if rc == L.FBK_E_NOTFOUND:
            return None
        L.check(rc)
        b = Batch(self, h.value)
        b.owned = False
        rid = np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_uint64)), shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint64)
        return b, rid

    def cache_release(self, batch: Batch) -> None:
        L.check(self.lib.fbk_cache_release(self.h, batch.h))

    def cache_invalidate(self, key_prefix: str) -> int:
        n = C.c_uint32()
        L.check(self.lib.fbk_cache_invalidate(self.h, key_prefix.encode(), C.byref(n)))
        return n.value

    def cache_configure(self, cap_bytes: int) -> None:
        L.check(self.lib.fbk_cache_configure(self.h, cap_bytes))

    def cache_stats(self) -> dict:
        v = [C.c_uint64() for _ in range(5)]
        L.check(self.lib.fbk_cache_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("entries", "bytes", "hits", "misses", "evictions"), (x.value for x in v)))

    def intersection_count(self, a: Batch, rows_a, b: Batch, rows_b) -> np.ndarray:
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        rb = np.ascontiguousarray(rows_b, dtype=np.uint32)
        assert ra.size == rb.size
        out = np.zeros(ra.size, dtype=np.uint64)
        L.check(self.lib.fbk_intersection_count(self.h, a.h, ra.ctypes.data, b.h, rb.ctypes.data, ra.size, out.ctypes.data))
        return out

    def setop(self, op: int, a: Batch, rows_a, b: Batch, rows_b, flags: int = 0) -> Tuple[Batch, np.ndarray]:
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        rb = np.ascontiguousarray(rows_b, dtype=np.uint32)
        assert ra.size == rb.size
        out = np.zeros(ra.size, dtype=np.uint64)
        h = C.c_void_p()
        L.check(
            self.lib.fbk_setop(self.h, op, a.h, ra.ctypes.data, b.h, rb.ctypes.data, ra.size, flags, C.byref(h), out.ctypes.data)
        )
        return Batch(self, h.value), out

    # -- n-way union ------------------------------------------------------------------
    def union_n(self, batch: Batch, groups, flags: int = 0) -> Tuple[Batch, np.ndarray]:
        """groups: array [n_groups, k] of row ordinals; out row g = union of group g."""
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(len(groups), -1) if len(groups) else np.zeros((0, 0), np.uint32)
        n_groups, k = g.shape
        out = np.zeros(n_groups, dtype=np.uint64)
        h = C.c_void_p()
        L.check(self.lib.fbk_union_n(self.h, batch.h, g.ctypes.data, n_groups, k, flags, C.byref(h), out.ctypes.data))
        return Batch(self, h.value), out

    def union_n_intersection_count(self, batch: Batch, groups, filt: Optional[Batch] = None, rows_f=None) -> np.ndarray:
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(len(groups), -1)
        n_groups, k = g.shape
        out = np.zeros(n_groups, dtype=np.uint64)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        L.check(
            self.lib.fbk_union_n_intersection_count(
                self.h, batch.h, g.ctypes.data, n_groups, k, filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, out.ctypes.data
            )
        )
        return out

    def fold_n(self, op: int, batch: Batch, groups, flags: int = 0) -> Tuple[Batch, np.ndarray]:
        """groups: [n_groups, k] row ordinals; out row g = r0 <op> r1 <op> ... folded left to right
        (executeIntersect/Union/Xor/DifferenceShard, executor.go:5357, 5382, 5513, 2950)."""
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(len(groups), -1) if len(groups) else np.zeros((0, 0), np.uint32)
        n_groups, k = g.shape
        out = np.zeros(n_groups, dtype=np.uint64)
        h = C.c_void_p()
        L.check(self.lib.fbk_fold_n(self.h, op, batch.h, g.ctypes.data, n_groups, k, flags, C.byref(h), out.ctypes.data))
        return Batch(self, h.value), out

    def fold_n_intersection_count(self, op: int, batch: Batch, groups, filt: Optional[Batch] = None, rows_f=None) -> np.ndarray:
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(len(groups), -1)
        n_groups, k = g.shape
        out = np.zeros(n_groups, dtype=np.uint64)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        L.check(
            self.lib.fbk_fold_n_intersection_count(
                self.h, op, batch.h, g.ctypes.data, n_groups, k, filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, out.ctypes.data
            )
        )
        return out

    def topk(self, a: Batch, rows_a, k: int = 0, filt: Optional[Batch] = None, rows_f=None) -> Tuple[np.ndarray, np.ndarray]:
        """rows_a: [n_shards, n_a]; (row indices, counts) of the k rows with the largest
        |row ∩ filter| summed over the shards (count descending, index ascending; zeros dropped)."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        cap = n_a if k == 0 else min(k, n_a)
        idx = np.zeros(max(cap, 1), dtype=np.uint32)
        cnt = np.zeros(max(cap, 1), dtype=np.uint64)
        n = C.c_uint32()
        L.check(
            self.lib.fbk_topk(
                self.h, a.h, ra.ctypes.data, n_a, filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None,
                n_shards, k, idx.ctypes.data, cnt.ctypes.data, cap, C.byref(n),
            )
        )
        return idx[: n.value].copy(), cnt[: n.value].copy()

    def topn(self, a: Batch, rows_a, n: int = 0, filt: Optional[Batch] = None, rows_f=None, min_threshold: int = 0,
             tanimoto_threshold: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """fbk_topn: topk with fragment.top's MinThreshold / TanimotoThreshold rules (fragment.go:1317)."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        cap = n_a if n == 0 else min(n, n_a)
        idx = np.zeros(max(cap, 1), dtype=np.uint32)
        cnt = np.zeros(max(cap, 1), dtype=np.uint64)
        got = C.c_uint32()
        L.check(
            self.lib.fbk_topn(
                self.h, a.h, ra.ctypes.data, n_a, filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None,
                n_shards, n, min_threshold, tanimoto_threshold, idx.ctypes.data, cnt.ctypes.data, cap, C.byref(got),
            )
        )
        return idx[: got.value].copy(), cnt[: got.value].copy()

    def topn_partials(self, a: Optional[Batch], rows_a, n_a: int, n: int = 0, filt: Optional[Batch] = None, rows_f=None, min_threshold: int = 0,
                      tanimoto_threshold: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """fbk_topn_partials: (totals [n_a], candidate flags [n_a]) of THIS context's shards — what a rank of the
        one-process-per-GPU deployment hands to featurebase_amd.dist.topn_reduce.  a = None / no rows: zeros."""
        tot, cand = np.zeros(n_a, dtype=np.uint64), np.zeros(n_a, dtype=np.uint64)
        if a is None or rows_a is None or len(rows_a) == 0:
            return tot, cand
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        assert ra.ndim == 2 and ra.shape[1] == n_a
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        L.check(self.lib.fbk_topn_partials(self.h, a.h, ra.ctypes.data, n_a, filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None,
                                           ra.shape[0], n, min_threshold, tanimoto_threshold, tot.ctypes.data, cand.ctypes.data))
        return tot, cand

    def topk_bsi(self, a: Batch, rows_a, filt: Optional[Batch] = None, rows_f=None, flags: int = 0) -> Tuple[Batch, int]:
        """The TopK counts as BSI planes over the row indices (bsiBuilder, bsi.go:251): (batch of depth rows, depth)."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        h, depth = C.c_void_p(), C.c_uint32()
        L.check(self.lib.fbk_topk_bsi(self.h, a.h, ra.ctypes.data, n_a, filt.h if filt is not None else None,
                                      rf.ctypes.data if rf is not None else None, n_shards, flags, C.byref(h), C.byref(depth)))
        return Batch(self, h.value), int(depth.value)

    def flip(self, batch: Batch, rows, start: int, end: int, flags: int = 0) -> Tuple[Batch, np.ndarray]:
        """out row i = rows[i] with the bits of [start, end] (inclusive, row-relative) negated: Bitmap.Flip (roaring.go:2769)."""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        out = np.zeros(r.size, dtype=np.uint64)
        h = C.c_void_p()
        L.check(self.lib.fbk_flip(self.h, batch.h, r.ctypes.data, r.size, start, end, flags, C.byref(h), out.ctypes.data))
        return Batch(self, h.value), out

    NO_COLUMN = 0xFFFFFFFFFFFFFFFF

    def rows(self, batch: Batch, rows, column: Optional[int] = None, limit: int = 0, row_ids=None) -> np.ndarray:
        """fragment.rows (fragment.go:2465): positions (into `rows`, the fragment's rows in ascending row-id
        order) of the rows that hold anything / hold `column`, under the reference's limit rule (row_ids: the
        fragment row ids of `rows`, needed when a column and a limit are both given)."""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        ids = np.ascontiguousarray(row_ids, dtype=np.uint64) if row_ids is not None else None
        if ids is not None and ids.size != r.size:
            raise ValueError("row_ids must name every row")
        out = np.zeros(max(r.size, 1), dtype=np.uint32)
        n = C.c_uint64()
        L.check(self.lib.fbk_rows(self.h, batch.h, r.ctypes.data, ids.ctypes.data if ids is not None else None, r.size,
                                  self.NO_COLUMN if column is None else int(column), int(limit), out.ctypes.data, out.size, C.byref(n)))
        return out[: n.value].copy()

    NO_ROW = 0xFFFFFFFF

    def shift(self, batch: Batch, rows, carry_rows=None, flags: int = 0) -> Tuple[Batch, np.ndarray]:
        """out row i = rows[i] shifted up by one column, column 0 taken from the last column of
        carry_rows[i] (the previous shard's row); NO_ROW = absent (Row.Shift, row.go:374)."""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        cr = np.ascontiguousarray(carry_rows, dtype=np.uint32) if carry_rows is not None else None
        assert cr is None or cr.size == r.size
        out = np.zeros(r.size, dtype=np.uint64)
        h = C.c_void_p()
        L.check(self.lib.fbk_shift(self.h, batch.h, r.ctypes.data, cr.ctypes.data if cr is not None else None, r.size, flags, C.byref(h), out.ctypes.data))
        return Batch(self, h.value), out

    def count_range(self, batch: Batch, rows, start: int, end: int) -> np.ndarray:
        """out[i] = bits of rows[i] in [start, end), positions relative to the row (0..2^20):
        Bitmap.CountRange (roaring.go:573)."""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        out = np.zeros(r.size, dtype=np.uint64)
        L.check(self.lib.fbk_count_range(self.h, batch.h, r.ctypes.data, r.size, start, end, out.ctypes.data))
        return out

    # -- GroupBy / TopK count matrix -----------------------------------------------------
    def count_matrix(self, a: Batch, rows_a, b: Batch, rows_b, filt: Optional[Batch] = None, rows_f=None, per_shard: bool = False):
        """rows_a: [n_shards, n_a], rows_b: [n_shards, n_b], rows_f: [n_shards].
        Returns total [n_a, n_b] (and the per-shard [n_shards, n_a, n_b] if asked)."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        rb = np.ascontiguousarray(rows_b, dtype=np.uint32)
        n_shards, n_a = ra.shape
        n_b = rb.shape[1]
        assert rb.shape[0] == n_shards
        tot = np.zeros((n_a, n_b), dtype=np.uint64)
        ps = np.zeros((n_shards, n_a, n_b), dtype=np.uint64) if per_shard else None
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        L.check(
            self.lib.fbk_count_matrix(
                self.h, a.h, ra.ctypes.data, n_a, b.h, rb.ctypes.data, n_b,
                filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None,
                n_shards, tot.ctypes.data, ps.ctypes.data if ps is not None else None,
            )
        )
        return (tot, ps) if per_shard else tot

    # -- Extract -------------------------------------------------------------------------------
    def extract(self, filt: Batch, rows_f, shard_ids, offset: int = 0, limit: Optional[int] = None) -> Extract:
        """Extract(Limit(filter, limit=, offset=), ...): the filter's columns (rows_f [n_shards] of `filt`, shard_ids strictly
        ascending) in ascending order, ranks [offset, offset + limit).  Returns the handle (.n columns) the per-field calls take."""
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32)
        ids = np.ascontiguousarray(shard_ids, dtype=np.uint64)
        assert rf.size == ids.size
        h, n = C.c_void_p(), C.c_uint64()
        L.check(self.lib.fbk_extract_open(self.h, filt.h, rf.ctypes.data, ids.ctypes.data, rf.size, offset, (1 << 64) - 1 if limit is None else limit,
                                          C.byref(h), C.byref(n)))
        return Extract(self, h.value, int(n.value), int(rf.size), filt)

    def extract_columns(self, columns, shard_ids) -> Tuple[Extract, np.ndarray]:
        """Extract over an explicit column list (any order; fbk_extract_open_columns): (handle, rank) where rank[k] is the slot of
        columns[k] in the handle's ascending order, so `values[rank]` reads a per-field result in the order of the list."""
        cols = np.ascontiguousarray(columns, dtype=np.uint64)
        ids = np.ascontiguousarray(shard_ids, dtype=np.uint64)
        h, rank = C.c_void_p(), np.zeros(cols.size, dtype=np.uint32)
        L.check(self.lib.fbk_extract_open_columns(self.h, cols.ctypes.data, cols.size, ids.ctypes.data, ids.size, C.byref(h), rank.ctypes.data))
        return Extract(self, h.value, int(cols.size), int(ids.size), None), rank

    # -- Sort ----------------------------------------------------------------------------------
    def bsi_sort(self, batch: Batch, base_rows, bit_depth: int, shard_ids, filt: Optional[Batch] = None, rows_f=None, desc: bool = False,
                 keep_zero: bool = False, offset: int = 0, limit: Optional[int] = None, cap: Optional[int] = None):
        """Sort(filter, field=, sort-desc=, limit=, offset=) by an int field (fbk_bsi_sort): (columns uint64[n], values int64[n] —
        Base not added —, total = the columns that take part before offset / limit).  Equal values come in ascending column id.
        One retry with the reported size when `cap` records were too few."""
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        ids = np.ascontiguousarray(shard_ids, dtype=np.uint64)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        assert base.size == ids.size and (rf is None or rf.size == ids.size)
        flags = (L.SORT_DESC if desc else 0) | (L.SORT_KEEP_ZERO if keep_zero else 0)
        if cap is None:
            cap = 1 << 16 if limit is None else min(limit, 1 << 24)
        n, total = C.c_uint64(), C.c_uint64()
        for _ in range(2):
            cols, vals = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.int64)
            rc = self.lib.fbk_bsi_sort(self.h, batch.h, base.ctypes.data, bit_depth, filt.h if filt is not None else None,
                                       rf.ctypes.data if rf is not None else None, ids.ctypes.data, ids.size, flags, offset,
                                       (1 << 64) - 1 if limit is None else limit, cols.ctypes.data, vals.ctypes.data, cap, C.byref(n), C.byref(total))
            if rc != L.FBK_E_CAPACITY:
                break
            cap = int(n.value)
        L.check(rc)
        return cols[: n.value].copy(), vals[: n.value].copy(), int(total.value)

    # -- Quantiles / Percentile ----------------------------------------------------------------
    def _quant_args(self, batch: Batch, base_rows, bit_depth: int, filt: Optional[Batch], rows_f):
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        assert rf is None or rf.size == base.size
        args = (self.h, batch.h, base.ctypes.data, bit_depth, filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, base.size)
        return args, (base, rf)

    def bsi_quantiles(self, batch: Batch, base_rows, bit_depth: int, ranks, filt: Optional[Batch] = None, rows_f=None):
        """The values at several ranks of an int field over exists ∩ filter in one select (fbk_bsi_quantiles): with s the ascending
        values, rank k asks for s[k] and `lib.RANK_FROM_TOP | k` for s[N-1-k].  Returns (values int64 — Base not added —, counts
        uint64 = the columns holding exactly that value, total N).  A rank past the end gives (0, 0).  Stored zeros take part."""
        args, keep = self._quant_args(batch, base_rows, bit_depth, filt, rows_f)
        rk = np.ascontiguousarray(ranks, dtype=np.uint64).reshape(-1)
        vals, cnts, total = np.zeros(rk.size, dtype=np.int64), np.zeros(rk.size, dtype=np.uint64), C.c_uint64()
        L.check(self.lib.fbk_bsi_quantiles(*args, rk.ctypes.data, rk.size, vals.ctypes.data, cnts.ctypes.data, C.byref(total)))
        del keep
        return vals, cnts, int(total.value)

    def bsi_percentile(self, batch: Batch, base_rows, bit_depth: int, nth, base: int = 0, filt: Optional[Batch] = None, rows_f=None):
        """Percentile(field=, nth=, filter=) of an int field for a list of nth in one select (fbk_bsi_percentile): (values int64 —
        `base` added —, counts uint64, total N).  counts[i] == 0: the median of nothing (N == 0)."""
        args, keep = self._quant_args(batch, base_rows, bit_depth, filt, rows_f)
        pn = np.ascontiguousarray(nth, dtype=np.float64).reshape(-1)
        vals, cnts, total = np.zeros(pn.size, dtype=np.int64), np.zeros(pn.size, dtype=np.uint64), C.c_uint64()
        L.check(self.lib.fbk_bsi_percentile(*args, base, pn.ctypes.data, pn.size, vals.ctypes.data, cnts.ctypes.data, C.byref(total)))
        del keep
        return vals, cnts, int(total.value)

    # -- GroupBy over three fields -------------------------------------------------------------
    def count_cube(self, p: Batch, rows_p, a: Batch, rows_a, b: Batch, rows_b, filt: Optional[Batch] = None, rows_f=None) -> np.ndarray:
        """GroupBy(Rows(p), Rows(a), Rows(b)) in one pass (fbk_count_cube): for every triple the count of P_p ∩ A_i ∩ B_j ∩ filt,
        summed over the shards.  rows_p [n_shards, n_p], rows_a [n_shards, n_a], rows_b [n_shards, n_b], rows_f [n_shards].
        Returns uint64 [n_p, n_a, n_b]; a zero is a group the reference skips."""
        rp = np.ascontiguousarray(rows_p, dtype=np.uint32)
        n_shards, n_p = rp.shape
        ra, rb = np.ascontiguousarray(rows_a, dtype=np.uint32), np.ascontiguousarray(rows_b, dtype=np.uint32)
        assert ra.ndim == 2 and rb.ndim == 2 and ra.shape[0] == n_shards and rb.shape[0] == n_shards
        n_a, n_b = ra.shape[1], rb.shape[1]
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        assert rf is None or rf.size == n_shards
        out = np.zeros((n_p, n_a, n_b), dtype=np.uint64)
        L.check(self.lib.fbk_count_cube(self.h, p.h, rp.ctypes.data, n_p, a.h, ra.ctypes.data, n_a, b.h, rb.ctypes.data, n_b,
                                        filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, n_shards, out.ctypes.data))
        return out

    # -- GroupBy with aggregate=Sum ------------------------------------------------------------
    def _msum_args(self, a: Batch, rows_a, b: Optional[Batch], rows_b, bsi: Batch, base_rows, filt: Optional[Batch], rows_f):
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        rb = np.ascontiguousarray(rows_b, dtype=np.uint32).reshape(n_shards, -1) if b is not None else None
        n_b = rb.shape[1] if rb is not None else 1
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        assert base.size == n_shards
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        args = (self.h, a.h, ra.ctypes.data, n_a, b.h if b is not None else None, rb.ctypes.data if rb is not None else None, n_b,
                filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, bsi.h, base.ctypes.data)
        return args, (ra, rb, base, rf), n_shards, n_a, n_b

    def count_matrix_sum(self, a: Batch, rows_a, b: Optional[Batch], rows_b, bsi: Batch, base_rows, bit_depth: int,
                         filt: Optional[Batch] = None, rows_f=None) -> Tuple[np.ndarray, np.ndarray]:
        """GroupBy(..., aggregate=Sum(field)) of the last two levels: for every pair (i, j) the BSI sum and the count over
        A_i ∩ B_j ∩ filt ∩ exists, summed over the shards (b = None: the one-field form, one column).
        rows_a [n_shards, n_a], rows_b [n_shards, n_b], base_rows / rows_f [n_shards].  Returns (sums int64, counts uint64),
        both [n_a, n_b]; the caller adds count * Base."""
        args, keep, n_shards, n_a, n_b = self._msum_args(a, rows_a, b, rows_b, bsi, base_rows, filt, rows_f)
        sums, counts = np.zeros((n_a, n_b), dtype=np.int64), np.zeros((n_a, n_b), dtype=np.uint64)
        L.check(self.lib.fbk_count_matrix_sum(*args, bit_depth, n_shards, sums.ctypes.data, counts.ctypes.data))
        del keep
        return sums, counts

    def query_count_matrix_sum(self, a: Batch, rows_a, b: Optional[Batch], rows_b, bsi: Batch, base_rows, bit_depth: int,
                               filt: Optional[Batch] = None, rows_f=None) -> Query:
        """count_matrix_sum as a prepared, launch-only query; read() returns (sums, counts)"""
        args, keep, n_shards, n_a, n_b = self._msum_args(a, rows_a, b, rows_b, bsi, base_rows, filt, rows_f)
        h = C.c_void_p()
        L.check(self.lib.fbk_query_count_matrix_sum(*args, bit_depth, n_shards, C.byref(h)))
        del keep
        return Query(self, h.value, "count_matrix_sum", (n_shards, n_a, n_b))

    def count_matrix_distinct(self, a: Batch, rows_a, b: Optional[Batch], rows_b, bsi: Batch, base_rows, bit_depth: int,
                              filt: Optional[Batch] = None, rows_f=None) -> Tuple[np.ndarray, np.ndarray]:
        """GroupBy(..., aggregate=Count(Distinct(field))) of the last two levels: for every pair (i, j) the number of distinct
        stored values over A_i ∩ B_j ∩ filt ∩ exists, taken over all the shards together, and the number of such columns
        (b = None: the one-field form, one column).  Arguments as count_matrix_sum.  Returns (distinct, counts), both uint64
        [n_a, n_b]."""
        args, keep, n_shards, n_a, n_b = self._msum_args(a, rows_a, b, rows_b, bsi, base_rows, filt, rows_f)
        distinct, counts = np.zeros((n_a, n_b), dtype=np.uint64), np.zeros((n_a, n_b), dtype=np.uint64)
        L.check(self.lib.fbk_count_matrix_distinct(*args, bit_depth, n_shards, distinct.ctypes.data, counts.ctypes.data))
        del keep
        return distinct, counts

    def count_matrix_minmax(self, a: Batch, rows_a, b: Optional[Batch], rows_b, bsi: Batch, base_rows, bit_depth: int,
                            filt: Optional[Batch] = None, rows_f=None, counts: bool = True, path: int = 0):
        """GroupBy with Min / Max of an int field per group (SQL MIN(x), MAX(x) ... GROUP BY a, b): for every pair (i, j) the
        smallest and the largest stored value over A_i ∩ B_j ∩ filt ∩ exists, taken over all the shards together, and how many
        columns hold each (b = None: the one-field form, one column).  Arguments as count_matrix_sum; path: L.MINMAX_AUTO,
        _DESCENT (at most 1024 groups) or _SCATTER.  Returns (mins int64, maxs int64, min_counts, max_counts uint64), all
        [n_a, n_b]; the count arrays are None with counts=False.  An empty group is (INT64_MAX, INT64_MIN, 0, 0); the caller adds Base."""
        args, keep, n_shards, n_a, n_b = self._msum_args(a, rows_a, b, rows_b, bsi, base_rows, filt, rows_f)
        mins, maxs = np.zeros((n_a, n_b), dtype=np.int64), np.zeros((n_a, n_b), dtype=np.int64)
        cmin = np.zeros((n_a, n_b), dtype=np.uint64) if counts else None
        cmax = np.zeros((n_a, n_b), dtype=np.uint64) if counts else None
        L.check(self.lib.fbk_count_matrix_minmax(*args, bit_depth, n_shards, path, mins.ctypes.data, maxs.ctypes.data,
                                                 cmin.ctypes.data if counts else None, cmax.ctypes.data if counts else None))
        del keep
        return mins, maxs, cmin, cmax

    def count_matrix_quantiles(self, a: Batch, rows_a, b: Optional[Batch], rows_b, bsi: Batch, base_rows, bit_depth: int, fractions,
                               filt: Optional[Batch] = None, rows_f=None, path: int = 0):
        """GroupBy with a percentile of an int field per group (SQL PERCENTILE_DISC(x, num / den) ... GROUP BY a, b): for every pair
        (i, j) and every (num, den) of `fractions` the value s[max(1, ceil(N * num / den)) - 1] of the ascending stored values over
        A_i ∩ B_j ∩ filt ∩ exists, taken over all the shards together, and how many columns hold exactly it (b = None: the
        one-field form, one column).  Arguments as count_matrix_sum; at most 16 fractions, den <= 2^20; path: L.GQUANT_AUTO, _LDS
        (few groups) or _GLOBAL.  Returns (values int64 [n_a, n_b, n_q], counts uint64 [n_a, n_b, n_q], totals uint64 [n_a, n_b]);
        an empty group is (0, 0) with total 0; the caller adds Base.  No fractions: the totals alone."""
        args, keep, n_shards, n_a, n_b = self._msum_args(a, rows_a, b, rows_b, bsi, base_rows, filt, rows_f)
        fr = np.ascontiguousarray(fractions, dtype=np.uint32).reshape(-1, 2)
        n_q = fr.shape[0]
        num, den = np.ascontiguousarray(fr[:, 0]), np.ascontiguousarray(fr[:, 1])
        vals, cnts = np.zeros((n_a, n_b, n_q), dtype=np.int64), np.zeros((n_a, n_b, n_q), dtype=np.uint64)
        totals = np.zeros((n_a, n_b), dtype=np.uint64)
        L.check(self.lib.fbk_count_matrix_quantiles(*args, bit_depth, n_shards, num.ctypes.data if n_q else None, den.ctypes.data if n_q else None, n_q, path,
                                                    vals.ctypes.data if n_q else None, cnts.ctypes.data if n_q else None, totals.ctypes.data))
        del keep
        return vals, cnts, totals

    # -- GroupBy having / sort / offset / limit ---------------------------------------------------
    def _select(self, call, args, sel, has_agg: bool, cap: Optional[int], aggs_slot: bool = True):
        """`call`(*args, sel, out_cells, out_counts[, out_aggs], cap, out_n, out_matched), one retry with the reported size when
        `cap` records were too few (as bsi_sort).  aggs_slot: the call has an out_aggs argument even when has_agg is false (NULL then)."""
        st = sel.struct() if isinstance(sel, GroupSelect) else sel
        if cap is None:
            cap = 1 << 16 if st.limit == (1 << 64) - 1 else min(int(st.limit), 1 << 24)
        n, matched = C.c_uint64(), C.c_uint64()
        for _ in range(2):
            cells, counts = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint64)
            aggs = np.zeros(max(cap, 1), dtype=np.int64) if has_agg else None
            outs = (cells.ctypes.data, counts.ctypes.data) + ((aggs.ctypes.data,) if has_agg else (None,) if aggs_slot else ())
            rc = call(*args, C.byref(st), *outs, cap, C.byref(n), C.byref(matched))
            if rc != L.FBK_E_CAPACITY:
                break
            cap = int(n.value)
        L.check(rc)
        k = int(n.value)
        if has_agg:
            return cells[:k].copy(), counts[:k].copy(), aggs[:k].copy(), int(matched.value)
        return cells[:k].copy(), counts[:k].copy(), int(matched.value)

    def count_matrix_select(self, a: Batch, rows_a, b: Batch, rows_b, sel, filt: Optional[Batch] = None, rows_f=None, cap: Optional[int] = None):
        """count_matrix's groups through having / sort / offset / limit on the device (fbk_count_matrix_select): (cells uint32 —
        cell = i * n_b + j —, counts uint64, matched = the groups before offset / limit).  sel: a GroupSelect."""
        ra, rb = np.ascontiguousarray(rows_a, dtype=np.uint32), np.ascontiguousarray(rows_b, dtype=np.uint32)
        n_shards, n_a = ra.shape
        assert rb.shape[0] == n_shards
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        args = (self.h, a.h, ra.ctypes.data, n_a, b.h, rb.ctypes.data, rb.shape[1], filt.h if filt is not None else None,
                rf.ctypes.data if rf is not None else None, n_shards)
        return self._select(self.lib.fbk_count_matrix_select, args, sel, False, cap, aggs_slot=False)

    def count_cube_select(self, p: Batch, rows_p, a: Batch, rows_a, b: Batch, rows_b, sel, filt: Optional[Batch] = None, rows_f=None, cap: Optional[int] = None):
        """count_cube's groups through having / sort / offset / limit on the device (fbk_count_cube_select): (cells uint32 —
        cell = (p * n_a + i) * n_b + j —, counts uint64, matched)."""
        rp, ra, rb = (np.ascontiguousarray(r, dtype=np.uint32) for r in (rows_p, rows_a, rows_b))
        n_shards, n_p = rp.shape
        assert ra.ndim == 2 and rb.ndim == 2 and ra.shape[0] == n_shards and rb.shape[0] == n_shards
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        args = (self.h, p.h, rp.ctypes.data, n_p, a.h, ra.ctypes.data, ra.shape[1], b.h, rb.ctypes.data, rb.shape[1],
                filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, n_shards)
        return self._select(self.lib.fbk_count_cube_select, args, sel, False, cap, aggs_slot=False)

    def count_matrix_sum_select(self, a: Batch, rows_a, b: Optional[Batch], rows_b, bsi: Batch, base_rows, bit_depth: int, sel,
                                filt: Optional[Batch] = None, rows_f=None, cap: Optional[int] = None):
        """count_matrix_sum's groups through having / sort / offset / limit on the device (fbk_count_matrix_sum_select): (cells
        uint32, counts uint64, sums int64 — Base not added —, matched)."""
        args, keep, n_shards, n_a, n_b = self._msum_args(a, rows_a, b, rows_b, bsi, base_rows, filt, rows_f)
        out = self._select(self.lib.fbk_count_matrix_sum_select, args + (bit_depth, n_shards), sel, True, cap)
        del keep
        return out

    def select_groups(self, counts, aggs, sel, cap: Optional[int] = None):
        """The selection stage alone over host arrays counts [n] and aggs [n] or None (fbk_select_groups): (cells, counts[, aggs],
        matched) — aggs only when given."""
        c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        g = np.ascontiguousarray(aggs, dtype=np.int64).reshape(-1) if aggs is not None else None
        assert g is None or g.size == c.size
        return self._select(self.lib.fbk_select_groups, (self.h, c.ctypes.data, g.ctypes.data if g is not None else None, c.size), sel, g is not None, cap)

    # -- prepared (launch-only) forms of the query-level calls -------------------------------
    def prepare_count_matrix(self, a: Batch, rows_a, b: Batch, rows_b, filt: Optional[Batch] = None, rows_f=None, keep_per_shard: bool = False) -> Query:
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        rb = np.ascontiguousarray(rows_b, dtype=np.uint32)
        n_shards, n_a = ra.shape
        n_b = rb.shape[1]
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        h = C.c_void_p()
        L.check(self.lib.fbk_query_count_matrix(self.h, a.h, ra.ctypes.data, n_a, b.h, rb.ctypes.data, n_b, filt.h if filt is not None else None,
                                                rf.ctypes.data if rf is not None else None, n_shards, 1 if keep_per_shard else 0, C.byref(h)))
        return Query(self, h.value, "count_matrix", (n_shards, n_a, n_b))

    def prepare_fold_intersection_count(self, op: int, batch: Batch, groups, filt: Optional[Batch] = None, rows_f=None) -> Query:
        g = np.ascontiguousarray(groups, dtype=np.uint32)
        g = g.reshape(len(groups), -1)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        h = C.c_void_p()
        L.check(self.lib.fbk_query_fold_intersection_count(self.h, op, batch.h, g.ctypes.data, g.shape[0], g.shape[1], filt.h if filt is not None else None,
                                                           rf.ctypes.data if rf is not None else None, C.byref(h)))
        return Query(self, h.value, "fold", (g.shape[0],))

    def prepare_bsi_sum(self, batch: Batch, base_rows, bit_depth: int, op: int = 0, predicate: int = 0, filt: Optional[Batch] = None, rows_f=None) -> Query:
        """op == 0: Sum over exists ∩ filt; op = BSI_*: Sum(Row(v op predicate), field = v) in one pass"""
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        h = C.c_void_p()
        L.check(self.lib.fbk_query_bsi_sum(self.h, batch.h, base.ctypes.data, base.size, bit_depth, op, C.c_int64(predicate), filt.h if filt is not None else None,
                                           rf.ctypes.data if rf is not None else None, C.byref(h)))
        return Query(self, h.value, "bsi", (base.size,))

    def prepare_bsi_range(self, batch: Batch, base_rows, op: int, bit_depth: int, predicate: int) -> Query:
        """Row(v op predicate) with the result rows kept on the device (Query.output()); read() = their cardinalities"""
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        h = C.c_void_p()
        L.check(self.lib.fbk_query_bsi_range(self.h, batch.h, base.ctypes.data, base.size, op, bit_depth, C.c_int64(predicate), C.byref(h)))
        return Query(self, h.value, "rows", (base.size,))

    def prepare_fold(self, op: int, batch: Batch, groups, flags: int = 0) -> Query:
        """The materialised n-way Union / Xor / Difference (fbk_fold_n) as a launch-only query; read() = cardinalities"""
        g = np.ascontiguousarray(groups, dtype=np.uint32)
        h = C.c_void_p()
        L.check(self.lib.fbk_query_fold(self.h, op, batch.h, g.ctypes.data, g.shape[0], g.shape[1], flags, C.byref(h)))
        return Query(self, h.value, "rows", (g.shape[0],))

    def prepare_topn(self, a: Batch, rows_a, n: int = 0, filt: Optional[Batch] = None, rows_f=None, min_threshold: int = 0, tanimoto_threshold: int = 0) -> Query:
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        h = C.c_void_p()
        L.check(self.lib.fbk_query_topn(self.h, a.h, ra.ctypes.data, n_a, filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, n_shards, n,
                                        min_threshold, tanimoto_threshold, C.byref(h)))
        return Query(self, h.value, "topn", (min(n, n_a) if n else n_a,))

    # -- BSI -----------------------------------------------------------------------------
    def bsi_sum(self, batch: Batch, base_rows, bit_depth: int, filt: Optional[Batch] = None, rows_f=None):
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        sums = np.zeros(base.size, dtype=np.int64)
        counts = np.zeros(base.size, dtype=np.uint64)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        L.check(
            self.lib.fbk_bsi_sum(
                self.h, batch.h, base.ctypes.data, base.size, bit_depth,
                filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, sums.ctypes.data, counts.ctypes.data,
            )
        )
        return sums, counts

    def bsi_moments(self, x: Batch, base_rows_x, depth_x: int, y: Optional[Batch] = None, base_rows_y=None, depth_y: int = 0,
                    filt: Optional[Batch] = None, rows_f=None) -> Moments:
        """n, Σx, Σy, Σx², Σy², Σxy over exists_x ∩ exists_y ∩ filter of all the shards given (fbk_bsi_moments): what SQL VAR
        and CORR are functions of (moments_var, moments_corr).  y is None: the one-field form.  Base is not applied (moments_shift)."""
        bx = np.ascontiguousarray(base_rows_x, dtype=np.uint32)
        by = np.ascontiguousarray(base_rows_y, dtype=np.uint32) if y is not None else None
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        assert (by is None or by.size == bx.size) and (rf is None or rf.size == bx.size)
        out = L.Moments()
        L.check(
            self.lib.fbk_bsi_moments(
                self.h, x.h, bx.ctypes.data, depth_x, y.h if y is not None else None, by.ctypes.data if by is not None else None, depth_y,
                filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, bx.size, C.byref(out),
            )
        )
        return Moments(int(out.n), int(out.sum_x), int(out.sum_y), int(out.sum_xx), int(out.sum_yy), int(out.sum_xy))

    def bsi_compare(self, x: Batch, base_rows_x, depth_x: int, base_x: int, y: Batch, base_rows_y, depth_y: int, base_y: int, op: int,
                    filt: Optional[Batch] = None, rows_f=None, flags: int = 0, count_only: bool = False) -> Tuple[Optional[Batch], np.ndarray]:
        """The Row of `value_x op value_y` per shard over exists_x ∩ exists_y ∩ filter (fbk_bsi_compare), values exact integers
        (sign ? -magnitude : magnitude) + base: SQL WHERE x < y.  Returns (batch, counts) as bsi_range does; count_only: (None, counts)
        with no output written on the device."""
        bx = np.ascontiguousarray(base_rows_x, dtype=np.uint32)
        by = np.ascontiguousarray(base_rows_y, dtype=np.uint32)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        assert by.size == bx.size and (rf is None or rf.size == bx.size)
        counts = np.zeros(bx.size, dtype=np.uint64)
        h = C.c_void_p()
        L.check(
            self.lib.fbk_bsi_compare(
                self.h, x.h, bx.ctypes.data, depth_x, C.c_int64(base_x), y.h, by.ctypes.data, depth_y, C.c_int64(base_y), op,
                filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, bx.size, flags,
                None if count_only else C.byref(h), counts.ctypes.data,
            )
        )
        return (None if count_only else Batch(self, h.value)), counts

    def _bsi_minmax(self, fn, batch: Batch, base_rows, bit_depth: int, filt: Optional[Batch], rows_f):
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        vals = np.zeros(base.size, dtype=np.int64)
        counts = np.zeros(base.size, dtype=np.uint64)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        L.check(
            fn(
                self.h, batch.h, base.ctypes.data, base.size, bit_depth,
                filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None, vals.ctypes.data, counts.ctypes.data,
            )
        )
        return vals, counts

    def bsi_min(self, batch: Batch, base_rows, bit_depth: int, filt: Optional[Batch] = None, rows_f=None):
        """Per shard (min, count): fragment.min (fragment.go:754)."""
        return self._bsi_minmax(self.lib.fbk_bsi_min, batch, base_rows, bit_depth, filt, rows_f)

    def bsi_max(self, batch: Batch, base_rows, bit_depth: int, filt: Optional[Batch] = None, rows_f=None):
        """Per shard (max, count): fragment.max (fragment.go:803)."""
        return self._bsi_minmax(self.lib.fbk_bsi_max, batch, base_rows, bit_depth, filt, rows_f)

    def bsi_distinct(self, batch: Batch, base_rows, bit_depth: int, filt: Optional[Batch] = None, rows_f=None) -> np.ndarray:
        """Sorted distinct stored values (int64, Base not added) of the columns in exists ∩ filter
        over all given shards (executeDistinctShardBSI, executor.go:2034)."""
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        n = C.c_uint64()
        cap = 1 << 16
        while True:
            out = np.zeros(cap, dtype=np.int64)
            rc = self.lib.fbk_bsi_distinct(self.h, batch.h, base.ctypes.data, base.size, bit_depth, filt.h if filt is not None else None,
                                           rf.ctypes.data if rf is not None else None, out.ctypes.data, cap, C.byref(n))
            if rc == L.FBK_E_CAPACITY:
                cap = int(n.value)
                continue
            L.check(rc)
            return out[: n.value].copy()

    def bsi_distinct_rows(self, batch: Batch, base_rows, bit_depth: int, base: int = 0, filt: Optional[Batch] = None, rows_f=None, flags: int = 0,
                          cap: Optional[int] = None) -> Tuple[Batch, np.ndarray, np.ndarray, np.ndarray]:
        """Distinct(filter, field=) of an int field as a device Row (fbk_bsi_distinct_rows): the columns of the result are the
        values + `base`, Pos for v >= 0 and Neg for -v of v < 0.  Returns (batch, pos_shards, neg_shards, counts): rows
        [0, len(pos_shards)) of the batch are Pos's shards, the next len(neg_shards) Neg's, one empty row follows; counts per row.
        One retry with the reported size when `cap` rows were too few."""
        rows = np.ascontiguousarray(base_rows, dtype=np.uint32)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        assert rf is None or rf.size == rows.size
        cap = 64 if cap is None else cap
        h, n_pos, n_neg = C.c_void_p(), C.c_uint32(), C.c_uint32()
        for _ in range(2):
            ids, counts = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
            rc = self.lib.fbk_bsi_distinct_rows(self.h, batch.h, rows.ctypes.data, bit_depth, base, filt.h if filt is not None else None,
                                                rf.ctypes.data if rf is not None else None, rows.size, flags, C.byref(h), ids.ctypes.data, cap,
                                                C.byref(n_pos), C.byref(n_neg), counts.ctypes.data)
            if rc != L.FBK_E_CAPACITY:
                break
            cap = n_pos.value + n_neg.value
        L.check(rc)
        n = n_pos.value + n_neg.value
        return Batch(self, h.value), ids[: n_pos.value].copy(), ids[n_pos.value : n].copy(), counts[:n].copy()

    def bsi_add(self, x: Batch, rows_x, y: Batch, rows_y, flags: int = 0) -> Batch:
        """rows_x: [n_groups, depth_x], rows_y: [n_groups, depth_y] plane rows (bit i = column i);
        out rows g*(D+1)+i = plane i of x + y (roaring.Add, roaring/add.go:12)."""
        rx = np.ascontiguousarray(rows_x, dtype=np.uint32).reshape(len(rows_x), -1)
        ry = np.ascontiguousarray(rows_y, dtype=np.uint32).reshape(len(rows_y), -1)
        assert rx.shape[0] == ry.shape[0]
        h = C.c_void_p()
        L.check(self.lib.fbk_bsi_add(self.h, x.h, rx.ctypes.data, rx.shape[1], y.h, ry.ctypes.data, ry.shape[1], rx.shape[0], flags, C.byref(h)))
        return Batch(self, h.value)

    def bsi_range(self, batch: Batch, base_rows, op: int, bit_depth: int, predicate: int, flags: int = 0) -> Tuple[Batch, np.ndarray]:
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        counts = np.zeros(base.size, dtype=np.uint64)
        h = C.c_void_p()
        L.check(self.lib.fbk_bsi_range(self.h, batch.h, base.ctypes.data, base.size, op, bit_depth, predicate, flags, C.byref(h), counts.ctypes.data))
        return Batch(self, h.value), counts

    def bsi_range_sum(self, batch: Batch, base_rows, op: int, bit_depth: int, predicate: int, filt: Optional[Batch] = None, rows_f=None):
        """Sum(Row(v op predicate), field = v) in one pass over the planes: (sums int64[n_shards], counts uint64[n_shards]),
        equal to bsi_sum with filter = bsi_range(op, predicate) (∩ filt)."""
        b = np.ascontiguousarray(base_rows, dtype=np.uint32)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        sums = np.zeros(b.size, dtype=np.int64)
        counts = np.zeros(b.size, dtype=np.uint64)
        L.check(self.lib.fbk_bsi_range_sum(self.h, batch.h, b.ctypes.data, b.size, op, bit_depth, C.c_int64(predicate),
                                           filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None,
                                           sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def bsi_range_between_sum(self, batch: Batch, base_rows, bit_depth: int, lo: int, hi: int, filt: Optional[Batch] = None, rows_f=None):
        """Sum(Row(lo <= v <= hi), field = v): (sums, counts) per shard, equal to bsi_sum over bsi_range_between (∩ filt)."""
        b = np.ascontiguousarray(base_rows, dtype=np.uint32)
        rf = np.ascontiguousarray(rows_f, dtype=np.uint32) if filt is not None else None
        sums = np.zeros(b.size, dtype=np.int64)
        counts = np.zeros(b.size, dtype=np.uint64)
        L.check(self.lib.fbk_bsi_range_between_sum(self.h, batch.h, b.ctypes.data, b.size, bit_depth, C.c_int64(lo), C.c_int64(hi),
                                                   filt.h if filt is not None else None, rf.ctypes.data if rf is not None else None,
                                                   sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def bsi_range_between(self, batch: Batch, base_rows, bit_depth: int, lo: int, hi: int, flags: int = 0) -> Tuple[Batch, np.ndarray]:
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        counts = np.zeros(base.size, dtype=np.uint64)
        h = C.c_void_p()
        L.check(self.lib.fbk_bsi_range_between(self.h, batch.h, base.ctypes.data, base.size, bit_depth, lo, hi, flags, C.byref(h), counts.ctypes.data))
        return Batch(self, h.value), counts

    # -- a whole bitmap call tree in one launch (fbk_expr_*) ------------------------------------
    def _expr_args(self, leaves: Sequence[ExprLeaf], prog, n_shards: Optional[int]):
        n = len(leaves)
        arr = (L.ExprLeaf * max(n, 1))()
        for i, lf in enumerate(leaves):
            arr[i].batch = lf.batch.h.value if lf.batch is not None else None
            arr[i].rows = lf.rows.ctypes.data
            arr[i].kind, arr[i].op, arr[i].bit_depth, arr[i].lo, arr[i].hi = lf.kind, lf.op, lf.bit_depth, lf.lo, lf.hi
        pr = np.ascontiguousarray(prog, dtype=np.uint32).reshape(-1)
        if n_shards is None:
            n_shards = int(leaves[0].rows.size) if n else 0
        return arr, n, pr, n_shards

    def expr_count(self, leaves: Sequence[ExprLeaf], prog, n_shards: Optional[int] = None) -> np.ndarray:
        """Per-shard cardinality of the call tree (leaves, postfix program: compile_expr), nothing materialised."""
        arr, n, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        out = np.zeros(n_shards, dtype=np.uint64)
        L.check(self.lib.fbk_expr_count(self.h, arr, n, pr.ctypes.data, pr.size, n_shards, out.ctypes.data))
        return out

    def expr_eval(self, leaves: Sequence[ExprLeaf], prog, flags: int = 0, n_shards: Optional[int] = None) -> Tuple[Batch, np.ndarray]:
        """The call tree's result as one row per shard of a new batch, and its cardinalities."""
        arr, n, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        out = np.zeros(n_shards, dtype=np.uint64)
        h = C.c_void_p()
        L.check(self.lib.fbk_expr_eval(self.h, arr, n, pr.ctypes.data, pr.size, n_shards, flags, C.byref(h), out.ctypes.data))
        return Batch(self, h.value), out

    def query_expr(self, leaves: Sequence[ExprLeaf], prog, flags: int = 0, count_only: bool = False, n_shards: Optional[int] = None) -> Query:
        """The call tree as a launch-only query: read() = cardinalities, output() = the result rows (not with count_only)."""
        arr, n, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        h = C.c_void_p()
        L.check(self.lib.fbk_query_expr(self.h, arr, n, pr.ctypes.data, pr.size, n_shards, flags | (L.EXPR_COUNT_ONLY if count_only else 0), C.byref(h)))
        return Query(self, h.value, "rows", (n_shards,))

    def expr_bsi_agg(self, agg: int, leaves: Sequence[ExprLeaf], prog, batch: Batch, base_rows, bit_depth: int, n_shards: Optional[int] = None):
        """Sum / Min / Max (agg = L.AGG_*) of the int field (batch, base_rows, bit_depth) over the call tree's result, in the tree's
        own launch: per shard (values int64, counts uint64), equal to bsi_sum / bsi_min / bsi_max with expr_eval's row as filter."""
        arr, n, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        vals, counts = np.zeros(n_shards, dtype=np.int64), np.zeros(n_shards, dtype=np.uint64)
        L.check(self.lib.fbk_expr_bsi_agg(self.h, arr, n, pr.ctypes.data, pr.size, n_shards, agg, batch.h if batch is not None else None, base.ctypes.data,
                                          bit_depth, vals.ctypes.data, counts.ctypes.data))
        return vals, counts

    def expr_bsi_sum(self, leaves: Sequence[ExprLeaf], prog, batch: Batch, base_rows, bit_depth: int, n_shards: Optional[int] = None):
        return self.expr_bsi_agg(L.AGG_SUM, leaves, prog, batch, base_rows, bit_depth, n_shards)

    def expr_bsi_min(self, leaves: Sequence[ExprLeaf], prog, batch: Batch, base_rows, bit_depth: int, n_shards: Optional[int] = None):
        return self.expr_bsi_agg(L.AGG_MIN, leaves, prog, batch, base_rows, bit_depth, n_shards)

    def expr_bsi_max(self, leaves: Sequence[ExprLeaf], prog, batch: Batch, base_rows, bit_depth: int, n_shards: Optional[int] = None):
        return self.expr_bsi_agg(L.AGG_MAX, leaves, prog, batch, base_rows, bit_depth, n_shards)

    def expr_row_counts(self, leaves: Sequence[ExprLeaf], prog, a: Batch, rows_a, per_shard: bool = False, filter_counts: bool = False):
        """rows_a: [n_shards, n_a]; totals [n_a] of |row ∩ tree| summed over the shards, in the tree's own launch — equal to
        count_matrix(a, rows_a, F, rows_f) with expr_eval's row F as the single B row.  per_shard / filter_counts add the
        [n_shards, n_a] counts and the tree's per-shard cardinalities (expr_count) to the returned tuple."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        arr, n, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        tot = np.zeros(n_a, dtype=np.uint64)
        ps = np.zeros((n_shards, n_a), dtype=np.uint64) if per_shard else None
        fc = np.zeros(n_shards, dtype=np.uint64) if filter_counts else None
        L.check(self.lib.fbk_expr_row_counts(self.h, arr, n, pr.ctypes.data, pr.size, a.h if a is not None else None, ra.ctypes.data, n_a, n_shards,
                                             tot.ctypes.data, ps.ctypes.data if per_shard else None, fc.ctypes.data if filter_counts else None))
        if not per_shard and not filter_counts:
            return tot
        return (tot,) + ((ps,) if per_shard else ()) + ((fc,) if filter_counts else ())

    def expr_topk(self, leaves: Sequence[ExprLeaf], prog, a: Batch, rows_a, k: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """topk with the call tree as the filter, in the tree's own launch (equal to topk over expr_eval's row)."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        arr, n, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        cap = n_a if k == 0 else min(k, n_a)
        idx = np.zeros(max(cap, 1), dtype=np.uint32)
        cnt = np.zeros(max(cap, 1), dtype=np.uint64)
        got = C.c_uint32()
        L.check(self.lib.fbk_expr_topk(self.h, arr, n, pr.ctypes.data, pr.size, a.h if a is not None else None, ra.ctypes.data, n_a, n_shards, k,
                                       idx.ctypes.data, cnt.ctypes.data, cap, C.byref(got)))
        return idx[: got.value].copy(), cnt[: got.value].copy()

    def expr_topn(self, leaves: Sequence[ExprLeaf], prog, a: Batch, rows_a, n: int = 0, min_threshold: int = 0,
                  tanimoto_threshold: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """topn with the call tree as the source row, in the tree's own launch (equal to topn over expr_eval's row)."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        n_shards, n_a = ra.shape
        arr, nl, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        cap = n_a if n == 0 else min(n, n_a)
        idx = np.zeros(max(cap, 1), dtype=np.uint32)
        cnt = np.zeros(max(cap, 1), dtype=np.uint64)
        got = C.c_uint32()
        L.check(self.lib.fbk_expr_topn(self.h, arr, nl, pr.ctypes.data, pr.size, a.h if a is not None else None, ra.ctypes.data, n_a, n_shards, n,
                                       min_threshold, tanimoto_threshold, idx.ctypes.data, cnt.ctypes.data, cap, C.byref(got)))
        return idx[: got.value].copy(), cnt[: got.value].copy()

    def query_expr_bsi(self, agg: int, leaves: Sequence[ExprLeaf], prog, batch: Batch, base_rows, bit_depth: int, n_shards: Optional[int] = None) -> Query:
        """expr_bsi_agg as a launch-only query: read() = (values, counts).  AGG_SUM runs may go to / accumulate into a caller's
        device buffer of 24 bytes per shard ({psum, nsum, count})."""
        arr, n, pr, n_shards = self._expr_args(leaves, prog, n_shards)
        base = np.ascontiguousarray(base_rows, dtype=np.uint32)
        h = C.c_void_p()
        L.check(self.lib.fbk_query_expr_bsi(self.h, arr, n, pr.ctypes.data, pr.size, n_shards, agg, batch.h if batch is not None else None, base.ctypes.data,
                                            bit_depth, C.byref(h)))
        return Query(self, h.value, "bsi", (n_shards,))

    def plan(self, a: Batch, rows_a, b: Batch, rows_b, device_counts_ptr: int = 0) -> Plan:
        ra = np.ascontiguousarray(rows_a, dtype=np.uint32)
        rb = np.ascontiguousarray(rows_b, dtype=np.uint32)
        assert ra.size == rb.size
        h = C.c_void_p()
        L.check(
            self.lib.fbk_plan_create(
                self.h, a.h, ra.ctypes.data, b.h, rb.ctypes.data, ra.size, C.c_void_p(device_counts_ptr or None), C.byref(h)
            )
        )
        return Plan(self, h.value, int(ra.size))


class Group:
    """Several GPUs behind one process (fbk_group_*): member m owns the shards s with s % G == m;
    partial counts are reduced inside the library (mapReduce + reduceFn, executor.go:6449-6533)."""

    def __init__(self, devices: Sequence[int]):
        self.lib = L.load()
        dv = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        L.check(self.lib.fbk_group_open(dv, len(devices), 0, C.byref(h)))
        self.h = h
        self.members: List[Context] = []
        for i in range(len(devices)):
            m = C.c_void_p()
            L.check(self.lib.fbk_group_member(self.h, i, C.byref(m)))
            self.members.append(Context(_handle=m.value, _borrowed=True))

    def __len__(self) -> int:
        return len(self.members)

    def set_reduce(self, mode: int) -> None:
        L.check(self.lib.fbk_group_set_reduce(self.h, mode))

    def plan_intersection_count_total(self, plans: Sequence[Optional[Plan]]) -> int:
        arr = (C.c_void_p * len(self.members))(*[(p.h if p is not None else None) for p in plans])
        tot = C.c_uint64()
        L.check(self.lib.fbk_group_plan_intersection_count_total(self.h, arr, C.byref(tot)))
        return int(tot.value)

    def count_matrix(self, per_member: Sequence[Optional[dict]], n_a: int, n_b: int) -> np.ndarray:
        """per_member[m]: None or dict(a=Batch, rows_a=[n_shards, n_a], b=Batch, rows_b=[n_shards, n_b],
        filt=Batch|None, rows_f=[n_shards])."""
        args = (L.MatrixArgs * len(self.members))()
        keep = []
        for m, pm in enumerate(per_member):
            if pm is None:
                continue
            ra = np.ascontiguousarray(pm["rows_a"], dtype=np.uint32)
            rb = np.ascontiguousarray(pm["rows_b"], dtype=np.uint32)
            assert ra.shape[1] == n_a and rb.shape[1] == n_b and ra.shape[0] == rb.shape[0]
            rf = np.ascontiguousarray(pm["rows_f"], dtype=np.uint32) if pm.get("filt") is not None else None
            keep += [ra, rb, rf]
            args[m].a, args[m].rows_a = pm["a"].h, ra.ctypes.data
            args[m].b, args[m].rows_b = pm["b"].h, rb.ctypes.data
            args[m].filter = pm["filt"].h if pm.get("filt") is not None else None
            args[m].rows_f = rf.ctypes.data if rf is not None else None
            args[m].n_shards = ra.shape[0]
        tot = np.zeros((n_a, n_b), dtype=np.uint64)
        L.check(self.lib.fbk_group_count_matrix(self.h, args, n_a, n_b, tot.ctypes.data))
        return tot

    def bsi_sum(self, per_member: Sequence[Optional[dict]], bit_depth: int) -> Tuple[int, int]:
        """per_member[m]: None or dict(batch=Batch, base_rows=[n_shards], filt=Batch|None, rows_f=[n_shards]).
        Returns (sum, count) over every shard of every member (fbk_group_bsi_sum)."""
        args = (L.BsiArgs * len(self.members))()
        keep = []
        for m, pm in enumerate(per_member):
            if pm is None:
                continue
            base = np.ascontiguousarray(pm["base_rows"], dtype=np.uint32)
            rf = np.ascontiguousarray(pm["rows_f"], dtype=np.uint32) if pm.get("filt") is not None else None
            keep += [base, rf]
            args[m].batch, args[m].base_rows = pm["batch"].h, base.ctypes.data
            args[m].filter = pm["filt"].h if pm.get("filt") is not None else None
            args[m].rows_f = rf.ctypes.data if rf is not None else None
            args[m].n_shards = base.size
        s, c = C.c_int64(), C.c_uint64()
        L.check(self.lib.fbk_group_bsi_sum(self.h, args, bit_depth, C.byref(s), C.byref(c)))
        return int(s.value), int(c.value)

    def topn(self, per_member: Sequence[Optional[dict]], n_a: int, n: int = 0, min_threshold: int = 0, tanimoto_threshold: int = 0):
        """per_member[m]: None or dict(a=Batch, rows_a=[n_shards, n_a], filt=Batch|None, rows_f=[n_shards]).
        Returns (row indexes, counts) of the TopN over the shards of all members (fbk_group_topn: fbk_topn's answer,
        however the shards are dealt)."""
        args = (L.TopnArgs * len(self.members))()
        keep = []
        for m, pm in enumerate(per_member):
            if pm is None:
                continue
            ra = np.ascontiguousarray(pm["rows_a"], dtype=np.uint32)
            assert ra.ndim == 2 and ra.shape[1] == n_a
            rf = np.ascontiguousarray(pm["rows_f"], dtype=np.uint32) if pm.get("filt") is not None else None
            keep += [ra, rf]
            args[m].a, args[m].rows_a = pm["a"].h, ra.ctypes.data
            args[m].filter = pm["filt"].h if pm.get("filt") is not None else None
            args[m].rows_f = rf.ctypes.data if rf is not None else None
            args[m].n_shards = ra.shape[0]
        cap = n_a
        idx, cnt, got = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64), C.c_uint32()
        L.check(self.lib.fbk_group_topn(self.h, args, n_a, n, min_threshold, tanimoto_threshold, idx.ctypes.data, cnt.ctypes.data, cap, C.byref(got)))
        return idx[: got.value].copy(), cnt[: got.value].copy()

    def reduce_u64(self, device_ptrs: Sequence[int], words: int) -> np.ndarray:
        arr = (C.c_void_p * len(self.members))(*[(p or None) for p in device_ptrs])
        out = np.zeros(words, dtype=np.uint64)
        L.check(self.lib.fbk_group_reduce_u64(self.h, arr, words, out.ctypes.data))
        return out

    def close(self) -> None:
        if self.h:
            L.check(self.lib.fbk_group_close(self.h))
            self.h = C.c_void_p(None)
            for m in self.members:
                m.h = C.c_void_p(None)
