"""Python model of the tail of the reference's GroupBy (executor.go:3176-3459), the yardstick of the selection tests.

  groups      the cells with count > 0, in ascending cell order: the odometer order, last field fastest (:8913)
  having      ApplyConditionToGroupCounts / satisfiesCondition (:3787-3916): one condition on count (uint64) or sum (int64)
  sort        getSorter (:3130-3162) + sort.Stable(groupCountSorter) (:3096-3126, :3409)
  offset / limit  applyLimitAndOffsetToGroupByResult (:3441-3459)

`select` is the C ABI's contract (include/fbk.h): offset >= matched gives nothing.  `reference_groupby` adds the reference's two quirks,
which fbk::Executor::GroupBy reproduces: with neither sort nor having the limit is applied while merging (:3302) and then offset and
limit again (:3331), and an offset >= the number of results is ignored (:3446).

A selection is a dict: sort = [(subject, desc), ...] with subject "count" | "sum", having = None | (subject, op, lo, hi) with op one
of OPS, offset, limit (None: no limit)."""
from __future__ import annotations

OPS = ("eq", "neq", "lt", "lte", "gt", "gte", "between", "btwn_lt_lte", "btwn_lte_lt", "btwn_lt_lt")
OP_CODE = {name: k + 1 for k, name in enumerate(OPS)}  # FBK_HAVING_*


def parse_sort(spec: str):
    """getSorter: [(subject, desc)] with subject "count" | "sum"; raises ValueError with the reference's message"""
    out = []
    for term in spec.split(","):
        term = term.strip()
        parts = term.split()
        if len(parts) == 0:
            raise ValueError(f"invalid sorting directive: '{term}'")
        if parts[0] == "count":
            subject = "count"
        elif parts[0] in ("aggregate", "sum"):
            subject = "sum"
        else:
            raise ValueError(f"sorting is only supported on count, aggregate, or sum, not '{parts[0]}'")
        if len(parts) == 1:
            desc = True
        elif len(parts) > 2:
            raise ValueError(f"parsing sort directive: '{term}': too many elements")
        elif parts[1] == "asc":
            desc = False
        elif parts[1] == "desc":
            desc = True
        else:
            raise ValueError(f"unknown sort direction '{parts[1]}'")
        out.append((subject, desc))
    return out


def satisfies(count: int, agg: int, having) -> bool:
    if having is None:
        return True
    subject, op, lo, hi = having
    x = count if subject == "count" else agg
    if subject == "count" and (lo < 0 or (op.startswith("b") and hi < 0)):
        return False  # Uint64Value / Uint64SliceValue fail on a negative literal (:3792-3795, :3822-3825)
    return {
        "eq": x == lo, "neq": x != lo, "lt": x < lo, "lte": x <= lo, "gt": x > lo, "gte": x >= lo,
        "between": lo <= x <= hi, "btwn_lt_lte": lo < x <= hi, "btwn_lte_lt": lo <= x < hi, "btwn_lt_lt": lo < x < hi,
    }[op]


def matched_cells(counts, aggs, having):
    return [c for c in range(len(counts)) if int(counts[c]) > 0 and satisfies(int(counts[c]), int(aggs[c]) if aggs is not None else 0, having)]


def stable_sort(cells, counts, aggs, sort):
    """sort.Stable with groupCountSorter.Less: terms in order, the input order among groups equal in every term"""
    out = list(cells)
    for subject, desc in reversed(list(sort)):  # (stable sorts, the last term first, compose to the lexicographic order)
        val = (lambda c: int(counts[c])) if subject == "count" else (lambda c: int(aggs[c]))
        out.sort(key=val, reverse=desc)  # (list.sort is stable, and with reverse=True equal elements KEEP their order)
    return out


def select(counts, aggs, sort=(), having=None, offset=0, limit=None):
    """The C ABI's stage: (cells of the result in order, matched)"""
    m = stable_sort(matched_cells(counts, aggs, having), counts, aggs, sort)
    lo = min(offset, len(m))
    end = len(m) if limit is None else lo + min(limit, len(m) - lo)
    return m[lo:end], len(m)


def _limit_offset(results, offset, limit):
    """applyLimitAndOffsetToGroupByResult (:3441-3459); offset / limit None: the argument is absent"""
    if offset is not None and offset < len(results):
        results = results[offset:]
    if limit is not None and limit < len(results):
        results = results[:limit]
    return results


def reference_groupby(counts, aggs, sort=(), having=None, offset=None, limit=None):
    """executeGroupBy's tail with its quirks: the cells of the result in order"""
    results = [c for c in range(len(counts)) if int(counts[c]) > 0]
    if not sort and having is None and limit is not None:
        results = results[:limit]  # mergeGroupCounts(..., limit) (:3302); a sorter or a having lifts that limit (:3203, :3210)
    if not sort and having is None:
        results = _limit_offset(results, offset, limit)
    if having is not None:
        results = [c for c in results if satisfies(int(counts[c]), int(aggs[c]) if aggs is not None else 0, having)]
    if sort:
        results = _limit_offset(stable_sort(results, counts, aggs, sort), offset, limit)
    elif having is not None:
        results = _limit_offset(results, offset, limit)
    return results


def select_np(counts, aggs, sort=(), having=None, offset=0, limit=None):
    """`select` in numpy for the large sizes of the GPU tests: (cells uint32, matched).  The CPU tests hold it against `select`."""
    import numpy as np

    counts = np.asarray(counts, dtype=np.uint64)
    aggs = np.asarray(aggs, dtype=np.int64) if aggs is not None else None
    mask = counts > 0
    if having is not None:
        subject, op, lo, hi = having
        if subject == "count":
            if lo < 0 or (op.startswith("b") and hi < 0):
                mask &= False
                lo = hi = 0
            x, lo, hi = counts, np.uint64(lo), np.uint64(hi)
        else:
            x, lo, hi = aggs, np.int64(lo), np.int64(hi)
        mask &= {
            "eq": lambda: x == lo, "neq": lambda: x != lo, "lt": lambda: x < lo, "lte": lambda: x <= lo, "gt": lambda: x > lo, "gte": lambda: x >= lo,
            "between": lambda: (lo <= x) & (x <= hi), "btwn_lt_lte": lambda: (lo < x) & (x <= hi), "btwn_lte_lt": lambda: (lo <= x) & (x < hi),
            "btwn_lt_lt": lambda: (lo < x) & (x < hi),
        }[op]()
    cells = np.flatnonzero(mask)
    if sort and cells.size:
        keys = []
        for subject, desc in sort:
            k = counts[cells] if subject == "count" else aggs[cells].view(np.uint64) ^ np.uint64(1 << 63)
            keys.append(~k if desc else k)
        cells = cells[np.lexsort(tuple(reversed(keys)))]  # (lexsort is stable; its LAST key is the primary one)
    lo_ = min(offset, cells.size)
    end = cells.size if limit is None else lo_ + min(limit, cells.size - lo_)
    return cells[lo_:end].astype(np.uint32), int(mask.sum())
