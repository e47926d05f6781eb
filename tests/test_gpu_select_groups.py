"""The GroupBy selection stage alone (fbk_select_groups) with values no GroupBy produces: the device path and the host path, pinned by
FBK_GROUPSEL_DEVICE / FBK_GROUPSEL_HOST, give identical output and both equal the model of the reference (groupby_select_ref.py),
bit for bit.  Sizes at the wave (64), unit (512), block (2048) and multi-block boundaries; the full product of specs for n <= 257,
a seeded sample of it above."""
import ctypes as C

import numpy as np
import pytest

import datagen
import groupby_select_ref as R
from featurebase_amd import lib as L
from featurebase_amd.roaring import GroupSelect

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 70, 255, 256, 257, 4097, (1 << 16) + 3, (1 << 20) + 1]
CONTENTS = ["zero", "equal", "half_zero", "agg_extremes", "huge_counts", "monotone"]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SORTS = [()] + [((s, d),) for s in ("count", "sum") for d in (False, True)] + [
    ((s0, d0), (s1, d1)) for s0, s1 in (("count", "sum"), ("sum", "count")) for d0 in (False, True) for d1 in (False, True)
]
NONE = None  # (a limit)
U64_MAX = (1 << 64) - 1


def make(content: str, n: int, rng):
    if content == "zero":
        return np.zeros(n, dtype=np.uint64), rng.integers(-3, 4, n).astype(np.int64)
    if content == "equal":  # the rank-K boundary falls inside ties that span units and blocks
        return np.full(n, 7, dtype=np.uint64), np.full(n, -5, dtype=np.int64)
    if content == "half_zero":
        return rng.choice(np.array([0, 1, 2, 3], dtype=np.uint64), n, p=[0.5, 0.2, 0.15, 0.15]), rng.integers(-2, 3, n).astype(np.int64)
    if content == "agg_extremes":
        return rng.integers(1, 4, n).astype(np.uint64), rng.choice(np.array([I64_MIN, -1, 0, 1, I64_MAX], dtype=np.int64), n)
    if content == "huge_counts":  # a signed compare orders 2^63 below 1
        return rng.choice(np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, U64_MAX], dtype=np.uint64), n), rng.integers(-2, 3, n).astype(np.int64)
    return np.arange(1, n + 1, dtype=np.uint64), (n // 2 - np.arange(n)).astype(np.int64)  # strictly ascending, strictly descending


def havings(counts, aggs, rng):
    """none, then each of the ten ops on each subject with bounds that occur in the array (so that < and <= differ)"""
    out = [None]
    for subject, src in (("count", counts), ("sum", aggs)):
        live = src[counts > 0] if (counts > 0).any() else src
        lo, hi = sorted(int(v) for v in rng.choice(live, 2))
        out += [(subject, op, lo, hi) for op in R.OPS]
    return out


def windows(matched: int):
    return [(0, NONE), (0, 0), (0, 1), (1, 1), (max(matched - 1, 0), 5), (matched, 1), (3, matched), (U64_MAX, U64_MAX)]


def run(ctx, counts, aggs, sort, having, offset, limit, path):
    sel = GroupSelect(sort=[(s, d) for s, d in sort], having=None if having is None else (having[0], R.OP_CODE[having[1]], having[2], having[3]),
                      offset=offset, limit=limit, path=path)
    cells, oc, oa, matched = ctx.select_groups(counts, aggs, sel, cap=max(counts.size, 1))
    return cells, oc, oa, matched


def check(ctx, counts, aggs, sort, having, offset, limit):
    exp, matched = R.select_np(counts, aggs, sort, having, offset, limit)
    for path in ("device", "host"):
        cells, oc, oa, m = run(ctx, counts, aggs, sort, having, offset, limit, path)
        what = (path, counts.size, sort, having, offset, limit)
        assert m == matched, what
        assert np.array_equal(cells, exp), what
        assert np.array_equal(oc, counts[exp]) and np.array_equal(oa, aggs[exp]), what


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("n", SIZES)
def test_select_groups_matches_the_model_on_both_paths(gpu_ctx, n, content):
    rng = datagen.rng_for(9301, n, CONTENTS.index(content))
    counts, aggs = make(content, n, rng)
    specs = []
    for having in havings(counts, aggs, rng):
        matched = R.select_np(counts, aggs, (), having)[1]
        specs += [(sort, having, off, lim) for sort in SORTS for off, lim in windows(matched)]
    if n > 257:
        pick = rng.choice(len(specs), size=12 if n < (1 << 16) else 5, replace=False)
        specs = [specs[i] for i in pick]
        # ... and, always, the selection (K < matched) under two terms and the stable sort of everything
        specs += [((("count", True), ("sum", False)), None, 3, 1000), ((("sum", True), ("count", False)), None, 0, NONE)]
    else:
        assert len(specs) == 13 * 21 * 8
    for sort, having, off, lim in specs:
        check(gpu_ctx, counts, aggs, sort, having, off, lim)


def test_counts_only_and_automatic_path(gpu_ctx):
    """aggs = NULL is the count-only form; with neither flag the library chooses (host at <= 2^16 cells, device above): same answers"""
    rng = datagen.rng_for(9303)
    for n in (20000, 1 << 16, (1 << 16) + 1):
        counts, _ = make("half_zero", n, rng)
        sel = GroupSelect(sort="count desc", having="count > 1", offset=2, limit=50)
        cells, oc, matched = gpu_ctx.select_groups(counts, None, sel)
        exp, m = R.select_np(counts, None, [("count", True)], ("count", "gt", 1, 0), 2, 50)
        assert matched == m and np.array_equal(cells, exp) and np.array_equal(oc, counts[exp])


@pytest.mark.parametrize("path", ["device", "host"])
def test_capacity_and_errors_leave_the_context_usable(gpu_ctx, path):
    lib, n = gpu_ctx.lib, 5000
    counts, aggs = np.arange(1, n + 1, dtype=np.uint64), np.arange(n, dtype=np.int64)
    cells, oc, oa = np.full(n, 77, dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)
    out_n, matched = C.c_uint64(), C.c_uint64()

    def call(st, cap, counts_p=counts.ctypes.data, aggs_p=aggs.ctypes.data, cells_p=cells.ctypes.data):
        return lib.fbk_select_groups(gpu_ctx.h, counts_p, aggs_p, n, C.byref(st), cells_p, oc.ctypes.data, oa.ctypes.data, cap, C.byref(out_n), C.byref(matched))

    st = GroupSelect(sort="sum desc", path=path).struct()
    assert call(st, n - 1) == L.FBK_E_CAPACITY
    assert out_n.value == n and matched.value == n and (cells == 77).all()
    assert call(st, n) == L.FBK_OK and out_n.value == n and np.array_equal(cells, np.arange(n - 1, -1, -1, dtype=np.uint32))
    bad = []
    for change in ("flags", "n_sort", "repeat", "op", "subject", "desc", "both"):
        s = GroupSelect(sort="sum desc, count asc", having="count > 1", path=path).struct()
        if change == "flags":
            s.flags |= 4
        elif change == "n_sort":
            s.n_sort = 3
        elif change == "repeat":
            s.sort[1].subject = L.GROUPSEL_AGG
        elif change == "op":
            s.having_op = 11
        elif change == "subject":
            s.sort[0].subject = 3
        elif change == "desc":
            s.sort[0].desc = 2
        else:
            s.flags = L.GROUPSEL_DEVICE | L.GROUPSEL_HOST
        bad.append(s)
    for s in bad:
        assert call(s, n) == L.FBK_E_INVALID
    assert call(st, n, cells_p=None) == L.FBK_E_INVALID  # NULL outputs with cap > 0
    assert call(st, n, counts_p=None) == L.FBK_E_INVALID
    assert call(st, n, aggs_p=None) == L.FBK_E_INVALID  # a sort on the aggregate of a call without one
    assert call(st, n) == L.FBK_OK and out_n.value == n
