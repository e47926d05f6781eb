"""CPU checks of GroupBy's having / sort / offset / limit (no GPU): the Python model of the reference's pipeline
(groupby_select_ref.py) against inputs and expected outputs recorded from the reference's own tests
(tests/golden/groupby_select_vectors.json), the sort-string and condition parsers of the Python helper (roaring.GroupSelect) against
getSorter's cases, the ctypes mirror of fbk_groupby_select against the C compiler's layout, the presence of the four entry points,
and NULL and invalid arguments, which come back as FBK_E_INVALID without a crash on a machine without a GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import datagen
import groupby_select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "groupby_select_vectors.json")))
ENTRY_POINTS = ["fbk_count_matrix_select", "fbk_count_cube_select", "fbk_count_matrix_sum_select", "fbk_select_groups"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


@pytest.mark.parametrize("q", VECTORS["queries"], ids=lambda q: q["query"])
def test_the_model_gives_the_reference_s_results(q):
    t = VECTORS["tables"][q["table"]]
    sort = R.parse_sort(q["sort"]) if q["sort"] else []
    having = tuple(q["having"]) if q["having"] else None
    assert R.reference_groupby(t["counts"], t["aggs"], sort, having, q["offset"], q["limit"]) == q["expected_cells"]
    # none of the recorded queries meets a quirk: the C ABI's contract gives the same list
    cells, _ = R.select(t["counts"], t["aggs"], sort, having, q["offset"] or 0, q["limit"])
    assert cells == q["expected_cells"]
    got, _ = R.select_np(t["counts"], t["aggs"], sort, having, q["offset"] or 0, q["limit"])
    assert list(got) == q["expected_cells"]


def test_the_two_quirks_of_the_reference():
    counts, aggs = [3, 0, 1, 4, 1, 5, 9, 2, 6], [0] * 9
    groups = [0, 2, 3, 4, 5, 6, 7, 8]
    # neither sort nor having: the limit while merging, then offset and limit again (executor.go:3302, :3331): groups O .. L-1
    assert R.reference_groupby(counts, aggs, offset=2, limit=5) == groups[2:5]
    assert R.select(counts, aggs, offset=2, limit=5)[0] == groups[2:7]
    assert R.reference_groupby(counts, aggs, offset=5, limit=5) == groups[:5]  # the offset is not below the 5 merged groups: ignored
    # an offset >= the number of results is ignored (:3446); the C ABI returns nothing there
    assert R.reference_groupby(counts, aggs, sort=[("count", True)], offset=8, limit=2) == [6, 8]
    assert R.select(counts, aggs, sort=[("count", True)], offset=8, limit=2) == ([], 8)
    assert R.reference_groupby(counts, aggs, having=("count", "gt", 3, 0), offset=4) == [3, 5, 6, 8]
    # with a sort the limit is lifted while merging (:3203): offset and limit once
    assert R.reference_groupby(counts, aggs, sort=[("count", False)], offset=2, limit=5) == [7, 0, 3, 5, 8]
    # a negative literal in a count condition matches nothing (:3792-3795)
    assert R.reference_groupby(counts, aggs, having=("count", "gt", -1, 0)) == []
    assert R.reference_groupby(counts, [-1] * 9, having=("sum", "gt", -2, 0)) == groups


def test_stable_sort_keeps_the_odometer_order_among_ties():
    counts, aggs = [2, 1, 2, 1, 2, 0, 1], [5, 5, -1, 7, 5, 9, 7]
    assert R.select(counts, aggs, [("count", True)])[0] == [0, 2, 4, 1, 3, 6]
    assert R.select(counts, aggs, [("count", False), ("sum", True)])[0] == [3, 6, 1, 0, 4, 2]
    assert R.select(counts, aggs, [("sum", True), ("count", False)])[0] == [3, 6, 1, 0, 4, 2]
    assert R.select(counts, aggs, [("sum", False)], offset=1, limit=3)[0] == [0, 1, 4]


def test_the_numpy_model_is_the_model():
    rng = datagen.rng_for(9330)
    subjects = ("count", "sum")
    for _ in range(400):
        n = int(rng.integers(1, 90))
        counts = rng.choice(np.array([0, 1, 2, 3, 1 << 63, (1 << 64) - 1], dtype=np.uint64), n)
        aggs = rng.choice(np.array([-(1 << 63), -1, 0, 1, (1 << 63) - 1], dtype=np.int64), n)
        order = list(rng.permutation(2)[: int(rng.integers(0, 3))])
        sort = [(subjects[i], bool(rng.integers(2))) for i in order]
        having = None
        if rng.integers(3):
            s = subjects[int(rng.integers(2))]
            src = counts if s == "count" else aggs
            lo, hi = sorted(int(v) for v in rng.choice(src, 2))
            having = (s, R.OPS[int(rng.integers(10))], lo, hi)
        offset, limit = int(rng.integers(0, n + 2)), None if rng.integers(2) else int(rng.integers(0, n + 2))
        exp, m = R.select(counts, aggs, sort, having, offset, limit)
        got, m2 = R.select_np(counts, aggs, sort, having, offset, limit)
        assert list(got) == exp and m == m2


@pytest.mark.parametrize("case", VECTORS["get_sorter"], ids=lambda c: repr(c["spec"]))
def test_sort_string_parsers(lib, case):
    from featurebase_amd.roaring import GroupSelect

    code = {"count": lib.GROUPSEL_COUNT, "sum": lib.GROUPSEL_AGG}
    for parse, subject in ((R.parse_sort, lambda s: s), (GroupSelect.parse_sort, lambda s: code[s])):
        if "error" in case:
            with pytest.raises(ValueError) as ei:
                parse(case["spec"])
            assert str(ei.value) == case["error"]
        else:
            assert parse(case["spec"]) == [(subject(s), d == "desc") for s, d in case["terms"]]


def test_the_helper_builds_the_struct(lib):
    from featurebase_amd.roaring import GroupSelect

    s = GroupSelect(sort="aggregate desc, count asc", having="-5 < sum <= 27", offset=2, limit=3, path="device").struct()
    assert (s.flags, s.n_sort) == (lib.GROUPSEL_DEVICE, 2)
    assert [(t.subject, t.desc) for t in s.sort] == [(lib.GROUPSEL_AGG, 1), (lib.GROUPSEL_COUNT, 0)]
    assert (s.having_subject, s.having_op, s.having_lo, s.having_hi, s.offset, s.limit) == (lib.GROUPSEL_AGG, lib.HAVING_BTWN_LT_LTE, -5, 27, 2, 3)
    s = GroupSelect(sort="count  asc,count asc ", having="count > 5").struct()  # a repeated subject is dropped: it never decides
    assert s.n_sort == 1 and (s.sort[0].subject, s.sort[0].desc) == (lib.GROUPSEL_COUNT, 0)
    assert (s.having_subject, s.having_op, s.having_lo, s.limit) == (lib.GROUPSEL_COUNT, lib.HAVING_GT, 5, (1 << 64) - 1)
    s = GroupSelect(having="count > -1").struct()  # nothing matches: lo > hi
    assert (s.having_op, s.having_lo, s.having_hi) == (lib.HAVING_BETWEEN, 1, 0)
    s = GroupSelect(having=("count", ">=", 1 << 63)).struct()  # a count bound is read as uint64
    assert s.having_lo == -(1 << 63)
    assert GroupSelect.parse_condition("sum >< [1, 9]") == (lib.GROUPSEL_AGG, lib.HAVING_BETWEEN, 1, 9)
    assert GroupSelect.parse_condition("3 <= count < 9") == (lib.GROUPSEL_COUNT, lib.HAVING_BTWN_LTE_LT, 3, 9)
    with pytest.raises(ValueError):
        GroupSelect.parse_condition("zip > 3")


def test_struct_layout_matches_the_compiler_s(lib, tmp_path):
    src = tmp_path / "layout.c"
    fields = ["flags", "n_sort", "sort", "having_subject", "having_op", "having_lo", "having_hi", "offset", "limit"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fbk.h"\nint main(void) {\n  printf("%zu %zu %zu\\n", sizeof(fbk_groupby_select), '
                   'sizeof(fbk_groupby_term), offsetof(fbk_groupby_term, desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(fbk_groupby_select, {f}));\n' for f in fields)
                   + '  printf("%u %u %u %u %u\\n", FBK_GROUPSEL_DEVICE, FBK_GROUPSEL_HOST, FBK_GROUPSEL_COUNT, FBK_GROUPSEL_AGG, FBK_HAVING_BTWN_LT_LT);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(lib.GroupbySelect), C.sizeof(lib.GroupbyTerm), lib.GroupbyTerm.desc.offset] == [64, 8, 4]
    assert [int(x) for x in out[1:1 + len(fields)]] == [getattr(lib.GroupbySelect, f).offset for f in fields]
    assert [int(x) for x in out[1 + len(fields)].split()] == [lib.GROUPSEL_DEVICE, lib.GROUPSEL_HOST, lib.GROUPSEL_COUNT, lib.GROUPSEL_AGG, lib.HAVING_BTWN_LT_LT]
    assert {name: k + 1 for k, name in enumerate(R.OPS)} == {
        "eq": lib.HAVING_EQ, "neq": lib.HAVING_NEQ, "lt": lib.HAVING_LT, "lte": lib.HAVING_LTE, "gt": lib.HAVING_GT, "gte": lib.HAVING_GTE,
        "between": lib.HAVING_BETWEEN, "btwn_lt_lte": lib.HAVING_BTWN_LT_LTE, "btwn_lte_lt": lib.HAVING_BTWN_LTE_LT, "btwn_lt_lt": lib.HAVING_BTWN_LT_LT}


def test_entry_points_are_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "fbk.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for name in ENTRY_POINTS:
        assert f"int32_t {name}(" in hdr and name in lib.SIGNATURES and f" T {name}\n" in out, name


def test_null_and_invalid_arguments_need_no_gpu(lib):
    """without a context nothing can run: FBK_E_INVALID, no crash, with or without a device in the machine"""
    from featurebase_amd.roaring import GroupSelect

    l = lib.load()
    st = GroupSelect(sort="count desc", limit=3).struct()
    counts, cells, oc = (C.c_uint64 * 4)(1, 2, 3, 4), (C.c_uint32 * 4)(), (C.c_uint64 * 4)()
    n, m = C.c_uint64(), C.c_uint64()
    assert l.fbk_select_groups(None, counts, None, 4, C.byref(st), cells, oc, None, 4, C.byref(n), C.byref(m)) == lib.FBK_E_INVALID
    assert l.fbk_select_groups(None, None, None, 0, None, None, None, None, 0, None, None) == lib.FBK_E_INVALID
    assert l.fbk_count_matrix_select(None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0, None, None) == lib.FBK_E_INVALID
    assert l.fbk_count_cube_select(None, None, None, 0, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0, None, None) == lib.FBK_E_INVALID
    assert l.fbk_count_matrix_sum_select(None, None, None, 0, None, None, 0, None, None, None, None, 0, 0, None, None, None, None, 0, None, None) == lib.FBK_E_INVALID
    assert b"NULL" in l.fbk_last_error(None)
