"""fbk_bsi_sort / fbk_extract_open_columns without a device: the ABI is declared and bound, bad arguments are errors (not crashes),
and the numpy brute force of tests/sort_ref.py — the yardstick of the GPU tests — reproduces the int query of the reference's
TestExecutor_Sort (tests/golden/sort_vectors.json) and agrees with the reference's own procedure restated on the oracle's rows
(consider / pos / neg, one Intersect and a dict update per plane, stable sort, pairwise merge, cut) wherever the reference is
deterministic: on inputs without equal values, and on inputs with ties after ordering each run of equal values by column."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen as D
import sort_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "sort_vectors.json")))
FUNCS = ["fbk_bsi_sort", "fbk_extract_open_columns"]
U64MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


def test_signatures_declared_and_exported(lib):
    l = lib.load()
    for f in FUNCS:
        assert f in lib.SIGNATURES and getattr(l, f) is not None, f
    assert [len(lib.SIGNATURES[f][1]) for f in FUNCS] == [16, 7]
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for f in FUNCS:
        assert f" T {f}\n" in out, f
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "fbk.h")).read()
    assert "#define FBK_SORT_DESC 1u" in hdr and "#define FBK_SORT_KEEP_ZERO 2u" in hdr
    assert (lib.SORT_DESC, lib.SORT_KEEP_ZERO) == (1, 2)


def test_sort_bad_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    n, tot = C.c_uint64(7), C.c_uint64(7)
    rows = np.zeros(4, dtype=np.uint32)
    ids = np.array([3, 2, 5, 1 << 44], dtype=np.uint64)
    cols, vals = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.int64)

    def err():
        return l.fbk_last_error(None).decode()

    def call(depth=8, base=rows.ctypes.data, sh=ids[2:].ctypes.data, n_sh=1, flags=0, oc=cols.ctypes.data, ov=vals.ctypes.data, cap=8, on=C.byref(n)):
        return l.fbk_bsi_sort(None, None, base, depth, None, None, sh, n_sh, flags, 0, 5, oc, ov, cap, on, C.byref(tot))

    assert l.fbk_bsi_sort(None, None, None, 0, None, None, None, 0, 0, 0, 0, None, None, 0, None, None) == lib.FBK_E_INVALID
    assert call(depth=65) == lib.FBK_E_INVALID and "bit depth" in err()
    assert call(on=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(base=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(sh=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(oc=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(ov=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(sh=ids.ctypes.data, n_sh=2) == lib.FBK_E_INVALID and "ascending" in err()
    assert call(sh=ids[2:].ctypes.data, n_sh=2) == lib.FBK_E_INVALID and "2^44" in err()
    assert call(flags=4) == lib.FBK_E_INVALID and "flag" in err()
    n.value = 7
    assert call() == lib.FBK_E_INVALID and "NULL" in err()  # ctx == NULL; the counts are reset before anything else
    assert n.value == 0 and tot.value == 0
    assert call(depth=64) == lib.FBK_E_INVALID


def test_open_columns_bad_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    h = C.c_void_p()
    cols = np.array([5, 6, (3 << 20) + 1], dtype=np.uint64)
    ids = np.array([3, 2, 5, 1 << 44], dtype=np.uint64)
    rank = np.zeros(4, dtype=np.uint32)

    def err():
        return l.fbk_last_error(None).decode()

    assert l.fbk_extract_open_columns(None, None, 0, None, 0, None, None) == lib.FBK_E_INVALID
    assert l.fbk_extract_open_columns(None, None, 3, ids[2:].ctypes.data, 1, C.byref(h), rank.ctypes.data) == lib.FBK_E_INVALID and "NULL" in err()
    assert l.fbk_extract_open_columns(None, cols.ctypes.data, 3, ids[2:].ctypes.data, 1, C.byref(h), None) == lib.FBK_E_INVALID and "NULL" in err()
    assert l.fbk_extract_open_columns(None, cols.ctypes.data, 3, None, 1, C.byref(h), rank.ctypes.data) == lib.FBK_E_INVALID and "NULL" in err()
    assert l.fbk_extract_open_columns(None, cols.ctypes.data, 1 << 31, ids[2:].ctypes.data, 1, C.byref(h), rank.ctypes.data) == lib.FBK_E_INVALID
    assert "2^31" in err()  # (checked before the list is read)
    assert l.fbk_extract_open_columns(None, cols.ctypes.data, 3, ids.ctypes.data, 2, C.byref(h), rank.ctypes.data) == lib.FBK_E_INVALID
    assert "ascending" in err()
    assert l.fbk_extract_open_columns(None, cols.ctypes.data, 3, ids[2:].ctypes.data, 2, C.byref(h), rank.ctypes.data) == lib.FBK_E_INVALID
    assert "2^44" in err()
    assert l.fbk_extract_open_columns(None, cols.ctypes.data, 3, ids[2:].ctypes.data, 1, C.byref(h), rank.ctypes.data) == lib.FBK_E_INVALID  # ctx == NULL
    assert not h.value


# ---- the golden query -----------------------------------------------------------------------------------------------------------
def golden_fragment():
    """the six bsint values as one shard: (depth, S [1, depth + 2, 16, 1024])"""
    vals = dict(map(tuple, GOLD["values"]["bsint"]))
    depth = max(abs(v) for v in vals.values()).bit_length()
    planes = [list(vals), [c for c, v in vals.items() if v < 0]] + [[c for c, v in vals.items() if (abs(v) >> p) & 1] for p in range(depth)]
    S = np.zeros((1, depth + 2, 16 * 1024), dtype=np.uint64)
    for r, cs in enumerate(planes):
        for c in cs:
            S[0, r, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return depth, S.reshape(1, depth + 2, 16, 1024), vals


def golden_filter(q, vals):
    import re

    k = int(re.fullmatch(r"Row\(bsint > (-?\d+)\)", q["filter"]).group(1))
    F = np.zeros((1, 16 * 1024), dtype=np.uint64)
    for c, v in vals.items():
        if v > k:
            F[0, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return F.reshape(1, 16, 1024)


def test_both_restatements_reproduce_the_reference_expectation(oracle):
    assert [q["supported"] for q in GOLD["queries"]] == [True, False, False]
    assert [q["field"] for q in GOLD["queries"]] == ["bsint", "bool", "keymutex"]
    q = GOLD["queries"][0]
    depth, S, vals = golden_fragment()
    F = golden_filter(q, vals)
    want_c, want_v = [c["column"] for c in q["columns"]], [c["rows"][0] for c in q["columns"]]
    assert (want_c, want_v) == ([4, 5], [3, 4]) and (q["limit"], q["offset"], q["desc"]) == (2, 1, False)
    cols, v, total = R.brute(S, F, [0], depth, q["desc"], False, q["offset"], q["limit"])
    assert (cols.tolist(), v.tolist(), total) == (want_c, want_v, 3)
    rc, rv = R.cut(*R.reference_sort(oracle, S, F, [0], depth, q["desc"]), q["offset"], q["limit"])
    assert (rc.tolist(), rv.tolist()) == (want_c, want_v)


def test_golden_vectors_are_the_reference_source():
    ref = os.environ.get("FBK_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference"))
    if not os.path.exists(os.path.join(ref, "executor_test.go")):
        pytest.skip("the reference tree is not here")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import extract_sort_vectors as E

    assert E.extract(ref) == GOLD


# ---- brute force == the reference's procedure on the oracle's rows ----------------------------------------------------------------
def _rnd(rng, shape, ands):
    w = np.zeros(shape + (16, 1024), dtype=np.uint64)
    for sl, lo, hi in ((0, 0, 4), (9, 1021, 1024)):  # a few words of two slots: the oracle walks every column in Python
        x = rng.integers(0, 1 << 63, shape + (hi - lo,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (hi - lo,), dtype=np.uint64)
        for _ in range(ands):
            x &= rng.integers(0, 1 << 63, shape + (hi - lo,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (hi - lo,), dtype=np.uint64)
        w[..., sl, lo:hi] = x
    return w


CUTS = [(0, None), (0, 1), (3, 10), (17, 64), (1, None), (0, 0)]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("depth,filtered", [(40, True), (40, False), (64, True)])
def test_brute_force_equals_the_reference_procedure_on_distinct_values(oracle, depth, filtered, desc):
    rng = D.rng_for(9000, depth, int(filtered), int(desc))
    n_sh, ids = 3, [0, 1, 4]
    S = _rnd(rng, (n_sh, depth + 2), 0)
    S[:, 0] &= _rnd(rng, (n_sh,), 0)  # exists about half; sign and planes also outside it
    F = _rnd(rng, (n_sh,), 0) if filtered else None
    cols, vals, total = R.brute(S, F, ids, depth, desc)
    assert total == cols.size > 100 and np.unique(vals).size == vals.size and (vals < 0).any() and (vals > 0).any()
    rc, rv = R.reference_sort(oracle, S, F, ids, depth, desc)
    assert np.array_equal(rc, cols) and np.array_equal(rv, vals)
    for off, lim in CUTS + [(total - 1, 5), (total, 5)]:
        bc, bv, bt = R.brute(S, F, ids, depth, desc, False, off, lim)
        cc, cv = R.cut(rc, rv, off, lim)
        assert bt == total and np.array_equal(bc, cc) and np.array_equal(bv, cv), (off, lim)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("depth", [1, 3])
def test_brute_force_equals_the_reference_procedure_with_ties(oracle, depth, desc):
    rng = D.rng_for(9050, depth, int(desc))
    n_sh, ids = 3, [2, 3, 9]
    S = _rnd(rng, (n_sh, depth + 2), 0)
    S[1, 0] = 0  # a shard without values
    S[0, 2:, 0, 0] = 0  # magnitude 0 under set sign bits: never in the reference's map
    F = _rnd(rng, (n_sh,), 0)
    cols, vals, total = R.brute(S, F, ids, depth, desc)
    assert total > 50 and np.unique(vals).size <= 2 * ((1 << depth) - 1) and not (vals == 0).any()
    rc, rv = R.canon(*R.reference_sort(oracle, S, F, ids, depth, desc), desc)
    assert np.array_equal(rc, cols) and np.array_equal(rv, vals)
    for off, lim in CUTS:
        bc, bv, _ = R.brute(S, F, ids, depth, desc, False, off, lim)
        cc, cv = R.cut(rc, rv, off, lim)
        assert np.array_equal(bc, cc) and np.array_equal(bv, cv), (off, lim)
    # with the zeros kept the brute force is the same list plus the columns of magnitude 0, at value 0
    kc, kv, kt = R.brute(S, F, ids, depth, desc, True)
    assert kt > total and np.array_equal(kc[kv != 0], cols) and np.array_equal(kv[kv != 0], vals)
