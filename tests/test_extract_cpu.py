"""fbk_extract_* without a device: the ABI is declared and bound, bad arguments are errors (not crashes), the numpy brute force
of tests/extract_ref.py — the yardstick of the GPU tests — reproduces the reference's TestExecutor_Execute_Extract table
(tests/golden/extract_vectors.json) and agrees with the reference's own procedure on the oracle's rows (filter.Columns() and a
column -> slot map, then one Intersect per bit plane / per field row), and the C++ program of the host mirror compiles.

The reference's fields in that test track existence, this project's host mirror does not: for a SET field the reference's nil
(the column exists in the index but not in the field) and [] are compared as equal; for the int field null must be null."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen as D
import extract_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "extract_vectors.json")))
FUNCS = ["fbk_extract_open", "fbk_extract_span", "fbk_extract_columns", "fbk_extract_bsi", "fbk_extract_rows", "fbk_extract_free"]


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
    assert [len(lib.SIGNATURES[f][1]) for f in FUNCS] == [9, 4, 3, 7, 9, 2]
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for f in FUNCS:
        assert f" T {f}\n" in out, f


def test_bad_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    h, n = C.c_void_p(), C.c_uint64()
    rows, ids = np.zeros(4, dtype=np.uint32), np.array([3, 2, 5, 6], dtype=np.uint64)
    buf = np.zeros(8, dtype=np.uint64)

    def err():
        return l.fbk_last_error(None).decode()

    assert l.fbk_extract_open(None, None, None, None, 0, 0, 0, None, None) == lib.FBK_E_INVALID
    assert l.fbk_extract_open(None, None, rows.ctypes.data, ids[1:].ctypes.data, 3, 0, 5, C.byref(h), C.byref(n)) == lib.FBK_E_INVALID
    assert "NULL" in err()  # ctx == NULL
    assert l.fbk_extract_open(None, None, rows.ctypes.data, ids.ctypes.data, 4, 0, 5, C.byref(h), C.byref(n)) == lib.FBK_E_INVALID
    assert "ascending" in err()  # descending shard_ids
    assert l.fbk_extract_open(None, None, rows.ctypes.data, ids[2:].ctypes.data, 2, 0, 5, None, C.byref(n)) == lib.FBK_E_INVALID
    assert not h.value
    assert l.fbk_extract_columns(None, None, buf.ctypes.data) == lib.FBK_E_INVALID
    assert l.fbk_extract_span(None, None, None, None) == lib.FBK_E_INVALID
    assert l.fbk_extract_bsi(None, None, None, rows.ctypes.data, 65, buf.ctypes.data, buf.ctypes.data) == lib.FBK_E_INVALID
    assert "bit depth" in err()
    assert l.fbk_extract_bsi(None, None, None, rows.ctypes.data, 64, buf.ctypes.data, buf.ctypes.data) == lib.FBK_E_INVALID
    assert l.fbk_extract_rows(None, None, None, rows.ctypes.data, 4097, buf.ctypes.data, buf.ctypes.data, 8, C.byref(n)) == lib.FBK_E_INVALID
    assert "4096" in err()
    assert l.fbk_extract_rows(None, None, None, rows.ctypes.data, 4, buf.ctypes.data, buf.ctypes.data, 8, C.byref(n)) == lib.FBK_E_INVALID
    assert l.fbk_extract_free(None, None) == lib.FBK_OK


# ---- the golden table ---------------------------------------------------------------------------------------------------------
def _words(columns, shard):
    w = np.zeros(16 * 1024, dtype=np.uint64)
    for c in columns:
        if c >> 20 == shard:
            p = c & 0xFFFFF
            w[p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    return w.reshape(16, 1024)


def golden_fragments():
    """the golden data as dense words: shards, filter (the existence row), per set field (row ids, [n_shards, n_rows, 16, 1024]),
    the int field as (base, depth, [n_shards, depth + 2, 16, 1024])"""
    shards = sorted({c >> 20 for c in GOLD["existence"]})
    F = np.stack([_words(GOLD["existence"], s) for s in shards])
    sets = {}
    for name, bits in GOLD["imported"].items():
        cleared = {(c["row"], c["column"]) for c in GOLD["cleared"] if c["field"] == name}
        bits = [(r, c) for r, c in bits if (r, c) not in cleared]
        ids = sorted({r for r, _ in bits})
        sets[name] = (ids, np.stack([np.stack([_words([c for r, c in bits if r == i], s) for i in ids]) for s in shards]))
    lo, hi = GOLD["int_range"]["bsint"]
    base = lo if lo > 0 else (hi if hi < 0 else 0)  # bsiBase
    vals = {c: v - base for c, v in GOLD["values"]["bsint"]}
    depth = max(abs(v) for v in vals.values()).bit_length()
    planes = [list(vals), [c for c, v in vals.items() if v < 0]] + [[c for c, v in vals.items() if (abs(v) >> p) & 1] for p in range(depth)]
    S = np.stack([np.stack([_words(p, s) for p in planes]) for s in shards])
    return shards, F, sets, (base, depth, S)


def table_of(shards, F, sets, bsi, fields, offset=0, limit=None):
    """the brute force as the reference's table: [{"column", "rows": [null or list per field]}]"""
    sh, pos, cols = X.select(F, shards, offset, limit)
    per_field = []
    for f in fields:
        if f in sets:
            ids, A = sets[f]
            per_field.append([[ids[i] for i in lst] for lst in X.csr_lists(*X.rows_expected(A, sh, pos))])
        else:
            base, depth, S = bsi
            vals, pres = X.bsi_expected(S, depth, sh, pos)
            per_field.append([[int(v) + base] if p else None for v, p in zip(vals, pres)])
    return [{"column": int(c), "rows": [pf[k] for pf in per_field]} for k, c in enumerate(cols)]


def same_table(got, exp, fields):
    assert [g["column"] for g in got] == [e["column"] for e in exp]
    for g, e in zip(got, exp):
        for f, a, b in zip(fields, g["rows"], e["rows"]):
            if f == "bsint":
                assert a == b, (g["column"], f, a, b)  # null must be null
            else:
                assert (a or []) == (b or []), (g["column"], f, a, b)  # a set field's nil and [] are one


def test_brute_force_reproduces_the_reference_table():
    shards, F, sets, bsi = golden_fragments()
    assert shards == [0, 1, 4] and GOLD["fields"] == ["set", "mutex", "bsint", "bool"]
    same_table(table_of(shards, F, sets, bsi, GOLD["fields"]), GOLD["columns"], GOLD["fields"])
    same_table(table_of(shards, F, sets, bsi, GOLD["fields"], 1, 4), GOLD["columns"][1:5], GOLD["fields"])  # executeLimitCall
    same_table(table_of(shards, F, sets, bsi, GOLD["fields"], 4, None), GOLD["columns"][4:], GOLD["fields"])
    assert table_of(shards, F, sets, bsi, GOLD["fields"], 6, None) == [] and table_of(shards, F, sets, bsi, GOLD["fields"], 0, 0) == []


def test_golden_vectors_are_the_reference_source():
    ref = os.environ.get("FBK_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference"))
    if not os.path.exists(os.path.join(ref, "executor_test.go")):
        pytest.skip("the reference tree is not here")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import extract_extract_vectors as E

    assert E.extract(ref) == GOLD


# ---- brute force == the reference's procedure on the oracle's rows ----------------------------------------------------------------
def _rnd(rng, shape, ands):
    w = np.zeros(shape + (16, 1024), dtype=np.uint64)
    for sl, lo, hi in ((0, 0, 6), (9, 1000, 1024)):  # a few words of two slots: the oracle walks every column in Python
        x = rng.integers(0, 1 << 63, shape + (hi - lo,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (hi - lo,), dtype=np.uint64)
        for _ in range(ands):
            x &= rng.integers(0, 1 << 63, shape + (hi - lo,), dtype=np.uint64) * 2 + rng.integers(0, 2, shape + (hi - lo,), dtype=np.uint64)
        w[..., sl, lo:hi] = x
    return w


@pytest.mark.parametrize("depth", [0, 1, 20, 64])
def test_brute_force_equals_the_reference_procedure(oracle, depth):
    rng = D.rng_for(8000, depth)
    n_sh, n_a = 3, 5
    F, S, A = _rnd(rng, (n_sh,), 1), _rnd(rng, (n_sh, depth + 2), 0), _rnd(rng, (n_sh, n_a), 1)
    S[:, 0] &= _rnd(rng, (n_sh,), 0)  # exists about half; sign and planes also outside it
    S[:, 2:, 0, 0] = 0  # magnitude 0 under set sign bits
    S[1, 0] = 0  # a shard without values
    A[:, 2] = 0  # an empty field row
    ids = [0, 1, 4]
    sh, pos, cols = X.select(F, ids)
    vals, pres = X.bsi_expected(S, depth, sh, pos)
    lists = X.csr_lists(*X.rows_expected(A, sh, pos))
    assert 200 < cols.size and pres.any() and not pres.all()
    k = 0
    for s in range(n_sh):
        p1, ov = X.oracle_bsi(oracle, F[s], S[s], depth)
        p2, ol = X.oracle_rows(oracle, F[s], A[s])
        assert p1 == p2 == pos[sh == s].tolist()
        assert [int(c) for c in cols[k:k + len(p1)]] == [(ids[s] << 20) + p for p in p1]
        assert ov == [int(v) if p else None for v, p in zip(vals[k:k + len(p1)], pres[k:k + len(p1)])]
        assert ol == lists[k:k + len(p1)]
        k += len(p1)
    assert k == cols.size
    # offset / limit cut the same list
    sh2, pos2, cols2 = X.select(F, ids, 7, 100)
    assert np.array_equal(cols2, cols[7:107]) and np.array_equal(X.select(F, ids, cols.size + 3, 5)[2], cols[:0])
    assert np.array_equal(X.select(F, ids, 5, (1 << 64) - 1)[2], cols[5:])


def test_cpp_program_compiles():
    import test_cpp_extract as T

    T.compile_it()
    assert os.path.exists(T.BIN)
