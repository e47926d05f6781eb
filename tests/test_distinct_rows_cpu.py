"""fbk_bsi_distinct_rows without a device: the ABI is declared and bound, bad arguments are errors (not crashes), the yardstick of the
GPU tests (tests/distinct_rows_ref.py) equals a brute-force Python set on seeded inputs, and the transcription of
TestExecutor_ForeignIndex (tests/golden/foreign_index_vectors.json) is well-formed and consistent with the yardstick."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import datagen as D
import distinct_rows_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FUNC = "fbk_bsi_distinct_rows"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    return L


def test_signature_declared_and_exported(lib):
    l = lib.load()
    assert FUNC in lib.SIGNATURES and getattr(l, FUNC) is not None
    assert len(lib.SIGNATURES[FUNC][1]) == 15
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    assert f" T {FUNC}\n" in out
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "fbk.h")).read()
    assert "int32_t fbk_bsi_distinct_rows(fbk_ctx* ctx, const fbk_batch* bsi, const uint32_t* base_rows, uint32_t bit_depth, int64_t base," in hdr
    assert "#define FBK_ABI_VERSION 6" in hdr
    from featurebase_amd.roaring import Context

    assert callable(Context.bsi_distinct_rows)


def test_bad_arguments_are_errors_not_crashes(lib):
    l = lib.load()
    rows = np.zeros(4, dtype=np.uint32)
    ids = np.zeros(4, dtype=np.uint64)
    h, n_pos, n_neg = C.c_void_p(5), C.c_uint32(7), C.c_uint32(7)

    def err():
        return l.fbk_last_error(None).decode()

    def call(depth=8, base_rows=rows.ctypes.data, n_sh=1, flags=0, ob=C.byref(h), oi=ids.ctypes.data, cap=4, op=C.byref(n_pos), on=C.byref(n_neg)):
        return l.fbk_bsi_distinct_rows(None, None, base_rows, depth, 0, None, None, n_sh, flags, ob, oi, cap, op, on, None)

    assert l.fbk_bsi_distinct_rows(None, None, None, 0, 0, None, None, 0, 0, None, None, 0, None, None, None) == lib.FBK_E_INVALID
    assert call(ob=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(op=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(on=None) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(oi=None) == lib.FBK_E_INVALID and "NULL" in err()
    h.value, n_pos.value, n_neg.value = 5, 7, 7
    assert call() == lib.FBK_E_INVALID and "NULL" in err()  # ctx == NULL; the outputs are reset before anything else
    assert h.value is None and n_pos.value == 0 and n_neg.value == 0
    assert call(depth=64) == lib.FBK_E_INVALID and "fbk_bsi_distinct" in err() and "bit depth" in err()
    assert call(depth=65) == lib.FBK_E_INVALID and "bit depth" in err()
    assert call(depth=63) == lib.FBK_E_INVALID and "NULL" in err()  # (the depth is fine: the context is what is missing)
    for flags in (2, 4, 1 << 31, 3):
        assert call(flags=flags) == lib.FBK_E_INVALID and "flags" in err(), flags
    assert call(flags=lib.SETOP_OPTIMIZE) == lib.FBK_E_INVALID and "NULL" in err()
    assert call(n_sh=(1 << 20) + 1) == lib.FBK_E_INVALID and "2^20" in err()
    assert call(base_rows=None) == lib.FBK_E_INVALID and "NULL" in err()


def _brute(columns, stored, base, keep):
    pos, neg = set(), set()
    for c, s in zip(columns, stored):
        if keep is not None and c not in keep:
            continue
        v = s + base
        (pos if v >= 0 else neg).add(abs(v))
    return pos, neg


def _flat(by_shard):
    out = []
    for sh in sorted(by_shard):
        p = [int(x) for x in by_shard[sh]]
        assert p == sorted(set(p)) and all(x >> 20 == sh for x in p) and p, sh
        out += p
    return out


@pytest.mark.parametrize("kind", ["small", "wide", "edges"])
def test_yardstick_equals_a_brute_force_set(kind):
    rng = D.rng_for(9970, {"small": 0, "wide": 1, "edges": 2}[kind])
    for it in range(60):
        n = int(rng.integers(0, 400))
        columns = [int(c) for c in rng.choice(1 << 22, n, replace=False)]
        if kind == "small":
            stored = [int(x) for x in rng.integers(-40, 41, n)]
            base = int(rng.integers(-30, 31))
        elif kind == "wide":
            stored = [int(x) for x in rng.integers(-(1 << 62), 1 << 62, n)]
            base = int(rng.integers(-(1 << 61), 1 << 61))
        else:
            pool = [0, 63, 64, 65535, 65536, (1 << 20) - 1, 1 << 20, 3 * (1 << 20) + 5, -1, -(1 << 20), -((1 << 20) + 1)]
            stored = [int(rng.choice(pool)) for _ in range(n)]
            base = int(rng.choice([0, 1, -1, 1 << 20, -(1 << 20)]))
        keep = None if it % 3 == 0 else set(c for c in columns if rng.random() < 0.5) | {(1 << 22) + 1}
        got = R.distinct_rows(columns, stored, base, None if keep is None else sorted(keep))
        pos, neg = _brute(columns, stored, base, keep)
        assert _flat(got["pos"]) == sorted(pos) and _flat(got["neg"]) == sorted(neg), (kind, it)
        if keep is None:  # the vectorised form the GPU tests use for large inputs
            fast = R.from_values(np.array(stored, dtype=np.int64), base)
            assert _flat(fast["pos"]) == sorted(pos) and _flat(fast["neg"]) == sorted(neg), (kind, it)


def test_yardstick_signs_zero_and_int64_ends():
    got = R.distinct_rows([1, 2, 3, 4, 5], [0, -5, 5, -7, 7], 5)
    assert _flat(got["pos"]) == [0, 5, 10, 12] and _flat(got["neg"]) == [2]  # v == 0 goes to Pos
    got = R.distinct_rows([1, 2], [-(1 << 63) + 1, (1 << 63) - 1], -1)
    assert _flat(got["neg"]) == [1 << 63] and _flat(got["pos"]) == [(1 << 63) - 2]
    with pytest.raises(OverflowError):
        R.distinct_rows([1], [(1 << 63) - 1], 1)
    with pytest.raises(OverflowError):
        R.from_values(np.array([-(1 << 63) + 1], dtype=np.int64), -2)
    assert R.distinct_rows([], [], 3) == {"pos": {}, "neg": {}}


def test_foreign_index_fixture_is_well_formed_and_consistent():
    fx = json.load(open(os.path.join(HERE, "golden", "foreign_index_vectors.json")))
    assert "one = 1" in fx["note"] and "twenty-one = 21" in fx["note"] and fx["shard_width"] == 1 << 20
    assert fx["parent_keys"] == {"one": 1, "two": 2, "three": 3, "twenty-one": 21, "twenty-two": 22, "twenty-three": 23}
    child, exp = fx["child"], fx["expected"]
    cols = [int(c) for c in child["parent_id"]]
    vals = [child["parent_id"][str(c)] for c in cols]
    assert sorted(cols) == [1, 2, 4, 1 << 20] and all(0 <= v < 1 << child["parent_id_bit_depth"] for v in vals)
    assert set(vals) <= set(fx["parent_keys"].values())
    every = R.distinct_rows(cols, vals, child["parent_id_base"])
    assert _flat(every["pos"]) == exp["distinct_parent_id_pos"] == [1, 2, 21] and _flat(every["neg"]) == exp["distinct_parent_id_neg"] == []
    j = exp["join"]
    blue = R.distinct_rows(cols, vals, child["parent_id_base"], child["color"][str(j["color_row"])])
    general = fx["parent"]["general"][str(j["general_row"])]
    assert sorted(set(_flat(blue["pos"])) & set(general)) == j["result"] == [1]
    assert sorted(c for c, v in zip(cols, vals) if v == 1) == exp["row_parent_id_eq_one"]
    assert sorted(c for c, v in zip(cols, vals) if v != 1) == exp["row_parent_id_neq_one"]
    empty = exp["stepchild_distinct_other_where_parent_id_eq_3"]
    none = R.distinct_rows([], [], 0, [])
    assert empty["pos"] == _flat(none["pos"]) == [] and empty["neg"] == _flat(none["neg"]) == []
