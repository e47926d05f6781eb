"""GPU parity of fbk_bsi_distinct_rows (Distinct() of an int field as SignedRow{Neg, Pos} on the device) against the numpy yardstick
of tests/distinct_rows_ref.py (the CPU test shows it equals a brute-force set), after fbk_batch_download.  Inputs are 1-3 sparse
shards unless noted: position arithmetic at the container, slot and shard edges; signs and bases; dense, encoded and empty filters;
encoded against dense fields; a call that densifies in two chunks; the window taken from the minimum and maximum; the optimize()
encodings; the capacity protocol, counts, agreement with fbk_bsi_distinct; the foreign-key join of TestExecutor_ForeignIndex."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import datagen as D
import distinct_rows_ref as R
from featurebase_amd import lib as L
from featurebase_amd.roaring import Container

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SW = 1 << 20


def _container(vals):
    """sorted positions of one slot -> a run container when they are few long runs, else an array"""
    v = np.asarray(vals, dtype=np.int64)
    cuts = np.nonzero(np.diff(v) != 1)[0]
    if v.size >= 8 and cuts.size + 1 <= v.size // 4:
        starts = np.concatenate(([v[0]], v[cuts + 1]))
        lasts = np.concatenate((v[cuts], [v[-1]]))
        return Container.run([(int(a), int(b)) for a, b in zip(starts, lasts)])
    return Container.array(v)


def _fragment(n_sh, depth, columns, stored, extra=()):
    """BSI rows (exists, sign, planes) of `n_sh` shards as encoded fbk rows: column ids shard * 2^20 + position, stored values
    (sign-magnitude, |v| < 2^depth; `-0` is given as the string "-0").  extra: (shard, row of the fragment, position) bits set
    whatever exists says."""
    bits = [[[] for _ in range(depth + 2)] for _ in range(n_sh)]
    for c, v in zip(columns, stored):
        sh, p = int(c) >> 20, int(c) & (SW - 1)
        neg = v == "-0" or int(v) < 0
        mag = 0 if v == "-0" else abs(int(v))
        assert sh < n_sh and mag < (1 << depth)
        bits[sh][0].append(p)
        if neg:
            bits[sh][1].append(p)
        for i in range(depth):
            if (mag >> i) & 1:
                bits[sh][2 + i].append(p)
    for sh, r, p in extra:
        bits[sh][r].append(p)
    rows = []
    for sh in range(n_sh):
        for r in range(depth + 2):
            ps = np.unique(np.asarray(bits[sh][r], dtype=np.int64))
            row = {}
            for sl in np.unique(ps >> 16):
                row[int(sl)] = _container(ps[(ps >> 16) == sl] & 0xFFFF)
            rows.append(row)
    return rows


def _set_rows(n_sh, columns):
    """one row per shard holding `columns`"""
    ps = np.unique(np.asarray(list(columns), dtype=np.int64))
    rows = []
    for sh in range(n_sh):
        mine = ps[(ps >> 20) == sh] & (SW - 1)
        rows.append({int(sl): _container(mine[(mine >> 16) == sl] & 0xFFFF) for sl in np.unique(mine >> 16)})
    return rows


def _dense(ctx, rows):
    """the same rows as one dense batch"""
    W = np.zeros((len(rows), 16, 1024), dtype=np.uint64)
    for r, row in enumerate(rows):
        for sl, c in row.items():
            W[r, sl] = c.words()
    return ctx.upload_dense(W.reshape(-1))


def _base(n_sh, depth):
    return np.arange(n_sh, dtype=np.uint32) * (depth + 2)


def _check(out, expected):
    """(batch, pos_shards, neg_shards, counts) against {sign: {shard: positions}}; returns the downloaded rows"""
    batch, pos_sh, neg_sh, counts = out
    rows = batch.download()
    assert pos_sh.dtype == np.uint64 and counts.dtype == np.uint64
    assert pos_sh.tolist() == sorted(expected["pos"]), ("pos shards", pos_sh.tolist(), sorted(expected["pos"]))
    assert neg_sh.tolist() == sorted(expected["neg"]), ("neg shards", neg_sh.tolist(), sorted(expected["neg"]))
    n = pos_sh.size + neg_sh.size
    assert len(rows) == n + 1 and rows[n] == {} and counts.size == n
    want = [expected["pos"][s] for s in sorted(expected["pos"])] + [expected["neg"][s] for s in sorted(expected["neg"])]
    for r, (sh, exp) in enumerate(zip(pos_sh.tolist() + neg_sh.tolist(), want)):
        assert rows[r] and all(k >> 4 == sh for k in rows[r]), ("keys are shard * 16 + slot", r, sh, sorted(rows[r]))
        got = R.row_positions(rows[r])
        assert np.array_equal(got, exp), (r, sh, got[:8], exp[:8], got.size, exp.size)
        assert int(counts[r]) == exp.size == sum(c.n for c in rows[r].values()), ("cardinality", r)
        assert all(c.n == int(np.unpackbits(c.words().view(np.uint8)).sum()) for c in rows[r].values())
    return rows


def _run(ctx, n_sh, depth, columns, stored, base=0, filter_columns=None, extra=(), enc=True, enc_f=True, flags=0, keep=False):
    """one call on a fragment built from (columns, stored) checked against the yardstick"""
    rows = _fragment(n_sh, depth, columns, stored, extra)
    bS = ctx.upload(rows) if enc else _dense(ctx, rows)
    bF = None
    if filter_columns is not None:
        fr = _set_rows(n_sh, filter_columns)
        bF = ctx.upload(fr) if enc_f else _dense(ctx, fr)
    try:
        out = ctx.bsi_distinct_rows(bS, _base(n_sh, depth), depth, base, bF, np.arange(n_sh) if bF is not None else None, flags)
        plain = [0 if v == "-0" else int(v) for v in stored]
        exp = R.distinct_rows(columns, plain, base, filter_columns)
        got = _check(out, exp)
        if keep:
            return out, got
        out[0].free()
        return None, got
    finally:
        bS.free()
        if bF is not None:
            bF.free()


# ---- position arithmetic -------------------------------------------------------------------------------------------------------
EDGES = [0, 63, 64, 65535, 65536, SW - 1, SW, 3 * SW + 5]


@pytest.mark.parametrize("enc", [False, True])
def test_edges_of_position_arithmetic(gpu_ctx, enc):
    cols = [7 + 64 * i for i in range(len(EDGES))] + [SW + 5, SW + 6]  # the same values again in a second input shard: one bit each
    vals = EDGES + [64, 3 * SW + 5]
    _, rows = _run(gpu_ctx, 2, 22, cols, vals, enc=enc)
    assert len(rows) == 4  # shards 0, 1, 3 of Pos and the empty row
    assert sorted(rows[0]) == [0, 1, 15] and sorted(rows[1]) == [16] and sorted(rows[2]) == [48]


@pytest.mark.parametrize("base", [5, 0, -5, 3 * SW + 1, -(3 * SW + 1)])
def test_bit_depth_zero_is_the_single_position_abs_base(gpu_ctx, base):
    out, rows = _run(gpu_ctx, 2, 0, [1, 2, 70000, SW + 3], [0, 0, 0, 0], base, keep=True)
    batch, pos_sh, neg_sh, counts = out
    try:
        assert counts.tolist() == [1]
        assert (pos_sh.tolist(), neg_sh.tolist()) == (([abs(base) >> 20], []) if base >= 0 else ([], [abs(base) >> 20]))
        assert R.row_positions(rows[0]).tolist() == [abs(base)]
    finally:
        batch.free()


# ---- signs -----------------------------------------------------------------------------------------------------------------------
def test_signs_bases_and_bits_outside_exists(gpu_ctx):
    cols = [3, 4, 5, 6, 64, 65, 66, SW + 1, SW + 2, SW + 3]
    vals = [-5, 5, 0, "-0", -70000, 70000, -(SW + 9), 12, -12, 1]
    # sign and plane bits at columns that do not exist, in both shards
    extra = [(0, 1, 900), (0, 2, 900), (0, 9, 901), (1, 1, 77), (1, 20, 77), (0, 1, 5)]
    for base in (0, 100, -100, 70001, -70001, 12, -1, 1 << 30, -(1 << 30)):
        _, rows = _run(gpu_ctx, 2, 21, cols, vals, base, extra=extra)
    _, rows = _run(gpu_ctx, 2, 21, cols, vals, 0, extra=extra, enc=False)
    # stored negatives go to Neg, v == 0 (also a sign bit over magnitude 0) to Pos: Pos 0, 1, 5, 12, 70000 in shard 0
    assert R.row_positions(rows[0]).tolist() == [0, 1, 5, 12, 70000]
    assert R.row_positions(rows[1]).tolist() == [5, 12, 70000] and R.row_positions(rows[2]).tolist() == [SW + 9]
    # a base that carries every stored negative into Pos, and one that carries every stored positive into Neg
    out, rows = _run(gpu_ctx, 2, 21, cols, vals, 2 * SW, extra=extra, keep=True)
    assert out[2].size == 0 and out[1].tolist() == [0, 1, 2]
    out[0].free()
    out, rows = _run(gpu_ctx, 2, 21, cols, vals, -2 * SW, extra=extra, keep=True)
    assert out[1].size == 0 and out[2].tolist() == [1, 2, 3]
    out[0].free()


# ---- filter ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field():
    rng = D.rng_for(9980)
    cols = np.concatenate([rng.choice(3 * SW, 6000, replace=False), np.arange(SW + 4096, SW + 4096 + 512)])
    cols = np.unique(cols)
    vals = rng.integers(-(3 * SW), 3 * SW, cols.size)
    vals[(cols >= SW + 4096) & (cols < SW + 4096 + 512)] = 7  # a run of columns that hold one value: run containers when encoded
    return cols.tolist(), vals.tolist()


@pytest.mark.parametrize("enc_f", [False, True])
def test_filters(gpu_ctx, field, enc_f):
    cols, vals = field
    rng = D.rng_for(9981, int(enc_f))
    pick = set(c for c in cols if rng.random() < 0.3)
    outside = [c for c in range(100, 3 * SW, 9973) if c not in set(cols)]  # filter bits outside exists change nothing
    filt = sorted(pick | set(outside) | set(range(SW + 4096, SW + 4096 + 300)))  # (a run container in the encoded filter)
    _run(gpu_ctx, 3, 22, cols, vals, -17, filt, enc_f=enc_f)
    _run(gpu_ctx, 3, 22, cols, vals, 0, filt, enc=False, enc_f=enc_f)
    # an empty filter, and one that misses exists entirely: the one empty row
    for f in ([], outside):
        out, rows = _run(gpu_ctx, 3, 22, cols, vals, 5, f, enc_f=enc_f, keep=True)
        assert out[1].size == 0 and out[2].size == 0 and out[3].size == 0 and rows == [{}]
        out[0].free()


def test_no_shards_and_nothing_in_exists(gpu_ctx):
    bS = gpu_ctx.upload(_fragment(2, 10, [], []))
    try:
        for base_rows in ([], _base(2, 10)):
            batch, pos_sh, neg_sh, counts = gpu_ctx.bsi_distinct_rows(bS, base_rows, 10, 3)
            assert pos_sh.size == 0 and neg_sh.size == 0 and counts.size == 0 and batch.download() == [{}]
            batch.free()
    finally:
        bS.free()


# ---- encoded against dense ---------------------------------------------------------------------------------------------------
def test_encoded_and_dense_fields_download_identically(gpu_ctx, field):
    cols, vals = field
    rows = _fragment(3, 22, cols, vals)
    assert any(c.typ == L.TYPE_RUN for r in rows for c in r.values()) and any(c.typ == L.TYPE_ARRAY for r in rows for c in r.values())
    bE, bD = gpu_ctx.upload(rows), _dense(gpu_ctx, rows)
    try:
        flat = []
        for b in (bE, bD, bE):  # (the third: two runs of one input download identically)
            out = gpu_ctx.bsi_distinct_rows(b, _base(3, 22), 22, 1000)
            d, p, n = out[0].download_flat()
            flat.append((d.tobytes(), p.tobytes(), n, out[1].tobytes(), out[2].tobytes(), out[3].tobytes()))
            out[0].free()
        assert flat[0] == flat[1] == flat[2]
    finally:
        bE.free()
        bD.free()


# ---- chunking ------------------------------------------------------------------------------------------------------------------
def test_two_densify_chunks(gpu_ctx):
    """40 encoded shards at bit depth 62: 64 densified rows per shard allow 2^28 / (64 * 2^17) = 32 shards per chunk"""
    rng = D.rng_for(9982)
    n_sh, depth = 40, 62
    cols = np.unique(rng.choice(n_sh * SW, 4000, replace=False))
    vals = rng.integers(0, 5 * SW, cols.size)  # small values in wide planes
    vals[::7] = -vals[::7]
    big = (1 << 61) + 12345  # a common high part keeps the positions within a few shards: the base takes it away again
    stored = [int(v) + big for v in vals]
    rows = _fragment(n_sh, depth, cols.tolist(), stored)
    bE = gpu_ctx.upload(rows)
    bD = _dense(gpu_ctx, rows)
    try:
        outE = gpu_ctx.bsi_distinct_rows(bE, _base(n_sh, depth), depth, -big)
        _check(outE, R.distinct_rows(cols.tolist(), stored, -big))
        outD = gpu_ctx.bsi_distinct_rows(bD, _base(n_sh, depth), depth, -big)
        a, b = outE[0].download_flat(), outD[0].download_flat()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and outE[3].tolist() == outD[3].tolist()
        outE[0].free()
        outD[0].free()
    finally:
        bE.free()
        bD.free()


# ---- window by min / max -------------------------------------------------------------------------------------------------------
def test_window_from_minimum_and_maximum(gpu_ctx):
    rng = D.rng_for(9983)
    cols = np.unique(rng.choice(2 * SW, 3000, replace=False)).tolist()
    vals = [(1 << 40) + int(x) for x in rng.integers(0, 2 * SW, len(cols))]
    vals[0], vals[-1] = 1 << 40, (1 << 40) + 2 * SW - 1
    out, rows = _run(gpu_ctx, 2, 63, cols, vals, keep=True)
    assert out[1].tolist() == [SW, SW + 1] and out[2].size == 0
    out[0].free()
    out, _ = _run(gpu_ctx, 2, 63, cols, vals, 5, keep=True)  # (three rows: the top value moves into the next shard)
    assert out[1].tolist() == [SW, SW + 1, SW + 2]
    out[0].free()
    _run(gpu_ctx, 2, 63, cols, [-v for v in vals], 0, cols[::2])  # Neg, with a filter
    # values of both signs far from zero: each sign's window starts at its own smallest position, not at 0
    out, _ = _run(gpu_ctx, 2, 63, [5, 6, SW + 7], [-(1 << 44) - 3, (1 << 45) + 9, (1 << 45) + 2 * SW], keep=True)
    assert out[1].tolist() == [1 << 25, (1 << 25) + 2] and out[2].tolist() == [1 << 24]
    out[0].free()
    out, _ = _run(gpu_ctx, 2, 63, [5, 6, SW + 7], [-(1 << 44) - 3, (1 << 45) + 9, (1 << 45) + 2 * SW], 1 << 44, [5, 6, SW + 7, 99], keep=True)
    assert out[1].tolist() == [3 << 24, (3 << 24) + 2] and out[2].tolist() == [0]
    out[0].free()


def test_too_wide_and_overflow_are_errors_and_the_context_goes_on(gpu_ctx):
    depth = 63
    for vals, base, word in (([5, 5 + (1 << 44)], 0, "fbk_bsi_distinct"), ([-5, -5 - (1 << 44)], 3, "fbk_bsi_distinct"),
                             ([-5, 7, 7 + (1 << 44)], 0, "fbk_bsi_distinct"), ([1, (1 << 63) - 1], 1, "int64"), ([-((1 << 63) - 1), 4], -2, "int64")):
        bS = gpu_ctx.upload(_fragment(1, depth, list(range(10, 10 + len(vals))), vals))
        h, n_pos, n_neg = C.c_void_p(), C.c_uint32(9), C.c_uint32(9)
        ids = np.zeros(8, dtype=np.uint64)
        base_rows = _base(1, depth)
        try:
            rc = gpu_ctx.lib.fbk_bsi_distinct_rows(gpu_ctx.h, bS.h, base_rows.ctypes.data, depth, base, None, None, 1, 0, C.byref(h), ids.ctypes.data, 8,
                                                   C.byref(n_pos), C.byref(n_neg), None)
            assert rc == L.FBK_E_INVALID and word in gpu_ctx.last_error()[1], (vals, base, gpu_ctx.last_error())
            assert h.value is None
        finally:
            bS.free()
        _run(gpu_ctx, 1, 8, [1, 2, 3], [4, -4, 200], 1)  # the same context answers a small call


# ---- FBK_SETOP_OPTIMIZE --------------------------------------------------------------------------------------------------------
def test_optimize_gives_run_array_and_bitmap_containers_like_the_oracle(gpu_ctx, oracle):
    O = oracle
    rng = D.rng_for(9984)
    run = np.arange(1000, 4000)  # slot 0: consecutive ids
    few = 65536 + np.sort(rng.choice(65536, 3000, replace=False))  # slot 1: fewer than 4096 scattered values
    many = 2 * 65536 + np.sort(rng.choice(65536, 5000, replace=False))  # slot 2: 5000 scattered values
    vals = np.concatenate([run, few, many])
    cols = rng.choice(2 * SW, vals.size, replace=False)
    out, rows = _run(gpu_ctx, 2, 18, cols.tolist(), vals.tolist(), flags=L.SETOP_OPTIMIZE, keep=True)
    out[0].free()
    got = rows[0]
    assert [got[k].typ for k in (0, 1, 2)] == [L.TYPE_RUN, L.TYPE_ARRAY, L.TYPE_BITMAP] and sorted(got) == [0, 1, 2]
    for k, exp in ((0, run), (1, few - 65536), (2, many - 2 * 65536)):
        oc = O.optimize(O.OContainer.bitmap(D.words_of(exp)))
        assert got[k].typ == oc.typ and got[k].n == oc.n == exp.size
        assert np.array_equal(np.asarray(got[k].data).reshape(-1), np.asarray(oc.data()).reshape(-1)), k
    # without the flag: bitmaps
    _, rows = _run(gpu_ctx, 2, 18, cols.tolist(), vals.tolist())
    assert [rows[0][k].typ for k in (0, 1, 2)] == [L.TYPE_BITMAP] * 3


# ---- sizes and agreement -------------------------------------------------------------------------------------------------------
def test_capacity_protocol(gpu_ctx):
    cols, vals = [1, 2, 3, SW + 1], [5, SW + 5, -(2 * SW + 1), -3]  # Pos shards 0, 1; Neg shards 0, 2
    bS = gpu_ctx.upload(_fragment(2, 22, cols, vals))
    base_rows = _base(2, 22)
    try:
        for cap in (3, 0):
            h, n_pos, n_neg = C.c_void_p(1), C.c_uint32(9), C.c_uint32(9)
            ids, cnt = np.full(8, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64)
            rc = gpu_ctx.lib.fbk_bsi_distinct_rows(gpu_ctx.h, bS.h, base_rows.ctypes.data, 22, 0, None, None, 2, 0, C.byref(h), ids.ctypes.data, cap,
                                                   C.byref(n_pos), C.byref(n_neg), cnt.ctypes.data)
            assert rc == L.FBK_E_CAPACITY and (n_pos.value, n_neg.value) == (2, 2) and h.value is None
            assert (ids == 77).all() and (cnt == 77).all()
        out = gpu_ctx.bsi_distinct_rows(bS, base_rows, 22, cap=4)
        _check(out, R.distinct_rows(cols, vals))
        out[0].free()
        out = gpu_ctx.bsi_distinct_rows(bS, base_rows, 22, cap=1)  # the wrapper's retry
        assert out[1].tolist() == [0, 1] and out[2].tolist() == [0, 2] and out[3].tolist() == [1, 1, 1, 1]
        out[0].free()
    finally:
        bS.free()


def test_agrees_with_bsi_distinct_on_random_data(gpu_ctx):
    from test_gpu_extract import _case, _upload

    rng = D.rng_for(9985)
    depth, base = 21, -40000
    F, S, _ = _case(rng, 2, 1, depth)
    bS, bF = _upload(gpu_ctx, S, True), _upload(gpu_ctx, F, False)
    try:
        listed = gpu_ctx.bsi_distinct(bS, _base(2, depth), depth, bF, np.arange(2))
        out = gpu_ctx.bsi_distinct_rows(bS, _base(2, depth), depth, base, bF, np.arange(2))
        rows = _check(out, R.from_planes(S, F, depth, base))
        n_pos = out[1].size
        pos = np.concatenate([R.row_positions(r) for r in rows[:n_pos]]).astype(np.int64)
        neg = -np.concatenate([R.row_positions(r) for r in rows[n_pos:-1]]).astype(np.int64)
        assert listed.size > 10000 and neg.size > 1000  # (a condition on the inputs)
        assert np.array_equal(np.sort(np.concatenate([neg, pos])), listed + base)
        assert int(out[3].sum()) == listed.size
        again = gpu_ctx.bsi_distinct_rows(bS, _base(2, depth), depth, base, bF, np.arange(2))
        a, b = out[0].download_flat(), again[0].download_flat()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        out[0].free()
        again[0].free()
    finally:
        bS.free()
        bF.free()


# ---- join ----------------------------------------------------------------------------------------------------------------------
def test_foreign_index_join(gpu_ctx):
    """Intersect(Row(general=ShardWidth), Distinct(Row(color="blue"), index=child, field=parent_id)) == {one}"""
    fx = json.load(open(os.path.join(HERE, "golden", "foreign_index_vectors.json")))
    child, exp = fx["child"], fx["expected"]
    depth = child["parent_id_bit_depth"]
    cols = [int(c) for c in child["parent_id"]]
    vals = [child["parent_id"][str(c)] for c in cols]
    j = exp["join"]
    # the parent's general rows over two shards (its ids all lie in shard 0; shard 1 is there for the empty row to be named)
    general_ids = sorted(int(k) for k in fx["parent"]["general"])
    parent_rows = []
    for rid in general_ids:
        parent_rows += _set_rows(2, fx["parent"]["general"][str(rid)])
    bS = gpu_ctx.upload(_fragment(2, depth, cols, vals))
    bC = gpu_ctx.upload(_set_rows(2, child["color"][str(j["color_row"])]))
    bP = gpu_ctx.upload(parent_rows)
    try:
        every = gpu_ctx.bsi_distinct_rows(bS, _base(2, depth), depth, child["parent_id_base"])
        rows = _check(every, R.distinct_rows(cols, vals))
        assert R.row_positions(rows[0]).tolist() == exp["distinct_parent_id_pos"]
        every[0].free()
        blue = gpu_ctx.bsi_distinct_rows(bS, _base(2, depth), depth, child["parent_id_base"], bC, [0, 1], L.SETOP_OPTIMIZE)
        batch, pos_sh, neg_sh, _ = blue
        assert pos_sh.tolist() == [0] and neg_sh.size == 0
        empty = pos_sh.size + neg_sh.size
        g = general_ids.index(j["general_row"])
        # Pos on the parent's shards 0 and 1: Pos does not reach shard 1, so the empty row stands for it
        pos_rows = [int(np.nonzero(pos_sh == s)[0][0]) if s in pos_sh.tolist() else empty for s in (0, 1)]
        joined, counts = gpu_ctx.setop(L.OP_AND, bP, [2 * g, 2 * g + 1], batch, pos_rows)
        res = joined.download()
        assert counts.tolist() == [1, 0] and R.row_positions(res[0]).tolist() == j["result"] and res[1] == {}
        joined.free()
        batch.free()
        # Distinct(Row(parent_id=3), field=other): nothing selected, an empty SignedRow
        bO = gpu_ctx.upload(_fragment(1, 17, [], []))
        bN = gpu_ctx.upload(_set_rows(1, []))
        out = gpu_ctx.bsi_distinct_rows(bO, [0], 17, 0, bN, [0])
        assert out[1].size == 0 and out[2].size == 0 and out[0].download() == [{}]
        out[0].free()
        bO.free()
        bN.free()
    finally:
        for b in (bS, bC, bP):
            b.free()
