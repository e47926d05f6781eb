"""GPU parity of fbk_bsi_sort (Sort(filter, field=, sort-desc=, limit=, offset=) by an int field) and fbk_extract_open_columns:
bit-exact against the numpy brute force of tests/sort_ref.py (the CPU test shows it agrees with the reference's procedure on the
oracle's rows wherever that is deterministic).  Dense and encoded field / filter in every combination, no filter, empty filter,
no shards; bit depths 0 .. 64; negative-only, positive-only and mixed fields; stored zeros dropped (the reference) or kept;
ascending and descending; ties (few distinct values, a tie run cut inside a 64-column word across a shard boundary, all columns
equal); offset / limit boundaries, the capacity protocol, *out_total; identities with fbk_bsi_min / _max / _distinct and
fbk_extract_columns; more than 2^31 columns under a limit; column-list handles against filter handles; the golden query."""
import ctypes as C

import numpy as np
import pytest

import datagen as D
import extract_ref as X
import sort_ref as R
from featurebase_amd import lib as L
from test_gpu_extract import _case, _rnd, _upload
from test_sort_cpu import GOLD, golden_filter, golden_fragment

pytestmark = pytest.mark.gpu

U64MAX = (1 << 64) - 1
ONES = np.uint64(U64MAX)


def _base(n_sh, depth):
    return np.arange(n_sh, dtype=np.uint32) * (depth + 2)


def _check(ctx, bS, S, depth, ids, bF=None, F=None, desc=False, keep_zero=False, offset=0, limit=None, base=None, rows_f=None, expect=None):
    """one call against the brute force (or `expect` = (columns, values, total) computed by the caller)"""
    n_sh = len(ids)
    base = _base(n_sh, depth) if base is None else base
    rows_f = np.arange(n_sh, dtype=np.uint32) if rows_f is None else rows_f
    cols, vals, total = ctx.bsi_sort(bS, base, depth, ids, bF, rows_f if bF is not None else None, desc=desc, keep_zero=keep_zero, offset=offset, limit=limit)
    ec, ev, et = R.brute(S, F, ids, depth, desc, keep_zero, offset, limit) if expect is None else expect
    what = (depth, desc, keep_zero, offset, limit)
    assert total == et, ("total", what, total, et)
    assert cols.dtype == np.uint64 and vals.dtype == np.int64
    assert np.array_equal(vals, ev), ("values", what)
    assert np.array_equal(cols, ec), ("columns", what)
    return cols, vals, total


@pytest.fixture(scope="module")
def small():
    rng = D.rng_for(9100)
    F, S, _ = _case(rng, 3, 1, 20)
    return F, S


@pytest.mark.parametrize("enc_s", [False, True])
@pytest.mark.parametrize("enc_f", [False, True])
def test_dense_and_encoded_combinations(gpu_ctx, small, enc_s, enc_f):
    F, S = small
    ids = [0, 1, 4]
    bS, bF = _upload(gpu_ctx, S, enc_s), _upload(gpu_ctx, F, enc_f)
    try:
        for desc in (False, True):
            for kz in (False, True):
                c, v, total = _check(gpu_ctx, bS, S, 20, ids, bF, F, desc, kz, 500, 1000)
                assert c.size == 1000 and total > 100000
            c, v, total = _check(gpu_ctx, bS, S, 20, ids, bF, F, desc, True)  # no limit: every record
            assert c.size == total and (v == 0).any() and (v < 0).any() and (v > 0).any()
        if not enc_f:  # no filter: every column of exists
            for desc in (False, True):
                _check(gpu_ctx, bS, S, 20, ids, None, None, desc, False, 77, 4000)
                _check(gpu_ctx, bS, S, 20, ids, None, None, desc, True)
    finally:
        bS.free()
        bF.free()


@pytest.mark.parametrize("enc", [False, True])
def test_empty_filter_and_no_shards(gpu_ctx, small, enc):
    F, S = small
    Z = np.zeros_like(F)
    bS, bZ = _upload(gpu_ctx, S, enc), _upload(gpu_ctx, Z, enc)
    try:
        for lim in (None, 10, 0):
            c, v, total = _check(gpu_ctx, bS, S, 20, [0, 1, 4], bZ, Z, limit=lim, keep_zero=True)
            assert c.size == 0 and total == 0
        c, v, total = gpu_ctx.bsi_sort(bS, [], 20, [], bZ, [], limit=5)
        assert c.size == 0 and v.size == 0 and total == 0
        c, v, total = gpu_ctx.bsi_sort(bS, [], 20, [])
        assert c.size == 0 and total == 0
    finally:
        bS.free()
        bZ.free()


@pytest.mark.parametrize("depth", [0, 1, 20, 63, 64])
def test_bit_depths(gpu_ctx, depth):
    rng = D.rng_for(9200, depth)
    n_sh = 3
    F, S, _ = _case(rng, n_sh, 1, depth, 3)
    F[1] = 0  # a shard with an empty filter row
    ids = [0, 5, (1 << 40) + 3]
    bS, bF = _upload(gpu_ctx, S, depth == 20), _upload(gpu_ctx, F, False)
    try:
        for desc in (False, True):
            for kz in (False, True):
                c, v, total = _check(gpu_ctx, bS, S, depth, ids, bF, F, desc, kz)
                _check(gpu_ctx, bS, S, depth, ids, bF, F, desc, kz, 100, 300)
                if depth == 0:
                    assert total == (c.size if kz else 0) and (v == 0).all()
                else:
                    assert (v < 0).any() and (v > 0).any() and ((v == 0).any() == kz)
                if depth == 64 and kz:
                    # magnitudes >= 2^63 wrap: a positive sign with the top plane set is a negative value
                    assert int(v.min() if not desc else v.max()) == int(v[0]) and (np.abs(v.astype(np.float64)) > 2.0**62).any()
        assert int(c.max()) >> 20 == (1 << 40) + 3
    finally:
        bS.free()
        bF.free()


@pytest.mark.parametrize("sign", ["negative", "positive"])
def test_one_signed_fields(gpu_ctx, sign):
    rng = D.rng_for(9300, len(sign))
    depth, n_sh = 12, 2
    F, S, _ = _case(rng, n_sh, 1, depth, 2)
    S[:, 1] = ONES if sign == "negative" else 0
    bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, True)
    try:
        for desc in (False, True):
            c, v, _ = _check(gpu_ctx, bS, S, depth, [3, 4], bF, F, desc, False, 0, 5000)
            assert ((v < 0) if sign == "negative" else (v > 0)).all()
            _check(gpu_ctx, bS, S, depth, [3, 4], bF, F, desc, True, 10, None)
    finally:
        bS.free()
        bF.free()


def test_stored_zeros(gpu_ctx):
    """columns of magnitude 0, with and without the sign bit, between negative and positive values"""
    rng = D.rng_for(9400)
    depth, n_sh = 6, 2
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    S[:, 0] = ONES
    S[:, 2:, 3] = 0  # slot 3: magnitude 0 under random sign bits
    S[:, 2:, 7, :100] = 0
    bS = _upload(gpu_ctx, S, False)
    try:
        for desc in (False, True):
            c0, v0, t0 = _check(gpu_ctx, bS, S, depth, [0, 1], desc=desc)
            c1, v1, t1 = _check(gpu_ctx, bS, S, depth, [0, 1], desc=desc, keep_zero=True)
            assert not (v0 == 0).any() and t1 - t0 == int((v1 == 0).sum()) >= 2 * (65536 + 6400)
            z = c1[v1 == 0]
            assert (np.diff(z.astype(np.int64)) > 0).all()  # the zeros in ascending column order, whatever their sign bit
            assert np.array_equal(c1[v1 != 0], c0)
            neg = int((v1 < 0).sum())
            _check(gpu_ctx, bS, S, depth, [0, 1], desc=desc, keep_zero=True, offset=(int((v1 > 0).sum()) if desc else neg) + 65000, limit=2000)
    finally:
        bS.free()


def test_ties(gpu_ctx):
    rng = D.rng_for(9500)
    # few distinct values over many columns
    depth, n_sh = 2, 3
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    F = _rnd(rng, (n_sh, 16, 1024))
    bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, False)
    try:
        for desc in (False, True):
            c, v, total = _check(gpu_ctx, bS, S, depth, [1, 2, 7], bF, F, desc, True)
            assert np.unique(v).size == 7
            for off, lim in ((0, 1), (12345, 100), (total // 2, 65), (total - 3, 10), (0, 1 << 19)):
                _check(gpu_ctx, bS, S, depth, [1, 2, 7], bF, F, desc, True, off, lim)
                _check(gpu_ctx, bS, S, depth, [1, 2, 7], bF, F, desc, False, off, lim)
    finally:
        bS.free()
        bF.free()
    # a tie run that crosses a shard boundary and is cut inside a 64-column word: ten columns of value 1, then value 5 on the last
    # 100 columns of shard 0 and the first 100 of shard 1, everything else larger
    depth, n_sh = 8, 2
    val = rng.integers(6, 200, (n_sh, 1 << 20))
    val[0, -100:] = 5
    val[1, :100] = 5
    val[0, 1000:1005] = 1
    val[1, 70000:70005] = 1
    S = np.zeros((n_sh, depth + 2, 1 << 20), dtype=np.uint8)
    S[:, 0] = 1
    for p in range(depth):
        S[:, 2 + p] = (val >> p) & 1
    S = np.packbits(S, axis=-1, bitorder="little").view(np.uint64).reshape(n_sh, depth + 2, 16, 1024)
    bS = _upload(gpu_ctx, S, False)
    try:
        for lim in (10 + 100 + 37, 10 + 100, 10 + 99, 10 + 100 + 64, 10 + 100 + 1, 10 + 200, 10 + 201, 5, 10, 11):
            c, v, _ = _check(gpu_ctx, bS, S, depth, [0, 1], limit=lim)
            _check(gpu_ctx, bS, S, depth, [0, 1], limit=10, offset=max(lim - 10, 0))
        c, v, _ = _check(gpu_ctx, bS, S, depth, [0, 1], limit=147)
        assert v[10:].tolist() == [5] * 137 and c[110:].tolist() == list(range(1 << 20, (1 << 20) + 37))
        # descending: the same run is the smallest, at the END of the order; equal values still in ascending column id
        total = 2 << 20
        c, v, _ = _check(gpu_ctx, bS, S, depth, [0, 1], desc=True, offset=total - 10 - 200 + 63, limit=100)
        assert (v == 5).all() and (np.diff(c.astype(np.int64)) > 0).all() and int(c[0]) == (1 << 20) - 37
    finally:
        bS.free()
    # all columns equal (negative)
    S = np.zeros((2, 5, 16, 1024), dtype=np.uint64)
    S[:, :3] = ONES
    S[:, 4] = ONES  # -5 everywhere
    bS = _upload(gpu_ctx, S, False)
    try:
        for desc in (False, True):
            for off, lim in ((0, 3), ((1 << 20) - 30, 64), (2 << 20, 5), ((2 << 20) - 1, 5)):
                c, v, total = _check(gpu_ctx, bS, S, 3, [6, 7], desc=desc, offset=off, limit=lim)
                assert total == 2 << 20 and (v == -5).all()
    finally:
        bS.free()


def test_offset_limit_boundaries_capacity_and_total(gpu_ctx):
    rng = D.rng_for(9600)
    depth, n_sh = 9, 3
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    F = np.zeros((n_sh, 16, 1024), dtype=np.uint64)
    F[:, 0, :30] = _rnd(rng, (n_sh, 30))
    F[:, 15, 1000:] = _rnd(rng, (n_sh, 24), 1)
    ids = [2, 3, 9]
    bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, True)
    try:
        _, _, total = R.brute(S, F, ids, depth)
        assert 500 < total < 5000
        vals = [0, 1, total - 1, total, total + 1, U64MAX]
        for desc in (False, True):
            for off in vals:
                for lim in vals:
                    _check(gpu_ctx, bS, S, depth, ids, bF, F, desc, False, off, None if lim == U64MAX else lim)
        # the raw protocol: *out_n always set, too small a capacity leaves the outputs untouched, *out_total may be NULL
        base, rf, sid = _base(n_sh, depth), np.arange(n_sh, dtype=np.uint32), np.array(ids, dtype=np.uint64)
        cols, vs, n, tot = np.full(64, 0xABCD, dtype=np.uint64), np.full(64, -77, dtype=np.int64), C.c_uint64(5), C.c_uint64(5)

        def raw(off, lim, cap, ptot):
            return gpu_ctx.lib.fbk_bsi_sort(gpu_ctx.h, bS.h, base.ctypes.data, depth, bF.h, rf.ctypes.data, sid.ctypes.data, n_sh, 0, off, lim, cols.ctypes.data,
                                            vs.ctypes.data, cap, C.byref(n), ptot)

        assert raw(3, 100, 64, C.byref(tot)) == L.FBK_E_CAPACITY and n.value == 100 and tot.value == total
        assert (cols == 0xABCD).all() and (vs == -77).all()
        assert raw(3, 100, 0, None) == L.FBK_E_CAPACITY and n.value == 100
        assert raw(total - 10, U64MAX, 64, None) == L.FBK_OK and n.value == 10
        ec, ev, _ = R.brute(S, F, ids, depth, False, False, total - 10, None)
        assert np.array_equal(cols[:10], ec) and np.array_equal(vs[:10], ev) and (cols[10:] == 0xABCD).all()
        assert raw(total, 5, 0, C.byref(tot)) == L.FBK_OK and n.value == 0 and tot.value == total
        c, v, t = gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf, cap=1)  # the wrapper retries once with the reported size
        assert c.size == total == t
        # row indices out of range and unknown flags are refused with a device present, too
        bad = base.copy()
        bad[1] = S.shape[0] * (depth + 2) - 3
        with pytest.raises(L.FbkError):
            gpu_ctx.bsi_sort(bS, bad, depth, ids, bF, rf)
        with pytest.raises(L.FbkError):
            gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf + 1)
    finally:
        bS.free()
        bF.free()


def test_identities_with_existing_calls(gpu_ctx, small):
    F, S = small
    n_sh, depth, ids = 3, 20, [0, 1, 2]
    bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, False)
    base, rf = _base(n_sh, depth), np.arange(n_sh, dtype=np.uint32)
    try:
        for desc, fold in ((False, gpu_ctx.bsi_min), (True, gpu_ctx.bsi_max)):
            c, v, total = gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf, desc=desc, keep_zero=True, limit=1)
            ext, cnt = fold(bS, base, depth, bF, rf)
            best = (max if desc else min)(int(e) for e, k in zip(ext, cnt) if k)
            assert int(v[0]) == best and total == int(gpu_ctx.bsi_sum(bS, base, depth, bF, rf)[1].sum())
            call, vall, _ = gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf, desc=desc, keep_zero=True)
            assert int(c[0]) == int(call[vall == best].min())
        cols, vals, total = gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf, keep_zero=True)
        assert np.array_equal(np.unique(vals), gpu_ctx.bsi_distinct(bS, base, depth, bF, rf))
        cols, vals, total = gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf)
        EF = S[:, 0] & F
        bEF = _upload(gpu_ctx, EF, False)
        try:
            with gpu_ctx.extract(bEF, rf, ids) as h:
                ecols = h.columns()
                ev, ep = h.bsi(bS, base, depth)
            assert ep.all() and np.array_equal(np.sort(cols), ecols[ev != 0])
            lookup = dict(zip(ecols.tolist(), ev.tolist()))
            assert [lookup[c] for c in cols[:5000].tolist()] == vals[:5000].tolist()  # the VALUE is fbk_extract_bsi's
        finally:
            bEF.free()
    finally:
        bS.free()
        bF.free()


def test_more_than_2_31_columns_with_a_limit(gpu_ctx):
    """2 200 shards that all name the same fragment and the same all-ones filter row: 2 200 x 2^20 > 2^31 columns take part, every
    value's tie run spans all shards, the cut falls inside one.  The brute force is one fragment and arithmetic."""
    rng = D.rng_for(9700)
    n_sh, depth = 2200, 8
    S = _rnd(rng, (1, depth + 2, 16, 1024))
    S[0, 0] = ONES
    F = np.full((1, 16, 1024), ONES, dtype=np.uint64)
    pos = np.arange(1 << 20, dtype=np.int64)
    v1, p1 = X.bsi_expected(S, depth, np.zeros(1 << 20, dtype=np.int64), pos)
    assert p1.all()
    ids = np.arange(n_sh, dtype=np.uint64) * 3 + 1
    total = n_sh << 20
    assert total > 1 << 31

    def expect(desc, off, lim):
        uniq = np.unique(v1)[::-1] if desc else np.unique(v1)
        per = np.array([(v1 == x).sum() for x in uniq], dtype=np.int64)  # columns of the value in ONE shard
        start = np.concatenate(([0], np.cumsum(per * n_sh)))  # first rank of every value's run
        t = np.arange(off, off + lim, dtype=np.int64)
        k = np.searchsorted(start, t, side="right") - 1
        within = t - start[k]
        by_value = {int(x): pos[v1 == x] for x in uniq[np.unique(k)]}
        cols = np.array([(int(ids[w // per[j]]) << 20) + int(by_value[int(uniq[j])][w % per[j]]) for j, w in zip(k, within)], dtype=np.uint64)
        return cols, uniq[k].astype(np.int64), total

    bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, False)
    base, rf = np.zeros(n_sh, dtype=np.uint32), np.zeros(n_sh, dtype=np.uint32)
    try:
        for desc in (False, True):
            for off in (0, 1 << 20):
                c, v, t = _check(gpu_ctx, bS, S, depth, ids, bF, F, desc, True, off, 1000, base=base, rows_f=rf, expect=expect(desc, off, 1000))
                assert c.size == 1000 and t == total
        with pytest.raises(L.FbkError) as ei:
            gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf, keep_zero=True)
        assert ei.value.code == L.FBK_E_INVALID and "limit" in str(ei.value)
        with pytest.raises(L.FbkError) as ei:
            gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf, keep_zero=True, offset=(1 << 31) - 5, limit=5)  # K = 2^31
        assert ei.value.code == L.FBK_E_INVALID
    finally:
        bS.free()
        bF.free()


def test_encoded_operands_in_several_chunks(gpu_ctx):
    """encoded field and filter past the 2^28-byte scratch: 200 shards x (8 + 2 + 1) rows x 2^17 bytes = two chunks of 100"""
    rng = D.rng_for(9800)
    n_sh, depth = 200, 8
    S1 = np.zeros((2, depth + 2, 16, 1024), dtype=np.uint64)
    S1[:, :, 3, 100:104] = _rnd(rng, (2, depth + 2, 4))
    S1[:, :, 9, 500:502] = _rnd(rng, (2, depth + 2, 2))
    F1 = np.zeros((2, 16, 1024), dtype=np.uint64)
    F1[:, 3, 100:104] = _rnd(rng, (2, 4))
    F1[:, 9, 500:502] = ONES
    pick = (np.arange(n_sh) % 2).astype(np.uint32)
    S, F = S1[pick], F1[pick]
    ids = np.arange(n_sh) * 2 + 5
    bS, bF = _upload(gpu_ctx, S1, True), _upload(gpu_ctx, F1, True)
    try:
        for desc in (False, True):
            _check(gpu_ctx, bS, S, depth, ids, bF, F, desc, False, 100, 3000, base=pick * (depth + 2), rows_f=pick)
            _check(gpu_ctx, bS, S, depth, ids, bF, F, desc, True, base=pick * (depth + 2), rows_f=pick)
    finally:
        bS.free()
        bF.free()


# ---- fbk_extract_open_columns ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", [False, True])
def test_open_columns_against_open_on_the_equivalent_filter(gpu_ctx, enc):
    rng = D.rng_for(9900, int(enc))
    n_sh, n_a, depth = 5, 3, 20
    _, S, A = _case(rng, n_sh, n_a, depth)
    ids = np.array([0, 1, 4, 1 << 30, (1 << 30) + 3], dtype=np.uint64)
    bS, bA = _upload(gpu_ctx, S, enc), _upload(gpu_ctx, A, enc)
    base, ra = _base(n_sh, depth), np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    try:
        for n, shards in ((1, [2]), (5000, [1, 2, 3]), (70000, [0, 1, 2, 3, 4]), (300, [4]), (64, [0, 3])):
            sh = rng.choice(shards, n)
            pos = rng.integers(0, 1 << 20, n)
            pos[: n // 4] = rng.integers(0, 200, n // 4)  # dense corners: many columns in a few words
            cols = np.unique((ids[sh] << np.uint64(20)) + pos.astype(np.uint64))
            cols = cols[rng.permutation(cols.size)]
            F = np.zeros((n_sh, 16 * 1024), dtype=np.uint64)
            s_of = np.searchsorted(ids, cols >> np.uint64(20))
            p_of = (cols & np.uint64(0xFFFFF)).astype(np.int64)
            np.bitwise_or.at(F, (s_of, p_of >> 6), np.uint64(1) << (p_of & 63).astype(np.uint64))
            bF = _upload(gpu_ctx, F.reshape(n_sh, 16, 1024), False)
            try:
                h1, rank = gpu_ctx.extract_columns(cols, ids)
                with h1, gpu_ctx.extract(bF, np.arange(n_sh), ids) as h2:
                    assert h1.n == h2.n == cols.size and h1.span() == h2.span()
                    sorted_cols = h2.columns()
                    assert np.array_equal(h1.columns(), sorted_cols) and np.array_equal(sorted_cols[rank], cols)
                    v1, p1 = h1.bsi(bS, base, depth)
                    v2, p2 = h2.bsi(bS, base, depth)
                    assert np.array_equal(v1, v2) and np.array_equal(p1, p2)
                    o1, i1 = h1.rows(bA, ra)
                    o2, i2 = h2.rows(bA, ra)
                    assert np.array_equal(o1, o2) and np.array_equal(i1, i2)
                    sh_i, pos_i, _ = X.select(F.reshape(n_sh, 16, 1024), ids)
                    ev, ep = X.bsi_expected(S, depth, sh_i, pos_i)
                    assert np.array_equal(v1[rank], ev[rank]) and np.array_equal(p1, ep)
            finally:
                bF.free()
    finally:
        bS.free()
        bA.free()


def test_open_columns_rejects_duplicates_and_foreign_shards(gpu_ctx):
    ids = np.array([2, 5], dtype=np.uint64)
    for cols, word in (([(2 << 20) + 7, (5 << 20) + 1, (2 << 20) + 7], "twice"), ([(2 << 20) + 7, (3 << 20) + 1], "shard"), ([7], "shard"),
                       ([(6 << 20)], "shard")):
        with pytest.raises(L.FbkError) as ei:
            gpu_ctx.extract_columns(cols, ids)
        assert ei.value.code == L.FBK_E_INVALID and word in str(ei.value)
    with pytest.raises(L.FbkError):
        gpu_ctx.extract_columns([5], [])
    for sid in (ids, []):
        h, rank = gpu_ctx.extract_columns([], sid)  # n == 0: a valid, empty handle
        with h:
            assert h.n == 0 and rank.size == 0 and h.columns().size == 0 and h.span() == (0, 0)
    h, rank = gpu_ctx.extract_columns([(5 << 20) + 9], ids)
    with h:
        assert h.span() == (1, 1) and h.columns().tolist() == [(5 << 20) + 9] and rank.tolist() == [0]


# ---- the golden query, end to end ---------------------------------------------------------------------------------------------------
def test_golden_query_end_to_end(gpu_ctx):
    """Extract(Sort(Row(bsint > 1), field = bsint, limit = 2, offset = 1), Rows(bsint)) of the reference's TestExecutor_Sort"""
    q = GOLD["queries"][0]
    depth, S, vals = golden_fragment()
    bS = _upload(gpu_ctx, S, True)
    try:
        import re

        k = int(re.fullmatch(r"Row\(bsint > (-?\d+)\)", q["filter"]).group(1))
        bF, counts = gpu_ctx.bsi_range(bS, [0], L.BSI_GT, depth, k)
        try:
            assert np.array_equal(bF.download()[0][0].words() if 0 in bF.download()[0] else None, golden_filter(q, vals)[0, 0])
            cols, v, total = gpu_ctx.bsi_sort(bS, [0], depth, [0], bF, [0], desc=q["desc"], offset=q["offset"], limit=q["limit"])
            assert total == int(counts.sum()) == 3
            h, rank = gpu_ctx.extract_columns(cols, [0])
            with h:
                ev, ep = h.bsi(bS, [0], depth)
            table = [{"column": int(c), "rows": [int(ev[r])]} for c, r in zip(cols, rank) if ep[r]]
            assert table == q["columns"] and v.tolist() == [c["rows"][0] for c in q["columns"]]
        finally:
            bF.free()
    finally:
        bS.free()
