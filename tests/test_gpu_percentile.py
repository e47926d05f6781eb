"""GPU parity of fbk_bsi_quantiles (the values at several ranks of an int field in one radix select) and fbk_bsi_percentile
(Percentile(field=, nth=, filter=) replayed from four of them): bit-exact against np.sort and against the reference's search loop
restated in tests/pct_ref.py (the CPU test shows the loop and the replay agree).  Dense and encoded field / filter in every
combination, no filter, empty filter, no shards; the bit depths of every pass count and of the 64-bit key; one-signed fields, stored
zeros, all columns equal, few distinct values; ranks at and past the ends, from the top, repeated, more ranks than one launch has
prefixes, 1024 ranks, none; identities with fbk_bsi_min / _max / _sort; several densify chunks; two contexts at once."""
import threading

import numpy as np
import pytest

import datagen as D
import pct_ref as P
from featurebase_amd import lib as L
from test_gpu_extract import _case, _rnd, _upload

pytestmark = pytest.mark.gpu

T = L.RANK_FROM_TOP
ONES = np.uint64((1 << 64) - 1)
NTHS = [0, 100, 50, 25, 75, 99, 1, 0.1, 99.9, 33.3]
EXITS = {"min", "max", "balanced", "bounds"}


def _base(n_sh, depth):
    return np.arange(n_sh, dtype=np.uint32) * (depth + 2)


def _ranks_for(n, rng=None, extra=()):
    r = [0, n - 1 if n else 0, n, n + 5, T | 0, T | (n - 1 if n else 0), T | n, n // 2, n // 2, n // 3, 7, 7, T | 7, T | (n // 4)] + list(extra)
    if rng is not None and n:
        r += [int(x) for x in rng.integers(0, n, 8)]
    return r


def _check_q(ctx, bS, vals, depth, ranks, bF=None, base=None, rows_f=None, n_sh=None):
    """one fbk_bsi_quantiles call against np.sort of `vals` (the values of exists ∩ filter)"""
    base = _base(n_sh, depth) if base is None else base
    rows_f = np.arange(len(base), dtype=np.uint32) if rows_f is None else rows_f
    gv, gc, gt = ctx.bsi_quantiles(bS, base, depth, ranks, bF, rows_f if bF is not None else None)
    ev, ec, et = P.quantiles(vals, ranks)
    assert gv.dtype == np.int64 and gc.dtype == np.uint64
    assert gt == et, ("total", depth, gt, et)
    assert np.array_equal(gv, ev), ("values", depth, [hex(int(r)) for r in ranks], gv, ev)
    assert np.array_equal(gc, ec), ("counts", depth, gc, ec)
    return gv, gc, gt


def _check_p(ctx, bS, vals, depth, nths, fbase=0, bF=None, base=None, rows_f=None, n_sh=None):
    """one fbk_bsi_percentile call against the search loop; returns the exits the cases took"""
    base = _base(n_sh, depth) if base is None else base
    rows_f = np.arange(len(base), dtype=np.uint32) if rows_f is None else rows_f
    gv, gc, gt = ctx.bsi_percentile(bS, base, depth, nths, fbase, bF, rows_f if bF is not None else None)
    assert gt == vals.size and gv.size == gc.size == len(nths)
    exits = set()
    for i, nth in enumerate(nths):
        want = P.percentile_search(vals, float(nth), fbase)
        if want is None:
            assert int(gc[i]) == 0 and int(gv[i]) == 0
            continue
        assert (int(gv[i]), int(gc[i])) == want[:2], ("percentile", depth, nth, fbase, int(gv[i]), int(gc[i]), want)
        exits.add(want[2])
    return exits


@pytest.fixture(scope="module")
def small():
    rng = D.rng_for(9960)
    F, S, _ = _case(rng, 3, 1, 20)
    return F, S, P.values(S, F, 20), P.values(S, None, 20)


@pytest.mark.parametrize("enc_s", [False, True])
@pytest.mark.parametrize("enc_f", [False, True])
def test_dense_and_encoded_combinations(gpu_ctx, small, enc_s, enc_f):
    F, S, vf, va = small
    rng = D.rng_for(9961, int(enc_s), int(enc_f))
    bS, bF = _upload(gpu_ctx, S, enc_s), _upload(gpu_ctx, F, enc_f)
    try:
        assert vf.size > 50000 and (vf == 0).any() and (vf < 0).any() and (vf > 0).any()
        _check_q(gpu_ctx, bS, vf, 20, _ranks_for(vf.size, rng), bF, n_sh=3)
        for fbase in (0, -12345, 1 << 40):
            _check_p(gpu_ctx, bS, vf, 20, NTHS, fbase, bF, n_sh=3)  # the list in ONE call
        for nth in NTHS:  # and each alone
            _check_p(gpu_ctx, bS, vf, 20, [nth], -12345, bF, n_sh=3)
        if not enc_f:  # no filter: every column of exists
            _check_q(gpu_ctx, bS, va, 20, _ranks_for(va.size, rng), n_sh=3)
            _check_p(gpu_ctx, bS, va, 20, NTHS, 1 << 40, n_sh=3)
    finally:
        bS.free()
        bF.free()


@pytest.mark.parametrize("enc", [False, True])
def test_empty_filter_no_shards_and_no_ranks(gpu_ctx, small, enc):
    F, S, vf, va = small
    Z = np.zeros_like(F)
    none = np.zeros(0, dtype=np.int64)
    bS, bZ, bF = _upload(gpu_ctx, S, enc), _upload(gpu_ctx, Z, enc), _upload(gpu_ctx, F, enc)
    try:
        gv, gc, gt = _check_q(gpu_ctx, bS, none, 20, [0, 5, T | 0, T | 9], bZ, n_sh=3)
        assert gt == 0 and not gc.any() and not gv.any()
        assert _check_p(gpu_ctx, bS, none, 20, NTHS, 77, bZ, n_sh=3) == set()  # the median of nothing
        for filt, rf in ((bZ, []), (None, None)):
            gv, gc, gt = gpu_ctx.bsi_quantiles(bS, [], 20, [0, T | 0, 3], filt, rf)
            assert gt == 0 and gv.tolist() == [0, 0, 0] and gc.tolist() == [0, 0, 0]
            gv, gc, gt = gpu_ctx.bsi_percentile(bS, [], 20, [0, 50, 100], 5, filt, rf)
            assert gt == 0 and gv.tolist() == [0, 0, 0] and gc.tolist() == [0, 0, 0]
        # no ranks: the count alone
        gv, gc, gt = gpu_ctx.bsi_quantiles(bS, _base(3, 20), 20, [], bF, np.arange(3))
        assert gv.size == 0 and gc.size == 0 and gt == vf.size
        gv, gc, gt = gpu_ctx.bsi_quantiles(bS, _base(3, 20), 20, [])
        assert gt == va.size == int(gpu_ctx.bsi_sum(bS, _base(3, 20), 20)[1].sum())
        gv, gc, gt = gpu_ctx.bsi_percentile(bS, _base(3, 20), 20, [], 0, bF, np.arange(3))
        assert gv.size == 0 and gt == vf.size
    finally:
        for b in (bS, bZ, bF):
            b.free()


@pytest.mark.parametrize("depth", [0, 1, 10, 11, 12, 21, 22, 33, 62, 63, 64])
def test_bit_depths(gpu_ctx, depth):
    """every pass count (1 .. 6) and the 64-bit key; bit depth 64: magnitudes >= 2^63 wrap to negative values"""
    rng = D.rng_for(9962, depth)
    n_sh = 2
    F, S, _ = _case(rng, n_sh, 1, depth, 3)
    vals = P.values(S, F, depth)
    bS, bF = _upload(gpu_ctx, S, depth in (12, 33)), _upload(gpu_ctx, F, depth == 22)
    try:
        assert vals.size > 10000
        gv, gc, gt = _check_q(gpu_ctx, bS, vals, depth, _ranks_for(vals.size, rng), bF, n_sh=n_sh)
        if depth == 0:
            assert not gv.any() and int(gc[0]) == vals.size
        elif depth > 1:
            assert int(gv[0]) < 0 < int(gv[4])
        if depth == 64:
            assert float(np.abs(vals.astype(np.float64)).max()) > 2.0**62
        exits = _check_p(gpu_ctx, bS, vals, depth, NTHS, 0, bF, n_sh=n_sh)
        assert {"min", "max"} <= exits
        if depth <= 33:
            _check_p(gpu_ctx, bS, vals, depth, NTHS, -(1 << 45) + 3, bF, n_sh=n_sh)
    finally:
        bS.free()
        bF.free()


def test_base_overflow_is_an_error(gpu_ctx):
    rng = D.rng_for(9963)
    F, S, _ = _case(rng, 1, 1, 63, 3)
    bS = _upload(gpu_ctx, S, False)
    try:
        with pytest.raises(L.FbkError) as ei:
            gpu_ctx.bsi_percentile(bS, [0], 63, [50], (1 << 62) + 5)
        assert ei.value.code == L.FBK_E_INVALID and "int64" in str(ei.value)
        with pytest.raises(L.FbkError):
            gpu_ctx.bsi_quantiles(bS, [3], 63, [0])  # rows past the batch
    finally:
        bS.free()


def test_one_signed_fields_zeros_equal_and_few_distinct(gpu_ctx):
    rng = D.rng_for(9964)
    depth, n_sh = 12, 2
    F, S, _ = _case(rng, n_sh, 1, depth, 2)
    for sign in ("negative", "positive"):
        S[:, 1] = ONES if sign == "negative" else 0
        vals = P.values(S, F, depth)
        assert ((vals <= 0) if sign == "negative" else (vals >= 0)).all() and (vals == 0).any() and (vals != 0).any()
        bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, True)
        try:
            _check_q(gpu_ctx, bS, vals, depth, _ranks_for(vals.size, rng), bF, n_sh=n_sh)
            _check_p(gpu_ctx, bS, vals, depth, NTHS, 9, bF, n_sh=n_sh)
        finally:
            bS.free()
            bF.free()
    # stored zeros, with and without the sign bit, between negative and positive values: they take part
    depth = 6
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    S[:, 0] = ONES
    S[:, 2:, 3] = 0
    S[:, 2:, 7, :100] = 0
    vals = P.values(S, None, depth)
    zeros = int((vals == 0).sum())
    assert zeros >= 2 * (65536 + 6400)
    bS = _upload(gpu_ctx, S, False)
    try:
        neg = int((vals < 0).sum())
        gv, gc, gt = _check_q(gpu_ctx, bS, vals, depth, [neg - 1, neg, neg + zeros - 1, neg + zeros, T | 0, 0], n_sh=n_sh)
        assert gv[1] == 0 and gv[2] == 0 and gc[1] == zeros and gv[0] == -1 and gv[3] == 1 and gt == n_sh << 20
        _check_p(gpu_ctx, bS, vals, depth, NTHS, 0, n_sh=n_sh)
    finally:
        bS.free()
    # few distinct values over many columns (the one-add path of a word whose columns share a bin), then all columns equal
    depth = 2
    S = _rnd(rng, (3, depth + 2, 16, 1024))
    F = _rnd(rng, (3, 16, 1024))
    vals = P.values(S, F, depth)
    bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, False)
    try:
        assert np.unique(vals).size == 7
        _check_q(gpu_ctx, bS, vals, depth, _ranks_for(vals.size, rng), bF, n_sh=3)
        _check_p(gpu_ctx, bS, vals, depth, NTHS + [12.5, 60, 87.5], -2, bF, n_sh=3)
    finally:
        bS.free()
        bF.free()
    S = np.zeros((2, 5, 16, 1024), dtype=np.uint64)
    S[:, :3] = ONES
    S[:, 4] = ONES  # -5 everywhere
    vals = P.values(S, None, 3)
    bS = _upload(gpu_ctx, S, False)
    try:
        gv, gc, gt = _check_q(gpu_ctx, bS, vals, 3, _ranks_for(vals.size, rng), n_sh=2)
        assert gt == 2 << 20 and int(gv[0]) == -5 and int(gc[0]) == 2 << 20
        assert _check_p(gpu_ctx, bS, vals, 3, NTHS, 5, n_sh=2) <= {"min", "max", "bounds"}
    finally:
        bS.free()


@pytest.mark.parametrize("depth", [21, 33])
def test_more_prefixes_than_one_launch_holds(gpu_ctx, depth):
    """9 and 17 ranks whose values differ pairwise in the digits above the last pass: more than 8 live prefixes, so a pass takes two
    and three walks; then 1024 ranks in one call"""
    rng = D.rng_for(9965, depth)
    n_sh = 2
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    vals = P.values(S, None, depth)
    s = np.sort(vals)
    bS = _upload(gpu_ctx, S, False)
    try:
        for n in (9, 17):
            ranks = [int(k) for k in np.linspace(0, s.size - 1, n).astype(np.int64)]
            top = {(int(s[k]) + (1 << depth)) >> 11 for k in ranks}  # everything above the last digit
            assert len(top) == n
            if depth == 21:
                assert len({(int(s[k]) + (1 << depth)) >> 11 for k in ranks}) == n  # two passes: they are the top digits
            mixed = [r if i % 2 else T | (s.size - 1 - r) for i, r in enumerate(ranks)]
            _check_q(gpu_ctx, bS, vals, depth, ranks, n_sh=n_sh)
            _check_q(gpu_ctx, bS, vals, depth, mixed[::-1], n_sh=n_sh)
        ranks = [int(x) for x in rng.integers(0, s.size + 100, 1024)]
        ranks[100:120] = ranks[0:20]
        ranks[500:600] = [T | r for r in ranks[500:600]]
        gv, gc, gt = _check_q(gpu_ctx, bS, vals, depth, ranks, n_sh=n_sh)
        assert np.unique(gv).size > 900
        with pytest.raises(L.FbkError) as ei:
            gpu_ctx.bsi_quantiles(bS, _base(n_sh, depth), depth, ranks + [0])
        assert ei.value.code == L.FBK_E_INVALID and "1024" in str(ei.value)
        nths = list(np.linspace(0, 100, 256))
        _check_p(gpu_ctx, bS, vals, depth, nths, 3, n_sh=n_sh)
        with pytest.raises(L.FbkError):
            gpu_ctx.bsi_percentile(bS, _base(n_sh, depth), depth, nths + [1.0])
    finally:
        bS.free()


def test_identities_with_existing_calls(gpu_ctx, small):
    F, S, vf, va = small
    n_sh, depth, ids = 3, 20, [0, 1, 2]
    bS, bF = _upload(gpu_ctx, S, False), _upload(gpu_ctx, F, False)
    base, rf = _base(n_sh, depth), np.arange(n_sh, dtype=np.uint32)
    try:
        gv, gc, gt = gpu_ctx.bsi_quantiles(bS, base, depth, [0, T | 0], bF, rf)
        for k, fold, pick in ((0, gpu_ctx.bsi_min, min), (1, gpu_ctx.bsi_max, max)):
            ext, cnt = fold(bS, base, depth, bF, rf)
            best = pick(int(e) for e, c in zip(ext, cnt) if c)
            assert int(gv[k]) == best and int(gc[k]) == sum(int(c) for e, c in zip(ext, cnt) if c and int(e) == best)
        assert gt == int(gpu_ctx.bsi_sum(bS, base, depth, bF, rf)[1].sum())
        s = np.sort(vf)
        ks = [0, 1, 999, gt // 2, gt - 1]
        gv, gc, _ = gpu_ctx.bsi_quantiles(bS, base, depth, ks, bF, rf)
        for k, v, c in zip(ks, gv, gc):
            _, sv, st = gpu_ctx.bsi_sort(bS, base, depth, ids, bF, rf, keep_zero=True, offset=k, limit=1)
            assert st == gt and int(sv[0]) == int(v) and int(c) == int((s == v).sum())
    finally:
        bS.free()
        bF.free()


def test_small_selections_take_all_four_exits(gpu_ctx):
    """a few columns under sparse filters, tie-heavy and spread values: the search loop leaves by each of its four exits"""
    rng = D.rng_for(9966)
    n_sh = 3
    exits = set()
    for depth, fbase in ((2, 0), (20, -500), (40, 1 << 41)):
        S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
        S[:, 0] = ONES
        bS = _upload(gpu_ctx, S, depth == 20)
        try:
            for n in (1, 2, 3, 7, 20, 64, 150):
                F = np.zeros((n_sh, 16 * 1024), dtype=np.uint64)
                sh, pos = rng.integers(0, n_sh, n), rng.integers(0, 1 << 20, n)
                np.bitwise_or.at(F, (sh, pos >> 6), np.uint64(1) << (pos & 63).astype(np.uint64))
                F = F.reshape(n_sh, 16, 1024)
                vals = P.values(S, F, depth)
                assert 0 < vals.size <= n
                bF = _upload(gpu_ctx, F, n % 2 == 0)
                try:
                    _check_q(gpu_ctx, bS, vals, depth, _ranks_for(vals.size, rng), bF, n_sh=n_sh)
                    exits |= _check_p(gpu_ctx, bS, vals, depth, NTHS + [float(x) for x in rng.uniform(0, 100, 6)], fbase, bF, n_sh=n_sh)
                finally:
                    bF.free()
        finally:
            bS.free()
    assert exits == EXITS, exits


def test_encoded_operands_in_several_chunks(gpu_ctx):
    """encoded field and filter past the 2^28-byte scratch: 200 shards x (8 + 2 + 1) rows x 2^17 bytes = two chunks of 100; the dense
    upload of the same rows is read in place, in one chunk"""
    rng = D.rng_for(9967)
    n_sh, depth = 200, 8
    S1 = np.zeros((2, depth + 2, 16, 1024), dtype=np.uint64)
    S1[:, :, 3, 100:104] = _rnd(rng, (2, depth + 2, 4))
    S1[:, :, 9, 500:502] = _rnd(rng, (2, depth + 2, 2))
    F1 = np.zeros((2, 16, 1024), dtype=np.uint64)
    F1[:, 3, 100:104] = _rnd(rng, (2, 4))
    F1[:, 9, 500:502] = ONES
    pick = (np.arange(n_sh) % 2).astype(np.uint32)
    vals = P.values(S1[pick], F1[pick], depth)
    ranks = _ranks_for(vals.size, rng)
    got = []
    for enc in (True, False):
        bS, bF = _upload(gpu_ctx, S1, enc), _upload(gpu_ctx, F1, enc)
        try:
            q = _check_q(gpu_ctx, bS, vals, depth, ranks, bF, base=pick * (depth + 2), rows_f=pick)
            _check_p(gpu_ctx, bS, vals, depth, NTHS, 11, bF, base=pick * (depth + 2), rows_f=pick)
            p = gpu_ctx.bsi_percentile(bS, pick * (depth + 2), depth, NTHS, 11, bF, pick)
            got.append((q[0].tolist(), q[1].tolist(), q[2], p[0].tolist(), p[1].tolist(), p[2]))
        finally:
            bS.free()
            bF.free()
    assert got[0] == got[1]


def test_two_forked_contexts_at_once(gpu_ctx, small):
    F, S, vf, va = small
    bS, bF = _upload(gpu_ctx, S, True), _upload(gpu_ctx, F, False)
    base, rf = _base(3, 20), np.arange(3, dtype=np.uint32)
    ranks = _ranks_for(vf.size, D.rng_for(9968))
    forks = [gpu_ctx.fork(), gpu_ctx.fork()]
    out, errs = [None, None], []

    def run(i):
        try:
            res = []
            for _ in range(4):
                q = forks[i].bsi_quantiles(bS, base, 20, ranks, bF, rf)
                p = forks[i].bsi_percentile(bS, base, 20, NTHS, -7, bF, rf)
                res.append((q[0].tolist(), q[1].tolist(), q[2], p[0].tolist(), p[1].tolist(), p[2]))
            out[i] = res
        except Exception as e:  # noqa: BLE001 (reported below, on the main thread)
            errs.append(e)

    try:
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        ev, ec, et = P.quantiles(vf, ranks)
        for res in out:
            for r in res:
                assert r == out[0][0]
        assert out[0][0][0] == ev.tolist() and out[0][0][1] == ec.tolist() and out[0][0][2] == et
    finally:
        for f in forks:
            f.close()
        bS.free()
        bF.free()
