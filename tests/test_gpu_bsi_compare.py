"""GPU parity of fbk_bsi_compare (the Row of SQL WHERE x < y over two int fields): bit-exact equality, through download, with
the numpy recurrences of tests/compare_ref.py, which tests/test_bsi_compare_cpu.py pins to the Python-int definition.  One
wavefront per (shard, slot) has no cross-block state, so 1 and 3 shards reach every mechanism: depth pairs 0..64, all six
operators, with and without a filter, nil containers, different bases, the pinned general instance, the same field on both sides,
a differential against fbk_bsi_range, encoded batches, FBK_SETOP_OPTIMIZE, the count-only form, the errors, and a seeded fuzz."""
import numpy as np
import pytest

import compare_ref as CR
import datagen as D
import msum_ref as R
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DEPTH_PAIRS = [(0, 0), (1, 1), (3, 7), (7, 3), (63, 64), (64, 64), (64, 0)]


def _rnd(rng, shape, ands=0):
    w = rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    for _ in range(ands):
        w &= rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    return w


def _field(rng, n_sh, depth, exists_ands=0, low=True):
    """random planes and signs everywhere (so: set outside exists too); low: half of the words hold small magnitudes only (the
    planes from depth / 2 on are clear there), so that equal values and near ties occur at every depth"""
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    S[:, 0] &= _rnd(rng, (n_sh, 16, 1024), exists_ands)
    if low and depth:
        S[:, 2 + depth // 2:, :, ::2] = 0
        S[:, 2:, :, ::8] = 0  # and one word in eight holds +-0 only
    return S


def _up(ctx, S):
    return ctx.upload_dense(S.reshape(-1)), np.arange(S.shape[0], dtype=np.uint32) * S.shape[1]


def _words(batch, n_sh):
    """download -> [n_sh, 16, 1024] uint64; the container keys are shard * 16 + slot"""
    rows = batch.download()
    assert len(rows) == n_sh
    w = np.zeros((n_sh, 16, 1024), dtype=np.uint64)
    for s, row in enumerate(rows):
        for k, c in row.items():
            assert k >> 4 == s, (s, k)
            w[s, k & 15] = c.words()
    return w


def _call(ctx, x, y, op, filt=None, flags=0, base_x=0, base_y=0):
    """x, y: (batch, base_rows, depth); filt: (batch, rows) -> (words [n_sh, 16, 1024], counts)"""
    out, counts = ctx.bsi_compare(x[0], x[1], x[2], base_x, y[0], y[1], y[2], base_y, op, filt[0] if filt else None, filt[1] if filt else None, flags)
    try:
        return _words(out, len(x[1])), counts
    finally:
        out.free()


def _model(Sx, dx, bx, Sy, dy, by, F=None, flags=0):
    """(lt, gt, E) [n_sh, 16, 1024] by the recurrence of the instance the library takes"""
    parts = [CR.expected(Sx[s], dx, bx, Sy[s], dy, by, F[s] if F is not None else None, flags) for s in range(Sx.shape[0])]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


def _popcounts(w):
    return [CR.popcount(w[s]) for s in range(w.shape[0])]


def _check_all_ops(ctx, x, y, model, filt=None, flags=0, base_x=0, base_y=0, what=None):
    lt, gt, E = model
    got = {}
    for op in CR.OPS:
        w, counts = _call(ctx, x, y, op, filt, flags, base_x, base_y)
        assert (w == CR.combine(op, lt, gt, E)).all(), (what, op)
        assert counts.tolist() == _popcounts(w), (what, op)
        got[op] = w
    # LT, EQ, GT partition E; NEQ = E \ EQ; LTE = LT ∪ EQ
    assert ((got[CR.LT] | got[CR.EQ] | got[CR.GT]) == E).all()
    assert not (got[CR.LT] & got[CR.EQ]).any() and not (got[CR.LT] & got[CR.GT]).any() and not (got[CR.EQ] & got[CR.GT]).any()
    assert (got[CR.NEQ] == (E & ~got[CR.EQ])).all() and (got[CR.LTE] == (got[CR.LT] | got[CR.EQ])).all()
    return got


@pytest.mark.parametrize("n_sh", [1, 3])
@pytest.mark.parametrize("dx,dy", DEPTH_PAIRS)
def test_dense_batches(gpu_ctx, n_sh, dx, dy):
    rng = D.rng_for(9900, n_sh, dx, dy)
    Sx, Sy, F = _field(rng, n_sh, dx), _field(rng, n_sh, dy), _rnd(rng, (n_sh, 16, 1024))
    if n_sh > 1:
        Sx[1, 0] = 0  # a shard without values
    F[0, 3] = 0       # a nil container in the filter,
    Sy[0, 0, 5] = 0   # in exists_y
    if dx:
        Sx[0, 2 + dx // 2, 7] = 0  # and in a middle plane
    x, y, bf = _up(gpu_ctx, Sx) + (dx,), _up(gpu_ctx, Sy) + (dy,), gpu_ctx.upload_dense(F.reshape(-1))
    try:
        plain, filtered = _model(Sx, dx, 0, Sy, dy, 0), _model(Sx, dx, 0, Sy, dy, 0, F)
        assert CR.popcount(plain[2]) > CR.popcount(filtered[2]) > 0
        if dx and dy:
            assert plain[0].any() and plain[1].any()
        got = _check_all_ops(gpu_ctx, x, y, plain, what="plain")
        assert got[CR.EQ].any()  # (equal values exist at every depth pair: the +-0 words)
        _check_all_ops(gpu_ctx, x, y, filtered, (bf, np.arange(n_sh, dtype=np.uint32)), what="filtered")
    finally:
        for b in (x[0], y[0], bf):
            b.free()


@pytest.mark.parametrize("dx,dy", [(3, 7), (63, 64), (64, 0)])
def test_different_base(gpu_ctx, dx, dy):
    rng = D.rng_for(9910, dx, dy)
    Sx, Sy, F = _field(rng, 1, dx), _field(rng, 1, dy), _rnd(rng, (1, 16, 1024))
    x, y, bf = _up(gpu_ctx, Sx) + (dx,), _up(gpu_ctx, Sy) + (dy,), gpu_ctx.upload_dense(F.reshape(-1))
    try:
        for bx, by in ((1, 0), (0, 1), (1 << dx if dx < 63 else I64_MAX, 0), (I64_MAX, I64_MIN), (I64_MIN, I64_MAX), (-5, -5 - (1 << min(dx, 62)))):
            model = _model(Sx, dx, bx, Sy, dy, by)
            _check_all_ops(gpu_ctx, x, y, model, base_x=bx, base_y=by, what=(bx, by))
        model = _model(Sx, dx, 7, Sy, dy, 8, F)
        _check_all_ops(gpu_ctx, x, y, model, (bf, np.zeros(1, dtype=np.uint32)), base_x=7, base_y=8, what="filtered")
    finally:
        for b in (x[0], y[0], bf):
            b.free()


@pytest.mark.parametrize("dx,dy", [(0, 0), (7, 3), (64, 64)])
def test_pinned_general_instance_equals_the_default(gpu_ctx, dx, dy):
    rng = D.rng_for(9920, dx, dy)
    Sx, Sy = _field(rng, 3, dx), _field(rng, 3, dy)
    x, y = _up(gpu_ctx, Sx) + (dx,), _up(gpu_ctx, Sy) + (dy,)
    try:
        assert CR.steps(dx, dy, 0, CR.PATH_OFFSET) == max(dx, dy) + 2 and not CR.is_general(0, 0)
        sm, gen = _model(Sx, dx, 0, Sy, dy, 0), _model(Sx, dx, 0, Sy, dy, 0, flags=CR.PATH_OFFSET)
        assert all((a == b).all() for a, b in zip(sm, gen))
        for bx in (0, I64_MIN, 12345):  # equal bases: k == 0 whatever they are
            a = _check_all_ops(gpu_ctx, x, y, sm, base_x=bx, base_y=bx)
            b = _check_all_ops(gpu_ctx, x, y, gen, flags=L.COMPARE_PATH_OFFSET, base_x=bx, base_y=bx)
            assert all((a[op] == b[op]).all() for op in CR.OPS)
    finally:
        x[0].free()
        y[0].free()


@pytest.mark.parametrize("depth", [0, 20, 64])
def test_the_same_field_on_both_sides(gpu_ctx, depth):
    rng = D.rng_for(9930, depth)
    S = _field(rng, 3, depth)
    x = _up(gpu_ctx, S) + (depth,)
    try:
        for flags in (0, L.COMPARE_PATH_OFFSET):
            eq, _ = _call(gpu_ctx, x, x, L.BSI_EQ, flags=flags)
            lt, cnt = _call(gpu_ctx, x, x, L.BSI_LT, flags=flags)
            assert (eq == S[:, 0]).all() and not lt.any() and not cnt.any()
        gt, _ = _call(gpu_ctx, x, x, L.BSI_GT, base_x=1)  # x + 1 > x wherever x exists
        assert (gt == S[:, 0]).all()
    finally:
        x[0].free()


@pytest.mark.parametrize("c", [37, -37, "-0", 0])
def test_differential_against_bsi_range(gpu_ctx, c):
    """y holds the constant c in every existing column: value_x op value_y is fbk_bsi_range(x, op, c) ∩ exists_y.  (x holds no
    "-0": the reference never stores one, and its range scan, which fbk_bsi_range follows, reads a set sign as "negative" even
    over magnitude 0, where this call reads the value 0.)"""
    rng = D.rng_for(9940, 0 if c == "-0" else c + 100)
    dx, dy, n_sh = 7, 6, 3
    Sx = _field(rng, n_sh, dx, low=False)
    Sx[:, 1] &= np.bitwise_or.reduce(Sx[:, 2:], axis=1)
    Sy = np.zeros((n_sh, dy + 2, 16, 1024), dtype=np.uint64)
    Sy[:, 0] = _rnd(rng, (n_sh, 16, 1024))
    Sy[1, 0, 9] = 0
    mag = 0 if c == "-0" else abs(c)
    if c == "-0" or c < 0:
        Sy[:, 1] = CR.ONES  # (outside exists as well)
    for i in range(dy):
        if (mag >> i) & 1:
            Sy[:, 2 + i] = CR.ONES
    x, y = _up(gpu_ctx, Sx) + (dx,), _up(gpu_ctx, Sy) + (dy,)
    try:
        for name, op in L.BSI_OPS.items():
            rng_out, _ = gpu_ctx.bsi_range(x[0], x[1], op, dx, 0 if c == "-0" else c)
            try:
                want = _words(rng_out, n_sh) & Sy[:, 0]
            finally:
                rng_out.free()
            for flags in (0, L.COMPARE_PATH_OFFSET):
                got, counts = _call(gpu_ctx, x, y, op, flags=flags)
                assert (got == want).all(), (name, flags)
                assert counts.tolist() == _popcounts(want)
    finally:
        x[0].free()
        y[0].free()


def _encoded_field(rng, n_sh, depth):
    """fragments whose rows are datagen's container archetypes (arrays, bitmaps, runs, empty and missing containers) among
    exists, signs and planes -> (rows for upload, words [n_sh, depth + 2, 16, 1024])"""
    rows, S = [], np.zeros((n_sh, depth + 2, 16, 1024), dtype=np.uint64)
    for s in range(n_sh):
        for r in range(depth + 2):
            row = D.random_row(rng, 0, p_missing=0.1 if r == 0 else 0.25)
            S[s, r] = R.words_of_row(row)
            rows.append({(s * (depth + 2) + r) * 16 + k: D.to_fbk(c) for k, c in row.items()})
    return rows, S


def _up_encoded(ctx, rows, n_sh, depth):
    return ctx.upload(rows), np.arange(n_sh, dtype=np.uint32) * (depth + 2)


@pytest.mark.parametrize("layout", ["both", "x", "y"])
def test_encoded_batches(gpu_ctx, oracle, layout):
    """array and run containers among planes, exists, signs and filter, read as they are encoded; x encoded against y dense and
    the reverse"""
    rng = D.rng_for(9950, ["both", "x", "y"].index(layout))
    n_sh, dx, dy = 3, 5, 9
    rows_x, Sx = _encoded_field(rng, n_sh, dx)
    rows_y, Sy = _encoded_field(rng, n_sh, dy)
    f_rows = [D.random_row(rng, 0, p_missing=0.2) for _ in range(n_sh)]
    F = np.stack([R.words_of_row(r) for r in f_rows])
    x = (_up_encoded(gpu_ctx, rows_x, n_sh, dx) if layout in ("both", "x") else _up(gpu_ctx, Sx)) + (dx,)
    y = (_up_encoded(gpu_ctx, rows_y, n_sh, dy) if layout in ("both", "y") else _up(gpu_ctx, Sy)) + (dy,)
    bf = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        for bx in (0, -3):
            plain, filtered = _model(Sx, dx, bx, Sy, dy, 0), _model(Sx, dx, bx, Sy, dy, 0, F)
            assert CR.popcount(filtered[2]) > 1000
            _check_all_ops(gpu_ctx, x, y, plain, base_x=bx, what=(layout, bx))
            _check_all_ops(gpu_ctx, x, y, filtered, (bf, rf), base_x=bx, what=(layout, bx, "filtered"))
    finally:
        for b in (x[0], y[0], bf):
            b.free()


def _rows_of(batch):
    """download -> per row {key: (type, data bytes, n)}"""
    return [{k: (c.typ, np.asarray(c.data).tobytes(), c.n) for k, c in row.items()} for row in batch.download()]


@pytest.mark.parametrize("mode", [1, 2])
def test_optimize_encodes_as_bsi_range_does(gpu_ctx, mode):
    """FBK_SETOP_OPTIMIZE: the same bits as the plain call, and container for container what fbk_bsi_range yields for those bits
    (y: the constant 3 in every column, so the two calls have the same result) — under both setop_direct_encode settings"""
    rng = D.rng_for(9960)
    dx, dy, c = 4, 2, 3
    pack = lambda bits: np.packbits(bits, axis=1, bitorder="little").view(np.uint64)  # [rows, 65536] bool -> [rows, 1024] words
    Sx = np.zeros((1, dx + 2, 16, 1024), dtype=np.uint64)
    run = np.zeros((dx + 2, 1 << 16), dtype=bool)  # slot 0: columns 100..5999 hold 3 -> one run for EQ
    run[0, 100:6000] = run[2, 100:6000] = run[3, 100:6000] = True
    Sx[0, :, 0] = pack(run)
    few = np.zeros((dx + 2, 1 << 16), dtype=bool)  # slot 1: 150 columns with random values -> arrays
    pick = rng.choice(1 << 16, 150, replace=False)
    few[0, pick] = True
    few[1:, pick] = rng.random((dx + 1, pick.size)) < 0.5
    Sx[0, :, 1] = pack(few)
    Sx[0, :, 2] = _rnd(rng, (dx + 2, 1024))  # slot 2: random values in half of the columns -> bitmaps
    Sy = np.zeros((1, dy + 2, 16, 1024), dtype=np.uint64)
    Sy[0, 0] = CR.ONES
    Sy[0, 2] = Sy[0, 3] = CR.ONES
    x, y = _up(gpu_ctx, Sx) + (dx,), _up(gpu_ctx, Sy) + (dy,)
    try:
        gpu_ctx.set_option("setop_direct_encode", mode)
        kinds = set()
        for op in CR.OPS:
            plain, pc = _call(gpu_ctx, x, y, op)
            out, counts = gpu_ctx.bsi_compare(x[0], x[1], dx, 0, y[0], y[1], dy, 0, op, flags=L.SETOP_OPTIMIZE)
            ref, rc = gpu_ctx.bsi_range(x[0], x[1], op, dx, c, L.SETOP_OPTIMIZE)
            try:
                assert (_words(out, 1) == plain).all() and counts.tolist() == pc.tolist() == rc.tolist()
                got, want = _rows_of(out), _rows_of(ref)
                assert got == want, op
                kinds |= {v[0] for v in got[0].values()}
            finally:
                out.free()
                ref.free()
        assert kinds == {L.TYPE_ARRAY, L.TYPE_BITMAP, L.TYPE_RUN}
    finally:
        gpu_ctx.set_option("setop_direct_encode", 2)
        x[0].free()
        y[0].free()


def test_count_only_form(gpu_ctx):
    rng = D.rng_for(9970)
    n_sh, dx, dy = 3, 9, 12
    Sx, Sy, F = _field(rng, n_sh, dx), _field(rng, n_sh, dy), _rnd(rng, (n_sh, 16, 1024))
    x, y, bf = _up(gpu_ctx, Sx) + (dx,), _up(gpu_ctx, Sy) + (dy,), gpu_ctx.upload_dense(F.reshape(-1))
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        before = [b.memory() for b in (x[0], y[0], bf)]
        for bx, flags in ((0, 0), (0, L.COMPARE_PATH_OFFSET), (-2, 0)):
            for filt in (None, (bf, rf)):
                for op in CR.OPS:
                    _, want = _call(gpu_ctx, x, y, op, filt, flags, base_x=bx)
                    none, counts = gpu_ctx.bsi_compare(x[0], x[1], dx, bx, y[0], y[1], dy, 0, op, filt[0] if filt else None, filt[1] if filt else None,
                                                       flags, count_only=True)
                    assert none is None and counts.tolist() == want.tolist() and counts.sum() > 0, (bx, flags, op)
        assert [b.memory() for b in (x[0], y[0], bf)] == before
    finally:
        for b in (x[0], y[0], bf):
            b.free()


def test_errors_leave_the_context_usable(gpu_ctx):
    rng = D.rng_for(9980)
    n_sh, dx, dy = 2, 8, 5
    Sx, Sy = _field(rng, n_sh, dx), _field(rng, n_sh, dy)
    (bx, rx), (by, ry) = _up(gpu_ctx, Sx), _up(gpu_ctx, Sy)
    try:
        want = CR.combine(CR.LT, *_model(Sx, dx, 0, Sy, dy, 0))
        ok = lambda: _call(gpu_ctx, (bx, rx, dx), (by, ry, dy), L.BSI_LT)[0]
        assert (ok() == want).all()
        bad = rx.copy()
        bad[1] = n_sh * (dx + 2) - 1  # the fragment's rows run past the batch
        cases = [
            dict(depth_x=65), dict(depth_y=65), dict(op=0), dict(op=7), dict(flags=2), dict(flags=0x200), dict(rx=bad),
            dict(filt=by, rows_f=np.array([0, n_sh * (dy + 2)], dtype=np.uint32)),
        ]
        for kw in cases:
            a = dict(depth_x=dx, depth_y=dy, op=L.BSI_LT, flags=0, rx=rx, filt=None, rows_f=None)
            a.update(kw)
            with pytest.raises(L.FbkError) as e:
                gpu_ctx.bsi_compare(bx, a["rx"], a["depth_x"], 0, by, ry, a["depth_y"], 0, a["op"], a["filt"], a["rows_f"], a["flags"])
            assert e.value.code == L.FBK_E_INVALID, kw
            assert (ok() == want).all(), kw
        # NULL arguments with a live context, and both outputs NULL
        lib, h = gpu_ctx.lib, L.C.c_void_p()
        cnt = np.zeros(n_sh, dtype=np.uint64)
        o, c = L.C.byref(h), cnt.ctypes.data
        for args in ((gpu_ctx.h, None, rx.ctypes.data, dx, 0, by.h, ry.ctypes.data, dy, 0, L.BSI_LT, None, None, n_sh, 0, o, c),
                     (gpu_ctx.h, bx.h, rx.ctypes.data, dx, 0, None, ry.ctypes.data, dy, 0, L.BSI_LT, None, None, n_sh, 0, o, c),
                     (gpu_ctx.h, bx.h, None, dx, 0, by.h, ry.ctypes.data, dy, 0, L.BSI_LT, None, None, n_sh, 0, o, c),
                     (gpu_ctx.h, bx.h, rx.ctypes.data, dx, 0, by.h, None, dy, 0, L.BSI_LT, None, None, n_sh, 0, o, c),
                     (gpu_ctx.h, bx.h, rx.ctypes.data, dx, 0, by.h, ry.ctypes.data, dy, 0, L.BSI_LT, by.h, None, n_sh, 0, o, c),
                     (gpu_ctx.h, bx.h, rx.ctypes.data, dx, 0, by.h, ry.ctypes.data, dy, 0, L.BSI_LT, None, None, n_sh, 0, None, None)):
            assert lib.fbk_bsi_compare(*args) == L.FBK_E_INVALID
            assert h.value is None and (ok() == want).all()
        # no shards: FBK_OK with an empty batch
        out, counts = gpu_ctx.bsi_compare(bx, rx[:0], dx, 0, by, ry[:0], dy, 0, L.BSI_LT)
        assert out.download() == [] and counts.size == 0
        out.free()
    finally:
        bx.free()
        by.free()


def test_fuzz(gpu_ctx, oracle):
    """30 seeded cases over the structural dimensions: depth pair, operator, k, filter or none, dense or encoded on each side,
    optimize, count-only"""
    rng = D.rng_for(9990)
    depths = [0, 1, 2, 5, 13, 31, 32, 33, 63, 64]
    for case in range(30):
        dx, dy = int(rng.choice(depths)), int(rng.choice(depths))
        n_sh = int(rng.integers(1, 3))
        k = [0, 0, 1, -1, 1 << dx if dx < 63 else 5, -(1 << dy) if dy < 63 else -5, int(rng.integers(-1 << 40, 1 << 40)), (1 << 64) - 1, -((1 << 64) - 1)][int(rng.integers(0, 9))]
        base_y = 0 if abs(k) < 1 << 63 else (I64_MIN if k > 0 else I64_MAX)
        base_x = base_y + k
        assert I64_MIN <= base_x <= I64_MAX
        enc_x, enc_y, with_f, optimize, count_only = (bool(rng.integers(0, 2)) for _ in range(5))
        flags = (L.SETOP_OPTIMIZE if optimize else 0) | (L.COMPARE_PATH_OFFSET if rng.integers(0, 2) else 0)
        op = CR.OPS[int(rng.integers(0, 6))]
        what = (case, dx, dy, k, op, enc_x, enc_y, with_f, flags, count_only)
        if enc_x and dx <= 13:
            rows, Sx = _encoded_field(rng, n_sh, dx)
            x = _up_encoded(gpu_ctx, rows, n_sh, dx) + (dx,)
        else:
            Sx = _field(rng, n_sh, dx)
            x = _up(gpu_ctx, Sx) + (dx,)
        if enc_y and dy <= 13:
            rows, Sy = _encoded_field(rng, n_sh, dy)
            y = _up_encoded(gpu_ctx, rows, n_sh, dy) + (dy,)
        else:
            Sy = _field(rng, n_sh, dy)
            y = _up(gpu_ctx, Sy) + (dy,)
        F, filt = None, None
        if with_f:
            f_rows = [D.random_row(rng, 0, p_missing=0.2) for _ in range(n_sh)]
            F = np.stack([R.words_of_row(r) for r in f_rows])
            filt = (gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows]), np.arange(n_sh, dtype=np.uint32))
        try:
            want = CR.combine(op, *_model(Sx, dx, base_x, Sy, dy, base_y, F, flags))
            out, counts = gpu_ctx.bsi_compare(x[0], x[1], dx, base_x, y[0], y[1], dy, base_y, op, filt[0] if filt else None, filt[1] if filt else None,
                                              flags, count_only=count_only)
            assert counts.tolist() == _popcounts(want), what
            if not count_only:
                try:
                    assert (_words(out, n_sh) == want).all(), what
                finally:
                    out.free()
        finally:
            for b in (x[0], y[0]) + ((filt[0],) if filt else ()):
                b.free()
