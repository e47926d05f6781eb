"""GPU parity of fbk_bsi_moments (the raw moments behind SQL VAR and CORR): exact equality with the reference model of
tests/moments_ref.py (decode every column, sum in Python ints, modulo 2^128; tests/test_bsi_moments_cpu.py pins the model to the
definition).  Dense batches over shard counts and depth pairs 0..64 with and without a filter; the one-field form; x and y the
same field; the inputs on which a late i32 flush or a 32-bit cross-slot sum goes wrong; encoded batches through the densify path
in two chunks; recovery after an error; the model's decode against the oracle's fragment for sampled columns."""
import numpy as np
import pytest

import datagen as D
import moments_ref as M
import msum_ref as R
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B(oracle):
    from oracle import pybsi

    pybsi._lib()
    return pybsi


def _rnd(rng, shape, ands=0):
    w = rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    for _ in range(ands):
        w &= rng.integers(0, 1 << 63, shape, dtype=np.uint64) * 2 + rng.integers(0, 2, shape, dtype=np.uint64)
    return w


def _field(rng, n_sh, depth, exists_ands=1):
    """random planes and signs everywhere (so: set outside exists too), exists thinned by ANDs"""
    S = _rnd(rng, (n_sh, depth + 2, 16, 1024))
    S[:, 0] &= _rnd(rng, (n_sh, 16, 1024), exists_ands)
    return S


def _up(ctx, S):
    return ctx.upload_dense(S.reshape(-1)), np.arange(S.shape[0], dtype=np.uint32) * S.shape[1]


def _same(got, want):
    assert tuple(got) == tuple(want), (got, want)


# n_shards in {1, 3, 17} x the seven depth pairs, each with and without a filter.  The 17-shard cases read 3 distinct random
# fragments of x, 4 of y and 2 filter rows through aliasing base_rows (shard s: x s % 3, y s % 4, filter s % 2 — twelve distinct
# (x, y) pairs), so that 17 shards of 63 + 64 planes cost 7 fragments to make and decode, not 34.  (17, 64, 64) is 1088 units
# over the launch's blocks: the unpacked kernel walks more than one unit in a block and crosses a shard boundary there.
DEPTH_PAIRS = [(0, 0), (1, 1), (7, 8), (8, 7), (20, 13), (63, 64), (64, 64)]
DENSE_CASES = [(n_sh, dx, dy) for n_sh in (1, 3, 17) for dx, dy in DEPTH_PAIRS]
# the kernel packs 4 (2) column blocks into its tile when the call has at most 8 (16) rows of the byte matrix: both sides of both
# thresholds — 8, 9, 16 and 17 rows; and the one-sided (0, 64)
DENSE_CASES += [(1, 28, 21), (1, 28, 28), (1, 56, 49), (1, 56, 56), (3, 0, 64)]


def _aliased(n_sh):
    """(fragments of x, of y, filter rows, ix, iy, ifl) of a case: distinct per shard up to 3 shards, aliased beyond"""
    if n_sh <= 3:
        r = list(range(n_sh))
        return n_sh, n_sh, n_sh, r, r, r
    return 3, 4, 2, [s % 3 for s in range(n_sh)], [s % 4 for s in range(n_sh)], [s % 2 for s in range(n_sh)]


@pytest.mark.parametrize("n_sh,dx,dy", DENSE_CASES)
def test_dense_batches(gpu_ctx, n_sh, dx, dy):
    rng = D.rng_for(9300, n_sh, dx, dy)
    assert M.rows_of(dx, dy)[3] == {(28, 21): 8, (28, 28): 9, (56, 49): 16, (56, 56): 17}.get((dx, dy), M.rows_of(dx, dy)[3])
    nx, ny, nf, ix, iy, ifl = _aliased(n_sh)
    Sx, Sy, F = _field(rng, nx, dx), _field(rng, ny, dy, exists_ands=0), _rnd(rng, (nf, 16, 1024))
    if nx > 2:
        Sx[1, 0] = 0  # a shard (several, when aliased) without values
    F[0, 3] = 0  # an empty container in the filter
    (bx, rx), (by, ry), bf = _up(gpu_ctx, Sx), _up(gpu_ctx, Sy), gpu_ctx.upload_dense(F.reshape(-1))
    rx, ry, rf = rx[ix], ry[iy], np.asarray(ifl, dtype=np.uint32)
    try:
        plain, filtered = M.expected_each(Sx, dx, Sy, dy, [None, F], ix, iy, ifl)
        assert plain.n > filtered.n > 0
        _same(gpu_ctx.bsi_moments(bx, rx, dx, by, ry, dy), plain)
        _same(gpu_ctx.bsi_moments(bx, rx, dx, by, ry, dy, bf, rf), filtered)
    finally:
        for b in (bx, by, bf):
            b.free()


@pytest.mark.parametrize("dx,dy,n_sh", [(20, 13, 300), (32, 32, 150), (0, 64, 150), (63, 64, 80)])
def test_blocks_that_walk_several_units(gpu_ctx, dx, dy, n_sh):
    """random fragments read by many shards (aliasing base_rows): more units than the launch has blocks for every packing — 16 units
    per shard at 4 column blocks per tile, 32 at 2, 64 unpacked — so a block walks several units, of different shards"""
    rng = D.rng_for(9350, dx, dy)
    ix, iy, ifl = [s % 3 for s in range(n_sh)], [s % 2 for s in range(n_sh)], [s % 2 for s in range(n_sh)]
    Sx, Sy, F = _field(rng, 3, dx), _field(rng, 2, dy, exists_ands=0), _rnd(rng, (2, 16, 1024))
    rows = M.rows_of(dx, dy)[3]
    units = n_sh * 64 // (4 if rows <= 8 else 2 if rows <= 16 else 1)
    assert units >= 4 * 1024  # every block of a launch of at most 1024 blocks takes four units or more
    (bx, rx), (by, ry), bf = _up(gpu_ctx, Sx), _up(gpu_ctx, Sy), gpu_ctx.upload_dense(F.reshape(-1))
    try:
        plain, filtered = M.expected_each(Sx, dx, Sy, dy, [None, F], ix, iy, ifl)
        _same(gpu_ctx.bsi_moments(bx, rx[ix], dx, by, ry[iy], dy), plain)
        _same(gpu_ctx.bsi_moments(bx, rx[ix], dx, by, ry[iy], dy, bf, np.asarray(ifl, dtype=np.uint32)), filtered)
    finally:
        for b in (bx, by, bf):
            b.free()


@pytest.mark.parametrize("depth", [0, 7, 20, 64])
def test_one_field_form_and_the_same_field_twice(gpu_ctx, depth):
    rng = D.rng_for(9400, depth)
    n_sh = 3
    S, F = _field(rng, n_sh, depth, exists_ands=2), _rnd(rng, (n_sh, 16, 1024))
    (bs, rs), bf = _up(gpu_ctx, S), gpu_ctx.upload_dense(F.reshape(-1))
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        plain, filtered = M.expected_each(S, depth, None, 0, [None, F])
        assert plain.sum_y == plain.sum_yy == plain.sum_xy == 0
        _same(gpu_ctx.bsi_moments(bs, rs, depth), plain)
        _same(gpu_ctx.bsi_moments(bs, rs, depth, filt=bf, rows_f=rf), filtered)
        twice = gpu_ctx.bsi_moments(bs, rs, depth, bs, rs, depth, bf, rf)  # the same batch and the same field
        _same(twice, M.expected(S, depth, S, depth, F))
        assert twice.sum_xy == twice.sum_xx == twice.sum_yy == filtered.sum_xx and twice.sum_y == twice.sum_x
    finally:
        bs.free()
        bf.free()


def _all_127(depth, signs):
    """one shard, every column selected, both fields at 2^depth - 1 (depth a multiple of 7: every chunk byte 127); y = x, -x, or
    x with alternating signs.  -> (Sx, Sy, the moments of the one shard)"""
    v, n = (1 << depth) - 1, 1 << 20
    Sx = np.full((1, depth + 2, 16, 1024), ~np.uint64(0), dtype=np.uint64)
    Sx[0, 1] = 0
    Sy = Sx.copy()
    Sy[0, 1] = {"plus": np.uint64(0), "minus": ~np.uint64(0), "alternating": np.uint64(0xAAAAAAAAAAAAAAAA)}[signs]
    sum_y, sum_xy = {"plus": (n * v, n * v * v), "minus": (-n * v, -n * v * v), "alternating": (0, 0)}[signs]
    return Sx, Sy, M.Moments(n, n * v, sum_y, n * v * v, n * v * v, sum_xy)


@pytest.mark.parametrize("signs", ["plus", "minus", "alternating"])
def test_every_column_at_the_largest_chunk_bytes(gpu_ctx, signs):
    """one shard, all 2^20 columns selected, x = 2^14 - 1 everywhere, y = x, -x, or x with alternating signs: every product is
    +-127^2 and a cell of the shard's matrix is 2^20 x 127^2 > 2^31: a 32-bit sum over the blocks' partial matrices goes wrong.
    (A block sees 2^14 columns of it: the flush inside a block is test_the_flush_inside_a_block's.)"""
    depth = 14
    Sx, Sy, want = _all_127(depth, signs)
    assert M.expected(Sx, depth, Sy, depth, None) == want and want.n * 127 * 127 > 1 << 31
    (bx, rx), (by, ry) = _up(gpu_ctx, Sx), _up(gpu_ctx, Sy)
    try:
        _same(gpu_ctx.bsi_moments(bx, rx, depth, by, ry, depth), want)
    finally:
        bx.free()
        by.free()


@pytest.mark.parametrize("depth,pack", [(14, 4), (35, 2), (56, 1)])
@pytest.mark.parametrize("signs", ["plus", "minus"])
def test_the_flush_inside_a_block(gpu_ctx, depth, pack, signs):
    """8192 shards that all read the ONE all-127 fragment (aliasing base_rows), for each packing: a launch of at most 1024 blocks
    gives a block 8 shards' worth of units or more — at least 2048 / 4096 / 8192 stripes at 4 / 2 / 1 column blocks per tile, far
    beyond the 64 after which the i32 accumulators are flushed.  A wave's cell then reaches stripes x 256 x 127^2 >= 8.4e9 in
    magnitude: past 2^31 without the flush (or with a late one) and past 2^32 were the wave's own sums 32 bits wide."""
    n_sh = 8192
    rows = M.rows_of(depth, depth)[3]
    assert (4 if rows <= 8 else 2 if rows <= 16 else 1) == pack and depth % 7 == 0
    stripes = n_sh * (1024 // pack) // 1024
    assert stripes > 64 and stripes * 256 * 127 * 127 > 1 << 32
    Sx, Sy, one = _all_127(depth, signs)
    want = M.wrapped(M.Moments(*(n_sh * v for v in one)))
    (bx, rx), (by, ry) = _up(gpu_ctx, Sx), _up(gpu_ctx, Sy)
    z = np.zeros(n_sh, dtype=np.uint32)
    try:
        _same(gpu_ctx.bsi_moments(bx, z, depth, by, z, depth), want)
    finally:
        bx.free()
        by.free()


def _upload_bsi(ctx, frags):
    rows, base = [], []
    for fr in frags:
        base.append(len(rows))
        for r, bm in enumerate(fr.rows):
            rows.append({r * 16 + k: D.to_fbk(c) for k, c in bm.items() if c.n} if bm is not None else {})
    return ctx.upload(rows), np.array(base, dtype=np.uint32)


def test_encoded_batches_densify_in_two_chunks(gpu_ctx, oracle, B):
    """64 shards of encoded x, y and filter at depth 64 x 64, few values: 133 rows are densified per shard, at most 61 shards fit
    a chunk, so the call takes two chunks of 32.  Fragments built with optimize() (planes as arrays and runs), the filter rows
    datagen's archetypes."""
    rng = D.rng_for(9500)
    n_sh, depth, n_vals = 64, 64, 120
    assert M.densify_chunk(n_sh, False, depth, False, depth, False) == 32
    lim = (1 << depth) - 1
    frags_x, frags_y, f_rows, xs, ys, xs1 = [], [], [], [], [], []
    for s in range(n_sh):
        cols = rng.choice(1 << 20, size=n_vals, replace=False)
        cols[: n_vals // 3] = (cols[: n_vals // 3] & 0xFFFF) | (5 << 16)  # a third of them in one container
        cols = np.unique(cols).tolist()
        val = lambda: int(rng.integers(0, lim, endpoint=True, dtype=np.uint64)) * (-1 if rng.random() < 0.4 else 1)
        vx = {c: val() for c in cols if rng.random() < 0.8}
        vy = {c: val() for c in cols if rng.random() < 0.8}
        if s == 7:
            vy = {}  # a shard in which y has no values
        row = D.random_row(rng, 0, p_missing=0.2)
        fbits = R.bits(R.words_of_row(row))
        frags_x.append(B.bsi_fragment_from_values(vx, depth))
        frags_y.append(B.bsi_fragment_from_values(vy, depth))
        f_rows.append(row)
        for c in cols:
            if c in vx and fbits[c]:
                xs1.append(vx[c])
                if c in vy:
                    xs.append(vx[c])
                    ys.append(vy[c])
    assert len(xs) > 500
    (bx, rx), (by, ry) = _upload_bsi(gpu_ctx, frags_x), _upload_bsi(gpu_ctx, frags_y)
    bf = gpu_ctx.upload([D.to_fbk_row(r) for r in f_rows])
    rf = np.arange(n_sh, dtype=np.uint32)
    try:
        _same(gpu_ctx.bsi_moments(bx, rx, depth, by, ry, depth, bf, rf), M.brute(xs, ys))
        _same(gpu_ctx.bsi_moments(bx, rx, depth, filt=bf, rows_f=rf), M.brute(xs1, None))
    finally:
        for b in (bx, by, bf):
            b.free()


def test_error_leaves_the_context_usable(gpu_ctx):
    rng = D.rng_for(9600)
    n_sh, dx, dy = 2, 8, 5
    Sx, Sy = _field(rng, n_sh, dx), _field(rng, n_sh, dy)
    (bx, rx), (by, ry) = _up(gpu_ctx, Sx), _up(gpu_ctx, Sy)
    try:
        want = M.expected(Sx, dx, Sy, dy, None)
        _same(gpu_ctx.bsi_moments(bx, rx, dx, by, ry, dy), want)
        bad = rx.copy()
        bad[1] = n_sh * (dx + 2) - 1  # the fragment's rows run past the batch
        for args in ((bx, rx, 65, by, ry, dy), (bx, rx, dx, by, ry, 65), (bx, rx, dx, None, None, 3), (bx, bad, dx, by, ry, dy),
                     (bx, rx, dx, by, ry, dy, by, np.array([0, n_sh * (dy + 2)], dtype=np.uint32))):
            with pytest.raises(L.FbkError) as e:
                gpu_ctx.bsi_moments(*args)
            assert e.value.code == L.FBK_E_INVALID
            _same(gpu_ctx.bsi_moments(bx, rx, dx, by, ry, dy), want)
        out = L.Moments(n=5)
        L.check(gpu_ctx.lib.fbk_bsi_moments(gpu_ctx.h, bx.h, rx.ctypes.data, dx, None, None, 0, None, None, 0, out))  # no shards
        assert bytes(out) == bytes(96)
    finally:
        bx.free()
        by.free()


@pytest.mark.parametrize("depth", [20, 63])
def test_the_models_decode_is_the_oracles(oracle, B, depth):
    """sampled columns: the value the oracle's fragment holds (its BSI Sum over a one-column filter) is the model's decode"""
    rng = D.rng_for(9700, depth)
    S = _field(rng, 1, depth)[0]
    frag = R.fragment_of_words(oracle, B, S)
    cols = [0, 1, 65535, 65536, (1 << 20) - 1] + rng.integers(0, 1 << 20, 40).tolist()
    vals = M.values_at(S, depth, cols)
    assert any(v is None for v in vals) and any(v is not None and v < 0 for v in vals) and any(v is not None and v > 0 for v in vals)
    for c, v in zip(cols, vals):
        s, n = B.bsi_sum(frag, B.row_from_columns([c]), True)
        assert (s, n) == ((v, 1) if v is not None else (0, 0)), c
