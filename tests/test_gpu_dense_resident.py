"""The dense count of a hot plan (k_icount_dense_resident): a plan whose rows fit the Infinity Cache, counted again with
nothing else enqueued on its context in between, takes a persistent grid of one block per compute unit that walks the pairs
in alternating directions.  Which kernel a launch takes changes nothing a caller can see: every launch of every plan below —
the cold first one, the hot ones in both directions, the ones after a disturbing call — must give numpy's counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -0x1111111111111112  # 0xEEEE...EE as int64: no count of a 2^20-bit row pair looks like it
LAUNCHES = 5  # cold, then hot: reversed, forward, reversed, forward


@pytest.fixture(scope="module")
def rows8():
    """8 dense rows (1 MiB) with seeded bits, an all-ones and an all-zero row among them, and the 8 x 8 table of |a & b|."""
    rng = np.random.default_rng(20261018)
    w = rng.integers(0, 2**64, size=(8, 16, 1024), dtype=np.uint64)
    w[2] &= rng.integers(0, 2**64, size=(16, 1024), dtype=np.uint64)  # a sparser row
    w[5] = ~np.uint64(0)
    w[6] = 0
    table = np.array([[int(np.bitwise_count(w[i] & w[j]).sum()) for j in range(8)] for i in range(8)], dtype=np.uint64)
    w.setflags(write=False)
    table.setflags(write=False)
    return w, table


@pytest.fixture(scope="module")
def batch8(gpu_ctx, rows8):
    b = gpu_ctx.upload_dense(rows8[0])
    yield b
    b.free()


def _grid():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count  # the resident kernel's grid: one block per compute unit


def _row_lists(n_pairs, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 8, size=n_pairs), rng.integers(0, 8, size=n_pairs)


class _Cells:
    """A caller-owned counts buffer and a cell for the total, refilled before every launch."""

    def __init__(self, n_pairs):
        import torch

        self.torch = torch
        self.counts = torch.empty(n_pairs, dtype=torch.int64, device="cuda:0")
        self.cell = torch.empty(1, dtype=torch.int64, device="cuda:0")

    def refill(self):
        self.counts.fill_(SENTINEL)
        self.cell.zero_()
        self.torch.cuda.synchronize()  # (the context launches on a stream of its own)

    def read(self, ctx):
        ctx.synchronize()  # a quiet call: the plan stays hot
        return self.counts.cpu().numpy().view(np.uint64), int(self.cell.cpu().numpy().view(np.uint64)[0])


def _launch(plan, cells, form):
    if form == "plain":
        plan.intersection_count()
    elif form == "total":
        plan.intersection_count_total(cells.cell.data_ptr())
    else:
        plan.intersection_count_accumulate(cells.cell.data_ptr())


def _check(got, cell, want, form, what):
    assert not (got == np.uint64(SENTINEL & (2**64 - 1))).any(), f"{what}: pairs never written {np.flatnonzero(got == np.uint64(SENTINEL & (2**64 - 1)))[:8]}"
    assert (got == want).all(), f"{what}: pairs {np.flatnonzero(got != want)[:8]} differ"
    if form != "plain":
        # the cell was zeroed before the launch: a pair counted twice, or never, shows here even where out[] is right
        assert cell == int(want.sum()), f"{what}: total {cell}, numpy {int(want.sum())}"


def _five_launches(ctx, batch, table, n_pairs, form, seed, between=None):
    ra, rb = _row_lists(n_pairs, seed)
    want = table[ra, rb]
    cells = _Cells(n_pairs)
    plan = ctx.plan(batch, ra, batch, rb, device_counts_ptr=cells.counts.data_ptr())
    try:
        for k in range(LAUNCHES):
            if between is not None and k == 3:
                between(plan)
            cells.refill()
            _launch(plan, cells, form)
            got, cell = cells.read(ctx)
            _check(got, cell, want, form, f"n_pairs {n_pairs}, {form}, launch {k}")
    finally:
        plan.free()


@pytest.mark.parametrize("which", ["1", "2", "3", "G-1", "G", "G+1", "2G+3"])
def test_stride_and_mirror_map(gpu_ctx, rows8, batch8, which):
    """The block stride, its remainder and the reversed walk: n_pairs around the grid size G, five launches in a row."""
    g = _grid()
    n_pairs = {"1": 1, "2": 2, "3": 3, "G-1": g - 1, "G": g, "G+1": g + 1, "2G+3": 2 * g + 3}[which]
    _five_launches(gpu_ctx, batch8, rows8[1], n_pairs, "accumulate", seed=n_pairs)


@pytest.mark.parametrize("form", ["plain", "total", "accumulate"])
def test_all_three_result_forms(gpu_ctx, rows8, batch8, form):
    _five_launches(gpu_ctx, batch8, rows8[1], _grid() + 1, form, seed=77)


@pytest.mark.parametrize("disturb", ["one_shot_count", "plan_setop"])
def test_disturbing_call_in_the_middle(gpu_ctx, rows8, batch8, disturb):
    """Another call on the context between launches 3 and 4: the plan goes back to the cold kernel, then hot again."""
    table = rows8[1]

    def between(plan):
        if disturb == "one_shot_count":
            got = gpu_ctx.intersection_count(batch8, [0, 1, 5], batch8, [3, 4, 6])
            assert (got == table[[0, 1, 5], [3, 4, 6]]).all()
        else:
            from featurebase_amd import lib as L

            plan.setop(L.OP_AND)

    for form in ("total", "accumulate"):
        _five_launches(gpu_ctx, batch8, table, _grid() + 1, form, seed=78, between=between)


@pytest.mark.parametrize("spb", [1, 4])
def test_other_dense_spb_values(gpu_ctx, rows8, batch8, spb):
    """dense_spb != 16 never takes the resident kernel, but its blocks end in the tail function the two kernels share."""
    gpu_ctx.set_option("dense_spb", spb)
    try:
        for form in ("plain", "total", "accumulate"):
            _five_launches(gpu_ctx, batch8, rows8[1], _grid() + 1, form, seed=79)
    finally:
        gpu_ctx.set_option("dense_spb", 16)


def test_plan_over_the_threshold(gpu_ctx, rows8):
    """Two batches of 1032 rows each: the plan's footprint bound is 258 MiB, over the 256 MiB threshold, so every launch takes
    the cold kernel (the bound itself: tests/test_dense_footprint_cpu.py).  The rows are the 8 seeded ones, repeated."""
    w, table = rows8
    reps = 129
    big = np.ascontiguousarray(np.tile(w, (reps, 1, 1)))
    A, B = gpu_ctx.upload_dense(big), gpu_ctx.upload_dense(big[::-1].copy())
    try:
        n = 8 * reps
        ra, rb = np.arange(n), np.arange(n)
        want = table[ra % 8, (n - 1 - rb) % 8]
        cells = _Cells(n)
        plan = gpu_ctx.plan(A, ra, B, rb, device_counts_ptr=cells.counts.data_ptr())
        try:
            for k in range(3):
                cells.refill()
                plan.intersection_count_accumulate(cells.cell.data_ptr())
                got, cell = cells.read(gpu_ctx)
                _check(got, cell, want, "accumulate", f"over the threshold, launch {k}")
        finally:
            plan.free()
    finally:
        A.free()
        B.free()
