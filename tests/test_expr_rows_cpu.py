"""CPU checks of fbk_expr_row_counts / fbk_expr_topk / fbk_expr_topn (no GPU): the generator and the numpy model of
tests/expr_rows_gen.py against each other and against the oracle's intersection counts, the ground the pool covers — asserted, not
promised —, fbk_expr::rows_per_block (compiled into a stand-alone program) against its Python restatement, the resources of
k_expr_rows_vs_filter and k_rows_vs_filter read from the built library's code object, and the presence of the three entry points in
include/fbk.h, lib.SIGNATURES and the library's exports (which fails before they existed)."""
import os
import re
import subprocess

import numpy as np
import pytest

import expr_gen as G
import expr_rows_gen as RG
from test_kernel_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fbk_expr_row_counts", "fbk_expr_topk", "fbk_expr_topn")
# what fbk_expr_topk.hip.h states for its kernel: __launch_bounds__(256, 8), that is at most 64 vector registers, and no scratch
VGPR_BOUND = 64


@pytest.fixture(scope="module")
def worlds(oracle):
    from oracle import pybsi

    pybsi._lib()
    return [RG.World(it) for it in range(6)]


def test_pool_covers_the_ground(worlds):
    from oracle import pyoracle as O

    for w in worlds:
        assert len(w.pool) == RG.POOL and not w.pool[1]
        r0 = w.pool[0]
        assert r0[0].typ == O.ARRAY and r0[0].n > 4096  # more than 8 KiB of payload
        assert r0[1].n == 65536 and 2 not in r0 and r0[3].typ == O.RUN
        enc = {c.typ for r in w.pool for c in r.values()}
        assert enc == {O.ARRAY, O.BITMAP, O.RUN}
        for n_a in RG.N_AS:
            rows = w.field(n_a)
            assert rows.shape == (w.n_shards, n_a) and rows[0, 0] == 0 and rows.max() < RG.POOL
    assert {w.n_shards for w in worlds} == {1, 2, 3}


def test_model_equals_the_oracle_row_by_row(worlds, oracle):
    """counts[s][i] of the model = the sum over the slots of the oracle's intersection_count of the field's container and the
    tree's container at that slot (the tree's row from the model's words)"""
    for w in worlds[:3]:
        tree = w.tree()
        f = w.model(tree)
        rows = w.field(65)
        tot, per, fc = w.model_counts(tree, rows)
        assert fc.tolist() == G.popcount(f).tolist() and tot.tolist() == per.sum(axis=0).tolist()
        for s in range(w.n_shards):
            filt = [oracle.OContainer.bitmap(f[s][k]) for k in range(16)]
            for i in (0, 1, 31, 64):
                row = w.pool[int(rows[s, i])]
                exp = sum(oracle.intersection_count(c, filt[k & 15]) for k, c in row.items() if c.n and filt[k & 15].n)
                assert int(per[s, i]) == exp, (w.it, s, i)
    # ordering of the totals: count descending, index ascending, zeros dropped
    assert RG.top_of(np.asarray([3, 0, 9, 3, 9], dtype=np.uint64), 0) == ([2, 4, 0, 3], [9, 9, 3, 3])
    assert RG.top_of(np.asarray([3, 0, 9, 3, 9], dtype=np.uint64), 3) == ([2, 4, 0], [9, 9, 3])


def test_rows_per_block_equals_its_restatement():
    exe = RG.build_rows_checker(os.path.join(ROOT, "build", "expr_rows_check_san"))
    grid = [(a, s, l) for a in (1, 2, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 1000, 4096, 4097, 65536, 1 << 22)
            for s in (1, 2, 3, 7, 8, 16, 96, 127, 128, 129, 1024, 1 << 26) for l in (0, 1, 2, 3, 17, 64, 65, 66, 130, 200, 1024)]
    got = RG.run_rows_checker(exe, grid)
    assert got == [RG.rows_per_block(*g) for g in grid]
    for (a, s, l), rpb in zip(grid, got):
        chunks = (a + rpb - 1) // rpb
        assert rpb % 64 == 0 and rpb >= 64 and (chunks - 1) * rpb < a
        assert chunks == 1 or (chunks - 1) * l <= a, (a, s, l)  # re-evaluating the tree at most doubles the reads
    # the cases tests/test_gpu_expr_rows.py relies on
    for s in (1, 2, 3):
        assert RG.chunks_of(200, s, 3) == (4, 8)
    assert RG.chunks_of(65, 1, 66) == (1, 65) and RG.rows_per_block(65, 1, 66) == 128 and RG.chunks_of(65, 1, 3) == (2, 1)
    # (L = 0 is what the one launch of k_rows_vs_filter passes, launch_rows_vs_filter: no second copy of the rule is left to compare)


def test_kernel_resources_from_the_code_object():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    meta = {k[0]: k for k in kernel_metadata(L.LIB_PATH)}
    new = [k for n, k in meta.items() if n.startswith("_ZN3fbk21k_expr_rows_vs_filterE")]
    old = [k for n, k in meta.items() if n.startswith("_ZN3fbk16k_rows_vs_filterE")]
    assert len(new) == 1 and len(old) == 1
    for _, scratch, vspill, sspill, vgpr in new + old:
        assert scratch == 0 and vspill == 0 and sspill == 0
    assert new[0][4] <= VGPR_BOUND, new[0]
    assert old[0][4] <= 64, old[0]


def test_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbk.h")).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in NAMES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES, name
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    from featurebase_amd.roaring import Context

    for name in ("expr_row_counts", "expr_topk", "expr_topn"):
        assert callable(getattr(Context, name))
