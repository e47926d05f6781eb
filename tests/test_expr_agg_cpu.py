"""CPU checks of fbk_expr_bsi_agg / fbk_query_expr_bsi (no GPU): the numpy model of tests/expr_agg_gen.py (Sum, Min and Max over
model_tree & exists) against the oracle's fragment.sum / min / max transcriptions applied to the materialised filter, the ground the
default iterations cover — asserted, not promised —, and the presence of the two entry points in include/fbk.h and lib.SIGNATURES
(which fails before they existed)."""
import os
import re

import numpy as np
import pytest

import expr_agg_gen as A
import expr_gen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(oracle):
    from oracle import pybsi

    pybsi._lib()
    out = []
    for it in range(G.ITERS):
        w = A.World(it)
        t = w.tree()
        out.append((w, t, w.model(t)))
    return out


def test_model_equals_the_oracle_on_the_materialised_filter(cases, oracle):
    from oracle import pybsi

    for w, t, filt in cases:
        for name in ("W", "V"):
            f = w.fields[name]
            got = {agg: f.aggregate(agg, filt) for agg in A.AGGS}
            for s in range(w.n_shards):
                bm = A.bitmap_of_words(filt[s])
                if bm is None:
                    bm = oracle.OBitmap()
                exp = {A.SUM: pybsi.bsi_sum(f.frags[s], bm, True), A.MIN: pybsi.bsi_min(f.frags[s], bm, f.depth), A.MAX: pybsi.bsi_max(f.frags[s], bm, f.depth)}
                for agg in A.AGGS:
                    assert (got[agg][0][s], got[agg][1][s]) == exp[agg], (w.it, name, s, agg, t)


def test_worlds_and_trees_cover_the_ground(cases, tmp_path):
    checker = G.build_checker(os.path.join(ROOT, "build", "expr_plan_check_san"))
    out = G.run_checker(checker, [G.postfix(t) for _, t, _ in cases], str(tmp_path / "corpus.txt"))
    depths, fields, signs = set(), set(), set()
    saved = bsi_last = empty_filter = nil_under_filter = full_exists = wraps = False
    for (w, t, filt), line in zip(cases, out):
        assert line[0] == "OK"
        f = w.fields[w.agg_field]
        fields.add(w.agg_field)
        depths.add(f.depth)
        leaves = G.postfix(t)[0]
        slots, ins = int(line[2]), [int(x) for x in line[5:]]
        saved |= slots > 0
        last = ins[-1]
        # the last lowered instruction reads a plane of a predicate, or is a register move only a predicate's scan emits
        bsi_last |= (leaves[(last >> 12) & 0xFFF].kind != G.ROW) if (last >> 24) <= G.I_MOR_XAN else (last >> 24) in (G.I_MZERO, G.I_X_FROM_M, G.I_ZERO_X)
        empty_filter |= not filt.any()
        ex = w.exists_words("W")
        assert not ex[:, A.NIL_SLOT].any() and (ex[0, A.FULL_SLOT] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        nil_under_filter |= bool(filt[:, A.NIL_SLOT].any())
        full_exists |= bool(filt[0, A.FULL_SLOT].any())
        for s, (cols, mag, neg) in enumerate(w.fields["W"].data):
            nz = mag != 0
            if nz.any():
                signs.add("negative" if neg[nz].all() else "positive" if not neg.any() else "mixed")
            wraps |= sum(int(x) for x in mag) >= 1 << 64
        enc = {c.typ for fr in w.fields["W"].frags for bm in fr.rows if bm is not None for _, c in bm.items()}
        if w.wdepth >= 5:
            assert len(enc) == 3, (w.it, enc)  # array, bitmap and run containers among W's rows
    assert {0, 64} <= depths, depths
    assert fields == {"V", "W"}
    assert signs == {"negative", "positive", "mixed"}
    assert saved and bsi_last and empty_filter and nil_under_filter and full_exists and wraps
    assert set(A.AGGS) == {0, 1, 2}  # every iteration runs all three on its field (test_gpu_expr_agg.py)


def test_entry_points_are_declared_and_bound():
    from featurebase_amd import lib as L

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fbk.h")).read(), flags=re.S)
    for name in ("fbk_expr_bsi_agg", "fbk_query_expr_bsi"):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES, name
    assert (L.AGG_SUM, L.AGG_MIN, L.AGG_MAX) == (0, 1, 2)
    for d, v in (("FBK_AGG_SUM", 0), ("FBK_AGG_MIN", 1), ("FBK_AGG_MAX", 2)):
        assert re.search(r"#define %s %du\b" % (d, v), hdr), d
