"""The five ways to a TopN share one pass body, one sizing rule and one ordering (fbk_topn_api.inc, fbk_topn_plan.h): on the same data
they must agree with each other and with the numpy model.  Three shards of expr_rows_gen.World(2), a field of 5, 65 and 200 rows;
option matrix_pass_kb = 1 (fields of 65 and more rows: one shard per pass, three passes) and 2^20 (one pass), both topn_semantics,
(n, MinThreshold, Tanimoto) with and without thresholds and a candidate pass; as the source no row, a filter row per shard, and
the call tree that is that single row leaf.  Compared: fbk_topn, fbk_topn_partials ordered on the host, fbk_query_topn run twice then
read, fbk_group_topn of a one-member group, fbk_expr_topn over the single-leaf tree — against fuzz_prepared_gen.topn_model (the rules
of fuzz_topn_gen's expectations) on the model's counts."""
import numpy as np
import pytest

import expr_rows_gen as RG
import test_gpu_expr_rows as TR
from featurebase_amd.roaring import Group
from fuzz_prepared_gen import topn_model

pytestmark = pytest.mark.gpu

PARAMS = ((0, 0, 0), (3, 0, 0), (3, 2, 0), (3, 0, 30), (3, 2, 30))


@pytest.fixture(scope="module")
def world(oracle):
    from oracle import pybsi

    pybsi._lib()
    w = RG.World(2)
    assert w.n_shards == 3
    grp = Group([0])  # (its member is the context of every path: the batches of a group call live on the member)
    env = TR.Env(grp.members[0], w)
    yield env, grp
    env.free()
    grp.close()


def pair(t):
    return t[0].tolist(), [int(c) for c in t[1]]


@pytest.mark.parametrize("n_a", [5, 65, 200])
def test_five_paths_agree(world, n_a):
    env, grp = world
    w, ctx, F = env.w, env.ctx, env.batches["F"]
    lf = w.a[1]  # the source: row lf.rows[s] of batch lf.batch in shard s
    filt, rows_f = env.batches[lf.batch], np.asarray(lf.rows, dtype=np.uint32)
    rows = w.field(n_a)
    cnt = RG.popc(w.pool_words)[rows]  # [n_shards, n_a] cardinalities
    _, per, fc = w.model_counts(lf, rows)
    assert per.any() and (per != cnt).any() and fc.all()
    no_src = np.zeros(w.n_shards, dtype=np.uint64)
    try:
        for kb in (1, 1 << 20):
            ctx.set_option("matrix_pass_kb", kb)
            for sem in (0, 1):
                ctx.set_option("topn_semantics", sem)
                for n, mt, tt in PARAMS:
                    for source in ("none", "row"):
                        f, rf = (filt, rows_f) if source == "row" else (None, None)
                        exp = topn_model(cnt, per, fc, True, n, mt, tt, sem) if f is not None else topn_model(cnt, cnt, no_src, False, n, mt, tt, sem)
                        tag = (n_a, kb, sem, n, mt, tt, source)
                        assert pair(ctx.topn(F, rows, n, f, rf, mt, tt)) == exp, tag
                        tot, cand = ctx.topn_partials(F, rows, n_a, n, f, rf, mt, tt)
                        assert RG.top_of(np.where(cand != 0, tot, np.uint64(0)), n) == exp, tag
                        q = ctx.prepare_topn(F, rows, n, f, rf, mt, tt)
                        try:
                            q.run()
                            q.run()
                            assert pair(q.read()) == exp, tag
                        finally:
                            q.free()
                        assert pair(grp.topn([dict(a=F, rows_a=rows, filt=f, rows_f=rf)], n_a, n, mt, tt)) == exp, tag
                        if f is not None:  # the tree that is that single row leaf
                            assert pair(ctx.expr_topn([env.leaf(lf)], TR.PUSH0, F, rows, n, mt, tt)) == exp, tag + ("tree",)
    finally:
        ctx.set_option("matrix_pass_kb", 1 << 20)
        ctx.set_option("topn_semantics", 1)
