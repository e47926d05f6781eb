"""Structural fuzz of fbk_topn / fbk_topk / fbk_query_topn / fbk_topn_partials / fbk_group_topn / fbk_topk_bsi on fields of thousands
of rows (tests/fuzz_topn_gen.py makes the cases and their expectations, tests/test_fuzz_topn_cpu.py checks them without a GPU): the
sizes at which k_topn_candidates takes more than one trip of its strided loops and its index key leaves level-0 bin 0, the default
host / device ordering switch at 4096 / 4097 rows, k_rows_vs_filter in several chunks a shard, and k_counts_to_bsi beyond slot 0.
Everything is integers: every form must return the model's (indexes, counts) exactly.  FBK_FUZZ_ITERS=<n> runs more iterations,
FBK_TEST_SEED re-rolls them."""
import numpy as np
import pytest

import datagen as D
import fuzz_topn_gen as G
from featurebase_amd import dist as fd
from featurebase_amd import lib as L
from featurebase_amd.roaring import Group

pytestmark = pytest.mark.gpu


def pairs(idx, cnt):
    return [int(i) for i in idx], [int(c) for c in cnt]


@pytest.mark.parametrize("it", range(G.ITERS))
def test_fuzz_topn_large_fields(gpu_ctx, it):
    """Every parameter set of both fields of the case under both topn_semantics through the one-shot call, a prepared query run and
    read twice, the partials of two dealings of the shards reduced as featurebase_amd.dist.topn_reduce does, two groups (one with a
    member that holds no shard) and, without thresholds, fbk_topk."""
    case = G.Case(it)
    ctx, rf = gpu_ctx, case.rf
    pool_rows, filter_rows = case.pool.upload_rows(), G.filter_upload_rows(case.filter_words)
    A, F = ctx.upload(pool_rows), ctx.upload(filter_rows)
    groups = [Group([0, 0]), Group([0, 0, 0])]
    keep = [A, F]
    members = []  # per group, per member: None or (pool batch, filter batch, shards)
    saved = {}
    try:
        for grp, dealing in zip(groups, case.group_dealings):
            grp.set_reduce(L.REDUCE_HOST)
            per = []
            for c, shards in zip(grp.members, dealing):
                if not shards:
                    per.append(None)
                    continue
                a, f = c.upload(pool_rows), c.upload(filter_rows)
                keep += [a, f]
                per.append((a, f, shards))
            members.append(per)
        every = [ctx] + [c for grp in groups for c in grp.members]
        saved.update({name: ctx.get_option(name) for name in list(case.options) + ["topn_semantics"]})
        for name, val in case.options.items():
            for c in every:
                c.set_option(name, val)
        for fld in case.fields:
            ra, n_a = fld.ra, fld.n_a
            for si, (n, mt, tt, hf) in enumerate(fld.sets):
                fa = (F, rf) if hf else (None, None)
                kw = dict(min_threshold=mt, tanimoto_threshold=tt)
                for sem in (1, 0):
                    where = (case, n_a, si, fld.why[si], fld.sets[si], sem)
                    exp = fld.expect[(si, sem)]
                    for c in every:
                        c.set_option("topn_semantics", sem)
                    assert pairs(*ctx.topn(A, ra, n, *fa, **kw)) == exp, ("topn", where)
                    q = ctx.prepare_topn(A, ra, n, *fa, **kw)
                    try:
                        for run in range(2):  # the second run must not see the first run's candidate flags
                            q.run()
                            assert pairs(*q.read()) == exp, ("prepared", run, where)
                            assert pairs(*q.read()) == exp, ("prepared, read again", run, where)
                    finally:
                        q.free()
                    for dealing in case.dealings:
                        tot, cand = np.zeros(n_a, dtype=np.uint64), np.zeros(n_a, dtype=np.uint64)
                        for shards in dealing:
                            t, c = ctx.topn_partials(A, ra[shards], n_a, n, *((F, rf[shards]) if hf else (None, None)), **kw)
                            et, ec = fld.members_expect(si, sem, shards)
                            assert np.array_equal(t, et), ("partial totals", shards, where)
                            assert np.array_equal(c != 0, ec), ("partial candidates", shards, where)
                            tot, cand = tot + t, cand + c
                        assert pairs(*fd.topn_reduce(tot, cand, n)) == exp, ("partials reduced", dealing, where)
                    for grp, per in zip(groups, members):
                        args = [None if m is None else dict(a=m[0], rows_a=ra[m[2]], filt=m[1] if hf else None, rows_f=rf[m[2]] if hf else None) for m in per]
                        assert pairs(*grp.topn(args, n_a, n, mt, tt)) == exp, ("group of %d" % len(per), where)
                    if sem == 0 and mt == 0 and tt == 0:
                        assert pairs(*ctx.topk(A, ra, n, *fa)) == exp, ("topk", where)
    finally:
        for name, val in saved.items():  # (the groups' members go with their groups)
            ctx.set_option(name, val)
        for b in keep:
            b.free()
        for grp in groups:
            grp.close()


def _decode(batch, depth):
    """the planes of a TopK-BSI result as [depth, 16, 1024] words: output row p holds plane p and nothing else"""
    rows = batch.download()
    assert len(rows) == depth
    W = np.zeros((depth, 16, 1024), dtype=np.uint64)
    for p, row in enumerate(rows):
        for k, c in row.items():
            assert k >> 4 == p, (p, k)
            w = c.words()
            assert c.n == int(np.bitwise_count(w).sum()) and c.n > 0, (p, k)
            W[p, k & 15] = w
    return W


@pytest.mark.parametrize("n_a", G.BSI_SIZES)
def test_fuzz_topk_bsi_wide_fields(gpu_ctx, n_a):
    """fbk_topk_bsi on 2^16 .. 2^20 rows: the decoded planes equal the totals for every row, nothing beyond n_a (the expected words are
    zero there), with and without optimize(); two shard sets of unequal depth merged by fbk_bsi_add; for the 131 077-row field the
    device ordering of TopK / TopN among many equal totals."""
    case = G.BsiCase(n_a)
    ctx, rf, ra = gpu_ctx, case.rf, case.ra
    A, F = ctx.upload(case.pool.upload_rows()), ctx.upload(G.filter_upload_rows(case.filter_words))
    keep = [A, F]
    semantics = ctx.get_option("topn_semantics")
    try:
        exp_depth = int(case.tot.max()).bit_length()
        for flags in (0, L.SETOP_OPTIMIZE):
            out, depth = ctx.topk_bsi(A, ra, F, rf, flags)
            keep.append(out)
            assert depth == exp_depth, (case, flags)
            W = _decode(out, depth)
            assert np.array_equal(G.decode_planes(W)[:n_a], case.tot), (case, flags)
            assert np.array_equal(W, case.planes), (case, flags, "a bit at a row id >= n_a")
        x, y = case.split
        ox, dx = ctx.topk_bsi(A, ra[x], F, rf[x])
        oy, dy = ctx.topk_bsi(A, ra[y], F, rf[y])
        keep += [ox, oy]
        assert dx == int(case.shard_tot[x].sum(axis=0).max()).bit_length() and dy == int(case.shard_tot[y].sum(axis=0).max()).bit_length() and dx != dy, (case, dx, dy)
        s = ctx.bsi_add(ox, np.arange(dx).reshape(1, -1), oy, np.arange(dy).reshape(1, -1))
        keep.append(s)
        W = _decode(s, max(dx, dy) + 1)  # (one plane more than the deeper operand: the carry)
        assert np.array_equal(G.decode_planes(W)[:n_a], case.tot) and not G.decode_planes(W)[n_a:].any(), case
        if n_a == 131077:  # the device ordering among many equal totals: with the filter and without it
            for fa, tot in (((F, rf), case.tot), ((None, None), case.pool.card[ra].sum(axis=0))):
                top = G.top_of(tot, 10)
                assert pairs(*ctx.topk(A, ra, 10, *fa)) == top, case
                ctx.set_option("topn_semantics", 0)
                assert pairs(*ctx.topn(A, ra, 10, *fa)) == top, case
            ctx.set_option("topn_semantics", 1)
            assert pairs(*ctx.topn(A, ra, 10, F, rf)) == case.topn_expect(10, 1), case
    finally:
        ctx.set_option("topn_semantics", semantics)
        for b in keep:
            b.free()


def test_topn_row_limits(gpu_ctx):
    """fbk_topn and fbk_topk take fields of up to 2^22 rows, fbk_topk_bsi of up to 2^20: one row more is FBK_E_INVALID, whatever the
    row list holds, and the context answers the next call."""
    ctx = gpu_ctx
    rows = [{0: D.fbk_container_of_vals(np.arange(k + 1, dtype=np.int64) * 3)} for k in range(3)]
    A = ctx.upload(rows)
    try:
        for n_a, calls in (((1 << 22) + 1, (lambda ra: ctx.topn(A, ra, 3), lambda ra: ctx.topk(A, ra, 3))), ((1 << 20) + 1, (lambda ra: ctx.topk_bsi(A, ra),))):
            ra = (np.arange(n_a, dtype=np.uint32) % 3).reshape(1, n_a)
            for call in calls:
                with pytest.raises(L.FbkError) as e:
                    call(ra)
                assert e.value.code == L.FBK_E_INVALID, (n_a, str(e.value))
                idx, cnt = ctx.topk(A, np.arange(3).reshape(1, 3), 0)
                assert pairs(idx, cnt) == ([2, 1, 0], [3, 2, 1])
    finally:
        A.free()
