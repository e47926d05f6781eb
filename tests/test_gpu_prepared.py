"""Prepared queries (fbk_query_*): the launch-only forms of the count matrix, the n-way fold with its fused count
and BSI Sum / one-pass Sum(Range).  Every result is compared with the CPU oracle (oracle/batch_oracle.c over the
same flattened rows: groupByIterator executor.go:8880, Bitmap.Union roaring.go:1272 + IntersectionCount :711,
fragment.sum fragment.go:724, rangeOp :937) and with the one-shot call; repeated runs, caller-owned device
buffers and the accumulate flag included."""
import numpy as np
import pytest

import datagen as D
from featurebase_amd import lib as L
from oracle import pybatch as PB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed():
    rows, groups, filt = D.config3_flat(12, 16, seed_idx=8100, workers=1)
    return rows, groups, filt, PB.RowSet.from_flat(rows.descs(), rows.payload(), rows.n_rows), PB.RowSet.from_flat(filt.descs(), filt.payload(), filt.n_rows)


def test_prepared_count_matrix_mixed_and_dense(gpu_ctx, mixed):
    import torch

    rows, g, filt, OA, OF = mixed
    n = g.shape[0]
    batch = gpu_ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows)
    F = gpu_ctx.upload_flat(filt.descs(), filt.payload(), filt.n_rows)
    fidx = np.arange(n)
    for ra, rb, f in ((g[:, :8], g[:, 8:], True), (g[:, :12], g[:, 12:], False), (g, fidx.reshape(-1, 1), None)):
        if f is None:  # TopK shape: rows x the filter row as B
            exp = PB.topk_counts(OA, ra, OF, fidx)[:, :, None]
            q = gpu_ctx.prepare_count_matrix(batch, ra, F, rb, keep_per_shard=True)
        else:
            exp = PB.count_matrix(OA, ra, OA, rb, OF if f else None, fidx if f else None)
            q = gpu_ctx.prepare_count_matrix(batch, ra, batch, rb, F if f else None, fidx if f else None, keep_per_shard=True)
        for _ in range(3):  # every run overwrites
            q.run()
        tot, ps = q.read(per_shard=True)
        assert (ps == exp).all() and (tot == exp.sum(axis=0)).all()
        # a caller-owned device buffer, accumulated into twice on top of a known value
        cell = torch.full((exp.shape[1] * exp.shape[2],), 5, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        q.run(cell.data_ptr(), accumulate=True)
        q.run(cell.data_ptr(), accumulate=True)
        gpu_ctx.synchronize()
        assert (cell.cpu().numpy().view(np.uint64).reshape(exp.shape[1:]) == 2 * exp.sum(axis=0) + 5).all()
        q.run(cell.data_ptr())  # without the flag: overwritten
        gpu_ctx.synchronize()
        assert (cell.cpu().numpy().view(np.uint64).reshape(exp.shape[1:]) == exp.sum(axis=0)).all()
        q.free()
    # dense rows: the matrix-core kernel
    wa, wb, wf = D.dense_rows(4 * 33, 0.5, 8201), D.dense_rows(4 * 40, 0.5, 8202), D.dense_rows(4, 0.5, 8203)
    A, B, Ff = gpu_ctx.upload_dense(wa), gpu_ctx.upload_dense(wb), gpu_ctx.upload_dense(wf)
    ra, rb = np.arange(4 * 33).reshape(4, 33), np.arange(4 * 40).reshape(4, 40)
    exp = PB.count_matrix(PB.RowSet.from_dense(wa), ra, PB.RowSet.from_dense(wb), rb, PB.RowSet.from_dense(wf), np.arange(4))
    q = gpu_ctx.prepare_count_matrix(A, ra, B, rb, Ff, np.arange(4))
    q.run()
    assert (q.read() == exp.sum(axis=0)).all()
    assert (gpu_ctx.count_matrix(A, ra, B, rb, Ff, np.arange(4)) == exp.sum(axis=0)).all()
    q.free()
    for b in (A, B, Ff, batch, F):
        b.free()


def test_prepared_fold_intersection_count(gpu_ctx, mixed):
    rows, g, filt, OA, OF = mixed
    n = g.shape[0]
    batch = gpu_ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows)
    F = gpu_ctx.upload_flat(filt.descs(), filt.payload(), filt.n_rows)
    fidx = np.arange(n)
    exp, exp_u = PB.union_n_intersection_count(OA, g, OF, fidx)
    q = gpu_ctx.prepare_fold_intersection_count(L.OP_OR, batch, g, F, fidx)
    q.run()
    q.run()
    assert (q.read() == exp).all()
    q.run(accumulate=True)
    assert (q.read() == 2 * exp).all()
    q.free()
    q = gpu_ctx.prepare_fold_intersection_count(L.OP_OR, batch, g)  # no filter: |∪ rows|
    q.run()
    assert (q.read() == exp_u).all()
    q.free()
    # Intersect of the four densest rows of each shard
    gi = g[:, :4]
    R, _ = PB.setop(PB.OP_AND, OA, gi[:, 0], OA, gi[:, 1])
    for k in (2, 3):
        R, cnt = PB.setop(PB.OP_AND, R, np.arange(n), OA, gi[:, k])
    q = gpu_ctx.prepare_fold_intersection_count(L.OP_AND, batch, gi)
    q.run()
    assert (q.read() == cnt).all()
    q.free()
    batch.free()
    F.free()


def test_prepared_bsi_sum_and_one_pass_range_sum(gpu_ctx):
    n_shards, depth = 7, 20
    rng = D.rng_for(8301)
    w = rng.integers(0, 2**64, (n_shards, depth + 2, 16, 1024), dtype=np.uint64)
    w[:, 0] |= rng.integers(0, 2**64, (n_shards, 16, 1024), dtype=np.uint64)
    w[-1, 0, 11:] = 0
    w[:, 1:] &= w[:, :1]
    wf = rng.integers(0, 2**64, (n_shards, 16, 1024), dtype=np.uint64)
    batch, F = gpu_ctx.upload_dense(w.reshape(-1)), gpu_ctx.upload_dense(wf)
    OA, OF = PB.RowSet.from_dense(w.reshape(-1, 16, 1024)), PB.RowSet.from_dense(wf)
    base, idx = np.arange(n_shards) * (depth + 2), np.arange(n_shards)
    for filt in (False, True):
        es, ec = PB.bsi_sum(OA, base, depth, OF if filt else None, idx if filt else None)
        q = gpu_ctx.prepare_bsi_sum(batch, base, depth, filt=F if filt else None, rows_f=idx if filt else None)
        q.run()
        q.run()
        s, c = q.read()
        assert (s == es).all() and (c == ec).all()
        q.free()
    for op, pred in ((L.BSI_GT, 1234), (L.BSI_LTE, -777), (L.BSI_LT, 1 << 19), (L.BSI_GTE, -(1 << 18))):
        R, _ = PB.bsi_range(OA, base, depth, op, pred)
        for filt in (False, True):
            if filt:
                RF, _ = PB.setop(PB.OP_AND, R, idx, OF, idx)
            es, ec = PB.bsi_sum(OA, base, depth, RF if filt else R, idx)
            q = gpu_ctx.prepare_bsi_sum(batch, base, depth, op, pred, F if filt else None, idx if filt else None)
            q.run()
            s, c = q.read()
            assert (s == es).all() and (c == ec).all(), (op, pred, filt)
            q.free()
    # a predicate only the two-pass form serves is refused at prepare time, with a message on the context
    with pytest.raises(L.FbkError):
        gpu_ctx.prepare_bsi_sum(batch, base, depth, L.BSI_EQ, 5)
    assert "one-pass" in gpu_ctx.last_error()[1]
    batch.free()
    F.free()


def test_prepared_query_argument_errors(gpu_ctx, mixed):
    rows, g, filt, OA, OF = mixed
    batch = gpu_ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows)
    with pytest.raises(L.FbkError):
        gpu_ctx.prepare_count_matrix(batch, g[:, :4] + 100000, batch, g[:, 4:8])  # row index out of range
    q = gpu_ctx.prepare_count_matrix(batch, g[:, :4], batch, g[:, 4:8])
    with pytest.raises(L.FbkError):
        q.read()  # before the first run
    other = gpu_ctx.fork()
    with pytest.raises(L.FbkError):
        L.check(other.lib.fbk_query_run(other.h, q.h, None, 0))  # prepared on another context
    other.close()
    q.free()
    batch.free()


def _words_of(batch):
    """bit content of every row of a batch: [n_rows, 16, 1024] uint64"""
    rows = batch.download()
    w = np.zeros((len(rows), 16, 1024), dtype=np.uint64)
    for r, row in enumerate(rows):
        for k, c in row.items():
            w[r, k & 15] = c.words()
    return w


def test_prepared_bsi_range_rows_stay_on_the_device(gpu_ctx):
    """fbk_query_bsi_range: Row(v op k) as a launch-only query whose result rows feed the next operator without leaving the
    device — Range(> k) then Sum(filter = that row), BASELINE config 5's pipeline, both prepared."""
    n_shards, depth = 6, 20
    rng = D.rng_for(8401)
    w = rng.integers(0, 2**64, (n_shards, depth + 2, 16, 1024), dtype=np.uint64)
    w[:, 0] |= rng.integers(0, 2**64, (n_shards, 16, 1024), dtype=np.uint64)
    w[-1, 0, 9:] = 0
    w[:, 1:] &= w[:, :1]
    batch = gpu_ctx.upload_dense(w.reshape(-1))
    OA = PB.RowSet.from_dense(w.reshape(-1, 16, 1024))
    base, idx = np.arange(n_shards) * (depth + 2), np.arange(n_shards)
    for op, pred in ((L.BSI_GT, 4321), (L.BSI_LTE, -99), (L.BSI_EQ, 77), (L.BSI_NEQ, 0), (L.BSI_LT, -(1 << 30)), (L.BSI_GTE, 0)):
        R, ecnt = PB.bsi_range(OA, base, depth, op, pred)
        q = gpu_ctx.prepare_bsi_range(batch, base, op, depth, pred)
        with pytest.raises(L.FbkError):
            q.output()  # no run yet
        for _ in range(2):  # every run rewrites the same output batch
            q.run()
        assert (q.read() == ecnt).all(), (op, pred)
        out = q.output()
        assert (_words_of(out) == R.words()).all(), (op, pred)
        # the borrowed rows as the filter of a prepared Sum and of the one-shot call
        es, ec = PB.bsi_sum(OA, base, depth, R, idx)
        s, c = gpu_ctx.bsi_sum(batch, base, depth, out, idx)
        assert (s == es).all() and (c == ec).all(), (op, pred)
        qs = gpu_ctx.prepare_bsi_sum(batch, base, depth, filt=out, rows_f=idx)
        q.run()
        qs.run()
        s, c = qs.read()
        assert (s == es).all() and (c == ec).all(), (op, pred)
        # the one-shot call agrees
        o1, c1 = gpu_ctx.bsi_range(batch, base, op, depth, pred)
        assert (c1 == ecnt).all() and (_words_of(o1) == R.words()).all()
        o1.free()
        qs.free()
        q.free()
    with pytest.raises(L.FbkError):
        gpu_ctx.prepare_bsi_range(batch, base, 9, depth, 1)  # ErrInvalidRangeOperation
    with pytest.raises(L.FbkError):
        gpu_ctx.prepare_bsi_range(batch, base + 10**6, L.BSI_GT, depth, 1)
    batch.free()


@pytest.mark.parametrize("flags", [0, L.SETOP_OPTIMIZE])
def test_prepared_fold_materialised(gpu_ctx, mixed, flags):
    """fbk_query_fold: Union / Xor / Difference of k rows per group, the result rows kept on the device; with FBK_SETOP_OPTIMIZE
    the descriptors and payload bytes equal the one-shot fbk_fold_n's."""
    rows, g, filt, OA, OF = mixed
    batch = gpu_ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows)
    eu, ucnt = PB.union_n(OA, g)
    q = gpu_ctx.prepare_fold(L.OP_OR, batch, g, flags)
    for _ in range(2):
        q.run()
    assert (q.read() == ucnt).all()
    out = q.output()
    assert (_words_of(out) == eu.words()).all()
    for op in (L.OP_OR, L.OP_XOR, L.OP_ANDNOT, L.OP_AND):
        qq = gpu_ctx.prepare_fold(op, batch, g[:, :5], flags)
        qq.run()
        o1, c1 = gpu_ctx.fold_n(op, batch, g[:, :5], flags)
        assert (qq.read() == c1).all()
        d0, p0, _ = qq.output().download_flat()
        d1, p1, _ = o1.download_flat()
        assert d0.tobytes() == d1.tobytes() and p0.tobytes() == p1.tobytes(), op
        assert qq.output().to_roaring() == o1.to_roaring()
        o1.free()
        qq.free()
    q.free()
    with pytest.raises(L.FbkError):
        gpu_ctx.prepare_fold(L.OP_AND, batch, g[:, :0], flags)  # Intersect needs at least one row per group (executor.go:5363)
    batch.free()


def test_prepared_topn_orders_on_the_device(gpu_ctx, mixed):
    """fbk_query_topn against the one-shot fbk_topn (both ordering paths of which are tied to the oracle in test_gpu_topn.py)
    and the oracle's per-shard counts: thresholds, n, with and without a source row, repeated runs."""
    rows, g, filt, OA, OF = mixed
    n = g.shape[0]
    batch = gpu_ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows)
    F = gpu_ctx.upload_flat(filt.descs(), filt.payload(), filt.n_rows)
    fidx = np.arange(n)
    exp_counts = PB.topk_counts(OA, g, OF, fidx).sum(axis=0)
    for use_f in (True, False):
        for top, mt, tt in ((0, 0, 0), (5, 0, 0), (1, 0, 0), (0, 3000, 0), (4, 0, 30), (0, 0, 90)):
            if tt and not use_f:
                continue
            fa = (F, fidx) if use_f else (None, None)
            e_idx, e_cnt = gpu_ctx.topn(batch, g, top, *fa, min_threshold=mt, tanimoto_threshold=tt)
            q = gpu_ctx.prepare_topn(batch, g, top, *fa, min_threshold=mt, tanimoto_threshold=tt)
            for _ in range(2):
                q.run()
            idx, cnt = q.read()
            assert idx.tolist() == e_idx.tolist() and cnt.tolist() == e_cnt.tolist(), (use_f, top, mt, tt)
            if use_f and not mt and not tt:
                assert all(int(c) == int(exp_counts[i]) for i, c in zip(idx, cnt))
                if top == 0:
                    assert len(idx) == int((exp_counts != 0).sum())
            q.free()
    with pytest.raises(L.FbkError):
        gpu_ctx.prepare_topn(batch, g, 3, F, fidx, tanimoto_threshold=101)
    batch.free()
    F.free()


def test_prepared_row_records_follow_a_rewritten_batch(gpu_ctx, mixed):
    """Prepared folds / TopN resolve the descriptors of every (group / shard, slot) into contiguous records on their first run
    (k_resolve_rows).  Same results as the one-shot calls, which do not use them; and when the batch the query reads is REWRITTEN
    on the device (here: the output of a plan, re-run with another operation) the next run resolves again instead of chasing the
    old descriptors."""
    rows, g, filt, OA, OF = mixed
    n = g.shape[0]
    batch = gpu_ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows)
    F = gpu_ctx.upload_flat(filt.descs(), filt.payload(), filt.n_rows)
    fidx = np.arange(n)
    try:
        # prepared (resolved records) against the one-shot calls, whose kernels gather the descriptors through the row lists
        q1 = gpu_ctx.prepare_fold_intersection_count(L.OP_OR, batch, g, F, fidx)
        q2 = gpu_ctx.prepare_fold(L.OP_XOR, batch, g[:, :7], L.SETOP_OPTIMIZE)
        q3 = gpu_ctx.prepare_topn(batch, g, 0, F, fidx)
        q4 = gpu_ctx.prepare_count_matrix(batch, g, F, fidx.reshape(-1, 1))
        for q in (q1, q2, q3, q4):
            q.run()
            q.run()
        d2, p2, _ = q2.output().download_flat()
        o2, c2 = gpu_ctx.fold_n(L.OP_XOR, batch, g[:, :7], L.SETOP_OPTIMIZE)
        e_d2, e_p2, _ = o2.download_flat()
        assert q1.read().tolist() == gpu_ctx.fold_n_intersection_count(L.OP_OR, batch, g, F, fidx).tolist()
        assert q1.read().tolist() == PB.union_n_intersection_count(OA, g, OF, fidx)[0].tolist()
        assert q2.read().tolist() == c2.tolist() and d2.tobytes() == e_d2.tobytes() and p2.tobytes() == e_p2.tobytes()
        e_idx, e_cnt = gpu_ctx.topn(batch, g, 0, F, fidx)
        idx, cnt = q3.read()
        assert idx.tolist() == e_idx.tolist() and cnt.tolist() == e_cnt.tolist()
        assert (q4.read() == gpu_ctx.count_matrix(batch, g, F, fidx.reshape(-1, 1))).all()
        o2.free()
        for q in (q1, q2, q3, q4):
            q.free()
        # a query over a batch that changes under it
        ia, ib = g[:, :6].reshape(-1), g[:, 6:12].reshape(-1)  # 6 output rows per shard
        plan = gpu_ctx.plan(batch, ia, batch, ib)
        plan.setop(L.OP_OR)
        O = plan.output()
        og = np.arange(n * 6).reshape(n, 6)
        q = gpu_ctx.prepare_fold_intersection_count(L.OP_OR, O, og, F, fidx)
        qt = gpu_ctx.prepare_topn(O, og, 0, F, fidx)
        qm = gpu_ctx.prepare_count_matrix(O, og, O, og[:, ::-1].copy(), F, fidx)  # 6 x 6 rows: the kernel with the prepared program
        for op in (L.OP_OR, L.OP_AND, L.OP_XOR):
            plan.setop(op)  # rewrites O in place
            q.run()
            qt.run()
            # the count matrix's program (row tables, resolved array items: addresses INTO O's arena) follows the rewrite too
            qm.run()
            qm.run()
            gpu_ctx.set_option("matrix_fused", 0)
            try:
                e_m = gpu_ctx.count_matrix(O, og, O, og[:, ::-1].copy(), F, fidx)
            finally:
                gpu_ctx.set_option("matrix_fused", -1)
            assert (qm.read() == e_m).all(), op
            assert q.read().tolist() == gpu_ctx.fold_n_intersection_count(L.OP_OR, O, og, F, fidx).tolist(), op
            e_idx, e_cnt = gpu_ctx.topn(O, og, 0, F, fidx)
            idx, cnt = qt.read()
            assert idx.tolist() == e_idx.tolist() and cnt.tolist() == e_cnt.tolist(), op
        q.free()
        qt.free()
        qm.free()
        plan.free()
    finally:
        gpu_ctx.set_option("matrix_fused", -1)
    batch.free()
    F.free()


def test_detached_plan_output_belongs_to_the_caller(gpu_ctx, mixed):
    """fbk_plan_detach_output hands the set-op output over: the plan's next set-op writes a fresh batch and leaves the detached one
    alone, and the detached batch is an owned batch like any other — fbk_batch_compact, which refuses the borrowed outputs of plans
    and prepared queries, moves it into a right-sized arena (found by tests/test_gpu_fuzz_prepared.py: it used to be refused)."""
    rows, g, filt, OA, OF = mixed
    batch = gpu_ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows)
    ia, ib = g[:, :4].reshape(-1), g[:, 4:8].reshape(-1)
    plan = gpu_ctx.plan(batch, ia, batch, ib)
    plan.setop(L.OP_AND, L.SETOP_OPTIMIZE)
    with pytest.raises(L.FbkError):
        plan.output().compact()  # borrowed: the plan's next run rewrites it in place
    EA, ca = PB.setop(PB.OP_AND, OA, ia, OA, ib)
    d = plan.detach_output()
    with pytest.raises(L.FbkError):
        plan.output()  # nothing to lend until the next set-op
    plan.setop(L.OP_XOR)
    EX, cx = PB.setop(PB.OP_XOR, OA, ia, OA, ib)
    assert plan.output().h.value != d.h.value
    assert (_words_of(plan.output()) == EX.words()).all() and (plan.read() == cx).all()
    assert (_words_of(d) == EA.words()).all() and (d.count(np.arange(len(ia))) == ca).all()
    before = d.memory()[0]
    assert before == len(ia) * 16 * 8192
    after = d.compact()
    assert after < before and after == d.memory()[0]
    assert (_words_of(d) == EA.words()).all()
    plan.setop(L.OP_OR)  # and again after the compaction: still the caller's rows
    assert (_words_of(d) == EA.words()).all()
    plan.free()
    d.free()
    batch.free()


@pytest.fixture(scope="module")
def small_rows():
    """2 shards x 2 rows = 4 rows of each kind: dense words [4, 16, 1024], mixed rows from datagen.random_row, and the 4 x 4
    tables of |a & b| of both (numpy popcounts; the oracle's intersectionCount for the mixed rows)."""
    from oracle import pyoracle as O

    dense = D.dense_rows(4, 0.3, 8200)
    dtab = np.array([[int(np.bitwise_count(dense[i] & dense[j]).sum()) for j in range(4)] for i in range(4)], dtype=np.uint64)
    rng = D.rng_for(8201)
    mixed = [D.random_row(rng, r) for r in range(4)]
    by_slot = [{k & 15: c for k, c in row.items()} for row in mixed]
    mtab = np.array([[sum(O.intersection_count(a[s], b[s]) for s in a if s in b) for b in by_slot] for a in by_slot], dtype=np.uint64)
    dense.setflags(write=False)
    return dense, dtab, mixed, mtab


def test_caller_owned_counts_outlive_the_plan(gpu_ctx, small_rows):
    """A plan created with device_counts_ptr writes the caller's buffer and never frees it: the counts are still there after the
    plan is gone and the pool has handed the plan's own blocks out again, to eight further plans of the same shape."""
    import torch

    _, _, mixed, mtab = small_rows
    M = gpu_ctx.upload([D.to_fbk_row(r) for r in mixed])
    ra, rb = np.array([0, 1]), np.array([2, 3])
    want = mtab[ra, rb]
    try:
        counts = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        plan = gpu_ctx.plan(M, ra, M, rb, device_counts_ptr=counts.data_ptr())
        plan.intersection_count()
        gpu_ctx.synchronize()
        plan.free()
        for k in range(8):
            p = gpu_ctx.plan(M, rb, M, ra[::-1].copy())  # library-owned counts, other values
            p.intersection_count()
            assert (p.read() == mtab[rb, ra[::-1]]).all(), k
            p.free()
        assert (counts.cpu().numpy().view(np.uint64) == want).all()
    finally:
        M.free()


def test_freeing_the_hot_plan(gpu_ctx, small_rows):
    """A dense plan counted twice is the context's hot plan (the second launch is k_icount_dense_resident); freeing it must leave
    nothing behind that a later plan — maybe at the same address — could be mistaken for: its first count is cold, its next two
    hot, all three right.  (This guards the sequence, not the compare-exchange in ~fbk_plan by itself: fbk_plan_free is not a
    quiet call, so entering it has already ended the plan's residency when the destructor runs.)"""
    dense, dtab, _, _ = small_rows
    A = gpu_ctx.upload_dense(dense)
    try:
        plan = gpu_ctx.plan(A, [0, 1], A, [1, 0])
        for _ in range(2):
            plan.intersection_count()
            assert (plan.read() == dtab[[0, 1], [1, 0]]).all()
        plan.free()
        plan = gpu_ctx.plan(A, [2, 3], A, [3, 3])
        for k in range(3):
            plan.intersection_count()
            assert (plan.read() == dtab[[2, 3], [3, 3]]).all(), k
        plan.free()
    finally:
        A.free()


def _mixed_field(rng, n_rows, p_slot):
    """n_rows rows of array / run / bitmap containers (encodings by datagen.fbk_container_of_vals, each slot present with
    probability p_slot) and their words [n_rows, 16, 1024]"""
    rows, words = [], np.zeros((n_rows, 16, 1024), dtype=np.uint64)
    for r in range(n_rows):
        row = {}
        for s in np.nonzero(rng.random(16) < p_slot)[0]:
            kind = int(rng.integers(8))
            if kind == 0:
                vals = D.vals_density(rng, 0.3)  # a bitmap
            elif kind <= 3:
                vals = D.vals_runs(rng, int(rng.choice([16, 128, 1024])), 0.4)
            else:
                vals = np.unique(rng.integers(0, 65536, int(rng.integers(1, 3000)))).astype(np.int64)  # an array
            row[r * 16 + int(s)] = D.fbk_container_of_vals(vals)
            words[r, s] = D.words_of(vals)
        rows.append(row)
    return rows, words


def test_a_kept_count_matrix_plan_across_its_modes(gpu_ctx):
    """One prepared count matrix run under a changing option matrix_pass_kb — one pass over the 3 shards (a program that is kept,
    records resolved once), one shard per pass (72 cells are 576 B, 200 cells 1600 B: three passes, each with a program of its own),
    one pass again — then accumulated into its own result; beside it the one-shot calls.  Encoded rows through the in-kernel
    decode, dense batches, and the TopK shape (200 rows against one, no filter); counts against numpy popcounts of the same rows."""
    from featurebase_amd.roaring import GroupSelect

    ns, per = 3, 200
    rng = D.rng_for(8300)
    head, hw = _mixed_field(rng, ns * 18, 0.85)   # per shard 9 rows of A, 8 of B, the filter row
    tail, tw = _mixed_field(rng, ns * per, 0.1)   # per shard 200 sparse rows of a third field
    kinds = {c.typ for r in head + tail for c in r.values()}
    assert kinds == {L.TYPE_ARRAY, L.TYPE_RUN, L.TYPE_BITMAP}
    M = gpu_ctx.upload(head + [{k + ns * 18 * 16: c for k, c in r.items()} for r in tail])
    dw = D.dense_rows(ns * 18, 0.5, 8301)
    Dn = gpu_ctx.upload_dense(dw)
    g = np.arange(ns * 18).reshape(ns, 18)
    ra, rb, rf = g[:, :9], g[:, 9:17], g[:, 17]
    rt = ns * 18 + np.arange(ns * per).reshape(ns, per)

    def matrix(w):  # [n_a, n_b] over the shards
        return np.array([[sum(int(np.bitwise_count(w[ra[s, i]] & w[rb[s, j]] & w[rf[s]]).sum()) for s in range(ns)) for j in range(8)] for i in range(9)], dtype=np.uint64)

    topk = np.array([[sum(int(np.bitwise_count(tw[s * per + i] & hw[rf[s]]).sum()) for s in range(ns))] for i in range(per)], dtype=np.uint64)
    shapes = [("encoded", M, ra, M, rb, M, rf, matrix(hw), 1), ("dense", Dn, ra, Dn, rb, Dn, rf, matrix(dw), -1),
              ("topk", M, rt, M, rf.reshape(ns, 1), None, None, topk, -1)]
    assert all(exp.any() for *_, exp, _ in shapes)
    kept = {o: gpu_ctx.get_option(o) for o in ("matrix_pass_kb", "matrix_fused")}
    try:
        for name, A, a, B, b, F, f, exp, fused in shapes:
            gpu_ctx.set_option("matrix_fused", fused)
            q = gpu_ctx.prepare_count_matrix(A, a, B, b, F, f)
            for kb in (1 << 20, 1, 1 << 20):
                gpu_ctx.set_option("matrix_pass_kb", kb)
                q.run()
                assert (q.read() == exp).all(), (name, kb)
                assert (gpu_ctx.count_matrix(A, a, B, b, F, f) == exp).all(), (name, kb, "one-shot")
                cells, counts, matched = gpu_ctx.count_matrix_select(A, a, B, b, GroupSelect(), F, f)
                got = np.zeros(exp.size, dtype=np.uint64)
                got[cells] = counts
                assert matched == cells.size == int((exp != 0).sum()) and (got.reshape(exp.shape) == exp).all(), (name, kb, "select")
            q.run(accumulate=True)  # into the query's own result
            assert (q.read() == 2 * exp).all(), (name, "accumulate")
            q.free()
    finally:
        for o, v in kept.items():
            gpu_ctx.set_option(o, v)
        M.free()
        Dn.free()


def _run_mode_batch():
    """2 shards x 13 rows: three rows of field A, three of field B, one filter row, and an int field of depth 4 (exists, sign,
    four planes).  Every row has an array, a run and a bitmap container (slots 0 .. 2); the field has negative values."""
    rng = D.rng_for(8500)
    makers = (lambda: np.unique(rng.integers(0, 65536, 1500)).astype(np.int64), lambda: D.vals_runs(rng, 16, 0.5), lambda: D.vals_density(rng, 0.4))
    rows = []
    for s in range(2):
        for r in range(8):  # A, B, the filter, exists
            rows.append({(len(rows) * 16 + sl): makers[(r + sl) % 3]() for sl in range(3)})
        exists = rows[-1]
        for p in (0.3, 0.5, 0.5, 0.5, 0.5):  # sign and planes: subsets of exists
            rows.append({(len(rows) * 16 + (k & 15)): v[rng.random(v.size) < p] for k, v in exists.items()})
    assert all(np.intersect1d(rows[s * 13 + 8][(s * 13 + 8) * 16], rows[s * 13 + 9][(s * 13 + 9) * 16]).size for s in range(2))  # negative values
    conts = [{k: D.fbk_container_of_vals(v) for k, v in row.items()} for row in rows]
    assert {c.typ for row in conts[:16] for c in row.values()} == {L.TYPE_ARRAY, L.TYPE_RUN, L.TYPE_BITMAP}
    g = np.arange(26).reshape(2, 13)
    return conts, g[:, 0:3], g[:, 3:6], g[:, 6], g[:, 7]


def test_run_modes_by_kind(gpu_ctx):
    """Which kinds of prepared query take FBK_QUERY_ACCUMULATE and which a caller's device buffer (the rules of fbk_query_run): every
    kind accepts or refuses each of the two with FBK_E_INVALID; a refused run leaves the result of the run before it readable and
    unchanged; an accepted accumulate doubles the result, an accepted redirect reads back what the query's own buffer held."""
    import torch
    from featurebase_amd.roaring import bsi_leaf, compile_expr, row_leaf

    conts, ra, rb, rf, base = _run_mode_batch()
    M = gpu_ctx.upload(conts)
    depth = 4
    leaves, prog = compile_expr(("and", row_leaf(M, ra[:, 0]), ("or", row_leaf(M, rb[:, 1]), bsi_leaf(M, base, L.BSI_LT, depth, 2))))
    # kind -> (prepare, accumulate accepted, a caller's buffer accepted)
    table = {
        "count matrix": (lambda: gpu_ctx.prepare_count_matrix(M, ra, M, rb, M, rf), True, True),
        "GroupBy Sum": (lambda: gpu_ctx.query_count_matrix_sum(M, ra, M, rb, M, base, depth, M, rf), False, False),
        "fold count": (lambda: gpu_ctx.prepare_fold_intersection_count(L.OP_OR, M, ra, M, rf), True, True),
        "fold rows": (lambda: gpu_ctx.prepare_fold(L.OP_OR, M, ra), False, True),
        "BSI Sum": (lambda: gpu_ctx.prepare_bsi_sum(M, base, depth, filt=M, rows_f=rf), False, True),
        "Sum(Range)": (lambda: gpu_ctx.prepare_bsi_sum(M, base, depth, L.BSI_GT, 3, M, rf), False, True),
        "BSI Range rows": (lambda: gpu_ctx.prepare_bsi_range(M, base, L.BSI_LT, depth, 5), False, True),
        "expr rows": (lambda: gpu_ctx.query_expr(leaves, prog), False, False),
        "expr count-only": (lambda: gpu_ctx.query_expr(leaves, prog, count_only=True), True, True),
        "expr Sum": (lambda: gpu_ctx.query_expr_bsi(L.AGG_SUM, leaves, prog, M, base, depth), True, True),
        "expr Min": (lambda: gpu_ctx.query_expr_bsi(L.AGG_MIN, leaves, prog, M, base, depth), False, False),
        "TopN": (lambda: gpu_ctx.prepare_topn(M, ra, 2, M, rf), False, False),
    }
    with_rows = ("fold rows", "BSI Range rows", "expr rows")

    def state(q, kind):
        r = q.read()
        parts = [np.asarray(x) for x in (r if isinstance(r, tuple) else (r,))]
        if kind in with_rows:
            parts.append(_words_of(q.output()))
        return parts

    def same(a, b):
        return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))

    try:
        for kind, (prepare, acc_ok, dev_ok) in table.items():
            q = prepare()
            q.run()
            first = state(q, kind)
            assert any(p.any() for p in first), kind
            cell = torch.zeros(q.result_ptr()[1] // 8, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for mode, ok, args in (("accumulate", acc_ok, dict(accumulate=True)), ("device_out", dev_ok, dict(device_ptr=cell.data_ptr()))):
                if ok:
                    q.run(**args)
                    got = state(q, kind)
                    exp = [2 * p for p in first] if mode == "accumulate" else first
                    assert same(got, exp), (kind, mode)
                    q.run()  # (back to the query's own buffer, overwritten)
                    assert same(state(q, kind), first), (kind, mode)
                else:
                    with pytest.raises(L.FbkError) as e:
                        q.run(**args)
                    assert e.value.code == L.FBK_E_INVALID, (kind, mode)
                    assert same(state(q, kind), first), (kind, mode)
            if not acc_ok and not dev_ok:
                with pytest.raises(L.FbkError) as e:
                    q.run(cell.data_ptr(), accumulate=True)
                assert e.value.code == L.FBK_E_INVALID, kind
                assert same(state(q, kind), first), kind
            q.free()
    finally:
        M.free()
