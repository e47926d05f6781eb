"""Structural fuzz of the prepared forms: fbk_query_* (count matrix, fold + count, BSI Sum, one-pass Sum(Range), BSI Range, materialised
fold, TopN) and fbk_plan_*.  They are the part of the ABI that keeps state between launches — resident row lists, result buffers and
output batches rewritten in place, resolved row records, the kept program of the count matrix, pass buffers sized by an option, the
bookkeeping behind fbk_query_read — so a case is a SCHEDULE, not a call: several live queries of different kinds on one context, run
in arbitrary order into their own buffers or caller cells, read (also stale), with the batches under them rewritten (a plan's output)
or compacted, options changed between prepare and run, one-shot calls in between, queries freed and prepared under the live ones,
outputs of row-valued queries as operands of later ones.  tests/fuzz_prepared_gen.py makes the cases and the model that gives every
step's expectation (numpy set algebra, oracle/pybatch.py for BSI, oracle/pytopn.py's rules for TopN); tests/test_fuzz_prepared_cpu.py
checks both without a GPU and asserts what the default iterations cover.  Everything is integer and bit-exact.  A refusal
(FBK_E_INVALID) passes only where the generator predicted it.

FBK_FUZZ_ITERS=<n> runs more iterations, FBK_TEST_SEED re-rolls them (scripts/fuzz_parity.sh).  A failure names seed, iteration, step
and query kind: G.Case(it) under that FBK_TEST_SEED is the same case again."""
import numpy as np
import pytest

import datagen as D
import fuzz_prepared_gen as G
from featurebase_amd import lib as L

pytestmark = pytest.mark.gpu
ITERS = G.ITERS
popc = lambda w: int(np.bitwise_count(w).sum())  # noqa: E731


def out_words(batch, n):
    res = batch.download()
    assert len(res) == n
    W = np.zeros((n, 16, 1024), dtype=np.uint64)
    for r, row in enumerate(res):
        for k, c in row.items():
            assert c.n == popc(c.words()) and c.n > 0, (r, k)  # empty results are nil slots
            W[r, k & 15] = c.words()
    return W, res


def check_optimized(O, res):
    """FBK_SETOP_OPTIMIZE: every container has the encoding Container.optimize() picks for its content"""
    for row in res:
        for c in row.values():
            oc = O.optimize(O.OContainer.bitmap(c.words()))
            assert c.n and c.typ == oc.typ and c.n == oc.n
            assert np.array_equal(np.asarray(c.data).reshape(-1), np.asarray(oc.data()).reshape(-1))


def upload_static(ctx, rows, W):
    return ctx.upload([D.to_fbk_row(r) for r in rows]) if rows is not None else ctx.upload_dense(W.reshape(-1))


def refused(call):
    with pytest.raises(L.FbkError) as e:
        call()
    assert e.value.code == L.FBK_E_INVALID, e.value


class Device:
    """The world of a case on the device and its live queries."""

    def __init__(self, ctx, O, case):
        import torch

        self.torch, self.ctx, self.O, self.c = torch, ctx, O, case
        self.b, self.q, self.cells = {}, {}, {}
        self.plan = None
        self.compacts = 0

    def open(self):
        ctx, case = self.ctx, self.c
        for name in case.statics:
            self.b[name] = upload_static(ctx, case.rows[name], case.W0[name])
        self.plan = ctx.plan(self.b["S0"], case.ia, self.b["S1"], case.ib)
        self.plan.setop(case.op0, 0)
        self.b["C"], _ = ctx.setop(case.opc, self.b["S0"], case.ja, self.b["S1"], case.jb, 0)
        for name in ("O", "C"):
            assert np.array_equal(out_words(self.batch(name), case.size[name])[0], case.W0[name]), name

    def batch(self, name):
        if name is None:
            return None
        if name == "O":
            o = self.plan.output()
            o.owned = False  # (borrowed: the plan frees it)
            return o
        return self.q[int(name[1:])].output() if name.startswith("q") else self.b[name]

    def close(self):
        errors = []
        for name, val in G.DEFAULTS.items():
            self.ctx.set_option(name, val)
        for thing in [self.q[i] for i in sorted(self.q, reverse=True)] + [self.plan] + [self.b[n] for n in sorted(self.b)]:  # dependants first
            try:
                if thing is not None:
                    thing.free()
            except Exception as e:  # whatever failed: everything else is still freed
                errors.append(e)
        return errors

    # -- the calls of a query description
    def prepare(self, q):
        ctx, a, b, f = self.ctx, self.batch(q["a"]), self.batch(q["b"]), self.batch(q["f"])
        k = q["kind"]
        if k == "count_matrix":
            return ctx.prepare_count_matrix(a, q["ra"], b, q["rb"], f, q.get("rf"), keep_per_shard=q["keep"])
        if k == "fold_icount":
            return ctx.prepare_fold_intersection_count(q["op"], a, q["groups"], f, q.get("rf"))
        if k == "fold":
            return ctx.prepare_fold(q["op"], a, q["groups"], q["flags"])
        if k == "bsi_sum":
            return ctx.prepare_bsi_sum(a, q["base"], q["depth"], filt=f, rows_f=q.get("rf"))
        if k == "bsi_range_sum":
            return ctx.prepare_bsi_sum(a, q["base"], q["depth"], q["op"], q["pred"], f, q.get("rf"))
        if k == "bsi_range":
            return ctx.prepare_bsi_range(a, q["base"], q["op"], q["depth"], q["pred"])
        return ctx.prepare_topn(a, q["ra"], q["top"], f, q.get("rf"), min_threshold=q["mt"], tanimoto_threshold=q["tt"])

    def oneshot(self, q, res):
        ctx, a, b, f = self.ctx, self.batch(q["a"]), self.batch(q["b"]), self.batch(q["f"])
        k = q["kind"]
        if k == "count_matrix":
            tot, ps = ctx.count_matrix(a, q["ra"], b, q["rb"], f, q.get("rf"), per_shard=True)
            assert np.array_equal(ps, res["ps"]) and np.array_equal(tot, res["value"])
        elif k == "fold_icount":
            assert np.array_equal(ctx.fold_n_intersection_count(q["op"], a, q["groups"], f, q.get("rf")), res["value"])
        elif k == "fold":
            out, cnt = ctx.fold_n(q["op"], a, q["groups"], q["flags"])
            W, rows = out_words(out, q["n"])
            out.free()
            assert np.array_equal(W, res["out"]) and np.array_equal(cnt, res["value"])
            if q["flags"]:
                check_optimized(self.O, rows)
        elif k == "bsi_sum":
            s, c = ctx.bsi_sum(a, q["base"], q["depth"], f, q.get("rf"))
            assert np.array_equal(s, res["sums"]) and np.array_equal(c, res["counts"])
        elif k == "bsi_range_sum":
            s, c = ctx.bsi_range_sum(a, q["base"], q["op"], q["depth"], q["pred"], f, q.get("rf"))
            assert np.array_equal(s, res["sums"]) and np.array_equal(c, res["counts"])
        elif k == "bsi_range":
            out, cnt = ctx.bsi_range(a, q["base"], q["op"], q["depth"], q["pred"])
            W, _ = out_words(out, q["n"])
            out.free()
            assert np.array_equal(W, res["out"]) and np.array_equal(cnt, res["value"])
        else:
            idx, cnt = ctx.topn(a, q["ra"], q["top"], f, q.get("rf"), min_threshold=q["mt"], tanimoto_threshold=q["tt"])
            assert (idx.tolist(), [int(x) for x in cnt]) == tuple(res["topn"])

    def cell_value(self, qi):
        self.ctx.synchronize()
        return self.cells[qi].cpu().numpy().view(np.uint64).copy()

    def check_cell(self, qi, q, exp):
        got = self.cell_value(qi)
        k = q["kind"]
        if k in ("bsi_sum", "bsi_range_sum"):  # the raw per-shard records (include/fbk.h, fbk_query_read)
            if k == "bsi_sum":
                h = got.reshape(q["n"], 3)
                sums, counts = (h[:, 0] - h[:, 1]).view(np.int64), h[:, 2]
            else:
                h = got.reshape(q["n"], 4)
                sums = ((h[:, 0] - h[:, 1]) if q["scan_positive"] else (h[:, 1] - h[:, 0])).view(np.int64)
                counts = h[:, 2] + h[:, 3]
            assert np.array_equal(sums, exp["res"]["sums"]) and np.array_equal(counts, exp["res"]["counts"])
        else:
            assert np.array_equal(got, exp["cell"])

    # -- steps
    def execute(self, st, exp):
        ctx, c = self.ctx, self.c
        qi = st.get("q")
        q = c.queries[qi] if qi is not None else None
        do = st["do"]
        if do == "prepare":
            if exp["refused"]:
                return refused(lambda: self.prepare(q))
            self.q[qi] = self.prepare(q)
            self.cells[qi] = self.torch.full((G.cell_words(q),), G.CELL_FILL, dtype=self.torch.int64, device="cuda")
            self.torch.cuda.synchronize()
        elif do == "run":
            ptr = self.cells[qi].data_ptr() if st["dest"] == "cell" else 0
            if exp["refused"]:
                return refused(lambda: self.q[qi].run(ptr, accumulate=st["acc"]))
            self.q[qi].run(ptr, accumulate=st["acc"])
            if st["dest"] == "cell":
                self.check_cell(qi, q, exp)
        elif do == "read":
            self.read(qi, q, exp)
        elif do == "mutate":
            if exp["refused"]:
                return refused(lambda: self.plan.setop(st["op"], st["flags"]))
            self.plan.setop(st["op"], st["flags"])
            W, rows = out_words(self.batch("O"), c.size["O"])
            assert np.array_equal(W, exp["words"])
            assert self.plan.read().tolist() == [popc(w) for w in exp["words"]]
            if st["flags"]:
                check_optimized(self.O, rows)
        elif do == "compact":
            before = self.b["C"].memory()[0]
            after = self.b["C"].compact()
            assert after == self.b["C"].memory()[0] and (after < before if (self.compacts == 0 and not c.dense) else after == before), (before, after)
            self.compacts += 1
        elif do == "set_option":
            for name, val in st["opts"].items():
                ctx.set_option(name, val)
        elif do == "oneshot":
            self.oneshot(q, exp["res"])
        elif do == "free":
            self.q.pop(qi).free()
            del self.cells[qi]
        else:
            raise ValueError(do)

    def read(self, qi, q, exp):
        Q, k, last, res = self.q[qi], q["kind"], exp["last"], exp["res"]
        if k == "count_matrix":
            if q["keep"]:
                tot, ps = Q.read(per_shard=True)
                assert np.array_equal(ps, res["ps"])
            else:
                tot = Q.read()
            assert np.array_equal(tot.reshape(-1), last)
        elif k == "fold_icount":
            assert np.array_equal(Q.read(), last)
        elif k in ("bsi_sum", "bsi_range_sum"):
            s, cn = Q.read()
            assert np.array_equal(s, last["sums"]) and np.array_equal(cn, last["counts"])
        elif k == "topn":
            idx, cnt = Q.read()
            assert (idx.tolist(), [int(x) for x in cnt]) == tuple(last["topn"])
        else:  # the row-valued kinds: cardinalities, and the rows the last run left in the query's batch
            assert np.array_equal(Q.read(), last)
            W, rows = out_words(Q.output(), q["n"])
            assert np.array_equal(W, res["out"])
            if k == "fold" and q["flags"]:
                check_optimized(self.O, rows)
                if not exp["stale"]:  # byte for byte what the one-shot call makes of the same rows
                    o1, c1 = self.ctx.fold_n(q["op"], self.batch(q["a"]), q["groups"], q["flags"])
                    d0, p0, _ = Q.output().download_flat()
                    d1, p1, _ = o1.download_flat()
                    o1.free()
                    assert d0.tobytes() == d1.tobytes() and p0.tobytes() == p1.tobytes() and np.array_equal(c1, last)


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_prepared_schedule(gpu_ctx, oracle, it):
    case = G.Case(it)
    model = G.Model(case)
    dev = Device(gpu_ctx, oracle, case)
    try:
        dev.open()
        for si, st in enumerate(case.steps):
            try:
                dev.execute(st, model.apply(st))
            except Exception as e:
                raise AssertionError(f"{case.describe(si)}: {type(e).__name__}: {e}") from e
    finally:
        errors = dev.close()
    assert not errors, errors


@pytest.mark.parametrize("it", range(ITERS))
def test_fuzz_plan_forms(gpu_ctx, oracle, it):
    """fbk_plan_*: set-ops with and without FBK_SETOP_OPTIMIZE alternating on one plan, the total after each, the three count forms,
    totals into a caller cell, and fbk_plan_detach_output: the detached batch keeps its rows across the plan's later set-ops, the
    plan's next output is another batch with the new rows, the caller frees what it detached."""
    import torch

    c = G.PlanCase(it)
    m = G.PlanModel(c)
    X = upload_static(gpu_ctx, c.rows["X"], c.W["X"])
    Y = X if c.same else upload_static(gpu_ctx, c.rows["Y"], c.W["Y"])
    cell = torch.full((1,), G.CELL_FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    plan, detached = gpu_ctx.plan(X, c.ia, Y, c.ib), []

    def cell_value():
        gpu_ctx.synchronize()
        return int(cell.cpu().numpy().view(np.uint64)[0])

    try:
        for si, st in enumerate(c.steps):
            what = f"seed {D.SEED:#x} it {it} step {si} kind plan: {st}"
            m.apply(st)
            if st[0] == "setop":
                plan.setop(st[1], st[2])
                out = plan.output()
                assert all(out.h.value != d.h.value for d, _ in detached), what
                W, rows = out_words(out, c.n)
                assert np.array_equal(W, m.out), what
                assert np.array_equal(plan.read(), m.counts), what
                if st[2]:
                    check_optimized(oracle, rows)
                for d, w in detached:  # what was handed out is the caller's: untouched by the plan's later runs
                    assert np.array_equal(out_words(d, c.n)[0], w), what
            elif st[0] == "total":
                plan.total()
            elif st[0] == "total_cell":
                plan.total(cell.data_ptr())
                assert cell_value() == m.cell, what
            elif st[0] == "intersection_count":
                plan.intersection_count()
            elif st[0] == "intersection_count_total":
                plan.intersection_count_total()
            elif st[0] == "intersection_count_accumulate":
                plan.intersection_count_accumulate(cell.data_ptr())
                assert cell_value() == m.cell, what
            elif st[0] == "read":
                if m.total is None:
                    assert np.array_equal(plan.read(), m.counts), what
                else:
                    counts, total = plan.read(want_total=True)
                    assert np.array_equal(counts, m.counts) and int(total) == m.total, what
            elif st[0] == "detach":
                d = plan.detach_output()
                assert np.array_equal(out_words(d, c.n)[0], m.detached[-1]), what
                detached.append((d, m.detached[-1]))
                if st[1]:  # the caller's batch now: compact accepts it (it refuses what a plan still owns) and keeps the rows
                    d.compact()
                    assert np.array_equal(out_words(d, c.n)[0], m.detached[-1]), what
                refused(plan.output)  # nothing to borrow until the next set-op
        assert detached
    finally:
        plan.free()
        for d, _ in detached:
            d.free()
        if Y is not X:
            Y.free()
        X.free()
