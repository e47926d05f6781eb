"""Sum / Min / Max of an int field over a call tree in the tree's own launch (fbk_expr_bsi_agg) against the pair of calls it replaces
(fbk_expr_eval with FBK_SETOP_OPTIMIZE as Executor::eval asks for it, then fbk_bsi_sum / _min / _max with that row as the filter):
timings for DESIGN.md §6, one JSON file per aggregate under --out.  bench_expr.py's shape: 96 shards of config 3's mixed rows, the
WHERE clause Intersect(Union(r0, r1), Not(r2), Row(x > 5)) with x its 64-plane field; the aggregated field is a 32-bit one (32 dense
planes + exists + sign, every column holding a value).  Both forms run ALTERNATING in one process on resident rows and their outputs
are compared every round.  The yardstick is the pair, never the new call against itself.

Per form: wall clock of the synchronous call(s) (median, min, max over --runs alternations after two warm-up rounds) and the kernel
time the library's own events report (option time_kernels; the pair: the sum of its two kernels).  Algorithmic bytes: every operand's
encoded payload once, the 34 rows of the aggregated fragment once; the pair writes the filter row and reads it back.  Then the
prepared forms, launch-only: fbk_query_expr_bsi against fbk_query_expr + fbk_query_bsi_sum chained through fbk_query_output, blocks of
--block runs between two synchronisations, alternating.
Usage: python scripts/bench_expr_agg.py --out profiles [--only sum|min|max] [--runs 200] [--shards 96]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_expr as BE  # noqa: E402

DEPTH = 32


def stats(xs):
    return BE.stats(xs)


def kernel_ns(ctx, fn, n):
    """median over n runs of the kernel time(s) fn's calls report, summed per run"""
    ctx.set_option("time_kernels", 1)
    try:
        out = [fn(lambda: ctx.get_option("last_kernel_ns")) for _ in range(n)]
    finally:
        ctx.set_option("time_kernels", 0)
    return round(float(np.median(out)) / 1e3, 1)


def case(w, field, base, name, tree, what, runs, block):
    ctx, L = w.ctx, w.L
    agg = {"sum": L.AGG_SUM, "min": L.AGG_MIN, "max": L.AGG_MAX}[name]
    two = {"sum": ctx.bsi_sum, "min": ctx.bsi_min, "max": ctx.bsi_max}[name]
    leaves, prog = BE.leaves_and_program(w, tree)

    def fused():
        return ctx.expr_bsi_agg(agg, leaves, prog, field, base, DEPTH)

    def pair(after=None):
        b, _ = ctx.expr_eval(leaves, prog, L.SETOP_OPTIMIZE)
        k = after() if after else 0
        r = two(field, base, DEPTH, b, w.idx)
        k += after() if after else 0
        return r, b, k

    # bytes (untimed)
    fv, fc = fused()
    (pv, pc), b, _ = pair()
    assert fv.tolist() == pv.tolist() and fc.tolist() == pc.tolist(), f"{name}: the fused result differs from the pair's"
    row_bytes = BE.Rows(b, w.idx, True).nbytes()
    b.free()
    tree_bytes = BE.fused_bytes(w, tree)
    field_bytes = w.n * (DEPTH + 2) * 16 * 8192
    out = {"case": name, "what": what, "shards": w.n, "runs": runs, "bit_depth": DEPTH, "program_words": int(prog.size), "leaves": len(leaves),
           "columns_aggregated": int(fc.sum()), "outputs_equal_every_round": True,
           "fused": {"calls": 1, "algorithmic_bytes_read": tree_bytes + field_bytes, "algorithmic_bytes_written": 0},
           "pair": {"calls": 2, "algorithmic_bytes_read": tree_bytes + field_bytes + row_bytes, "algorithmic_bytes_written": row_bytes,
                    "form": "fbk_expr_eval (FBK_SETOP_OPTIMIZE), then fbk_bsi_%s with the row as filter" % name}}

    def pair_kernels(read):
        _, b, k = pair(read)
        b.free()
        return k

    def fused_kernel(read):
        fused()
        return read()

    out["fused"]["kernel_us_median"] = kernel_ns(ctx, fused_kernel, max(5, runs // 8))
    out["pair"]["kernels_us_median"] = kernel_ns(ctx, pair_kernels, max(5, runs // 8))
    # wall clock of the synchronous calls, alternating; outputs compared every round
    tf, tp = [], []
    for i in range(runs + 2):
        t0 = time.perf_counter()
        fv, fc = fused()
        t1 = time.perf_counter()
        (pv, pc), b, _ = pair()
        t2 = time.perf_counter()
        b.free()
        assert fv.tolist() == pv.tolist() and fc.tolist() == pc.tolist(), f"{name}: round {i} differs"
        if i >= 2:
            tf.append(t1 - t0)
            tp.append(t2 - t1)
    out["fused"]["call"] = stats(tf)
    out["pair"]["call"] = stats(tp)
    out["fused_over_pair_wall"] = round(out["fused"]["call"]["median_us"] / out["pair"]["call"]["median_us"], 3)
    out["fused_over_pair_kernels"] = round(out["fused"]["kernel_us_median"] / out["pair"]["kernels_us_median"], 3)
    if name == "sum":  # the prepared forms: launch-only runs, `block` of them between two synchronisations
        qa = ctx.query_expr_bsi(agg, leaves, prog, field, base, DEPTH)
        qe = ctx.query_expr(leaves, prog, L.SETOP_OPTIMIZE)
        qe.run()
        qs = ctx.prepare_bsi_sum(field, base, DEPTH, filt=qe.output(), rows_f=w.idx)
        ta, tc = [], []
        for i in range(max(4, runs // block) + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                qa.run()
            ctx.synchronize()
            t1 = time.perf_counter()
            for _ in range(block):
                qe.run()
                qs.run()
            ctx.synchronize()
            t2 = time.perf_counter()
            a, c = qa.read(), qs.read()
            assert a[0].tolist() == c[0].tolist() == fv.tolist() and a[1].tolist() == c[1].tolist(), "prepared forms differ"
            if i >= 1:
                ta.append((t1 - t0) / block)
                tc.append((t2 - t1) / block)
        for q in (qs, qe, qa):
            q.free()
        out["prepared"] = {"block": block, "fused_run": stats(ta), "chained_runs": stats(tc),
                           "chained_form": "fbk_query_expr (FBK_SETOP_OPTIMIZE) + fbk_query_bsi_sum over fbk_query_output",
                           "fused_over_chained": round(stats(ta)["median_us"] / stats(tc)["median_us"], 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--shards", type=int, default=96)
    a = ap.parse_args()
    import datagen as D
    from featurebase_amd import lib as L
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    w = BE.World(ctx, a.shards)
    planes = D.dense_rows(a.shards * (DEPTH + 2), 0.5, 5002).reshape(a.shards, DEPTH + 2, 16, 1024)
    planes[:, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)  # exists: every column has a value
    field = ctx.upload_dense(planes.reshape(-1))
    del planes
    base = np.arange(a.shards, dtype=np.uint32) * (DEPTH + 2)
    what = "Intersect(Union(r0, r1), Not(r2), Row(x > 5))"
    tree = ("and", ("or", w.r(0), w.r(1)), ("not", w.exists(), w.r(2)), w.pred(L.BSI_GT, 5))
    os.makedirs(a.out, exist_ok=True)
    for name in ("sum", "min", "max"):
        if a.only and name != a.only:
            continue
        res = case(w, field, base, name, tree, f"{name.capitalize()}(field32) WHERE {what}", a.runs, a.block)
        with open(os.path.join(a.out, f"expr_agg_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res), flush=True)
    for b in (field, w.batch, w.F, w.V):
        b.free()
    ctx.close()


if __name__ == "__main__":
    main()
