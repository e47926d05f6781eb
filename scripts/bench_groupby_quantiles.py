"""GroupBy with a percentile per group (fbk_count_matrix_quantiles): timings for docs/history/DESIGN_group_quantiles_measurements.md,
one JSON file per workload under --out.  Rows are generated on the device (bench_groupby_minmax.py's mutex-like rows: every column
in one A row and one B row, values on three quarters of the columns); the time is the library's own events around the kernels of a
call (option time_kernels -> last_kernel_ns: every pass's memset, histogram launches and resolve), warm runs, median and p10 / p90.
Every workload compares the outputs of its arms.

  paths  128 shards; 1 .. 1024 groups; depths 8 and 20; n_q = 1 (the median) and 3 (quartiles); FBK_GQUANT_LDS (where the (group,
         request) pairs are within its cap) and FBK_GQUANT_GLOBAL pinned, alternating in one process.  What fixes kAutoLdsPairs: the
         largest swept number of pairs up to which the LDS path's median is not above the GLOBAL path's in every row.
         The digit widths are compared by running this workload on two builds of the library (FBK_LIB_PATH; --tag and --digits name
         the build: -DFBK_GQUANT_LDS_DIGIT / -DFBK_GQUANT_GLOBAL_DIGIT).
  old    128 shards, depth 20, the median; 8 groups (4 x 2) and 1024 groups (32 x 32): the one call against the composition it
         replaces — per group fbk_setop (AND), fbk_bsi_quantiles for the total and fbk_bsi_quantiles for the rank computed from it
         —, wall time of both in the same process, each arm repeated, outputs compared.
Usage: python scripts/bench_groupby_quantiles.py --out profiles [--only paths|old] [--runs 10] [--tag groupby_quantiles] [--digits 8,8]"""
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

from bench_groupby_minmax import mutex_batches, stats  # noqa: E402

AUTO, LDS, GLOBAL = 0, 1, 2
SIDES = [(1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8), (16, 8), (16, 16), (32, 32)]
FRACTIONS = {1: [(1, 2)], 3: [(1, 4), (1, 2), (3, 4)]}


def same(a, b):
    return bool(all(np.array_equal(x, y) for x, y in zip(a, b)))


def time_paths(ctx, args, depth, fr, paths, runs):
    """the pinned paths alternate, so that clocks and caches are shared fairly.  Returns ({path: stats}, {path: outputs})"""
    ns, out = {p: [] for p in paths}, {}
    ctx.set_option("time_kernels", 1)
    try:
        for r in range(3 + runs):
            for p in paths:
                out[p] = ctx.count_matrix_quantiles(*args, depth, fr, path=p)
                if r >= 3:
                    ns[p].append(ctx.get_option("last_kernel_ns"))
    finally:
        ctx.set_option("time_kernels", 0)
    return {p: stats(v) for p, v in ns.items()}, out


def paths(ctx, torch, runs, digits):
    lds_cap = (64 << 10) // (4 << digits[0])
    rows = []
    for depth in (8, 20):
        for n_a, n_b in SIDES:
            n_sh = 128
            (bA, bB, bS), ra, rb, base = mutex_batches(ctx, torch, n_sh, n_a, n_b, depth, 300 + depth)
            for n_q, fr in FRACTIONS.items():
                pairs = n_a * n_b * n_q
                pins = [LDS, GLOBAL] if pairs <= lds_cap else [GLOBAL]
                t, out = time_paths(ctx, (bA, ra, bB, rb, bS, base), depth, fr, pins, runs)
                row = {"shards": n_sh, "n_a": n_a, "n_b": n_b, "groups": n_a * n_b, "n_q": n_q, "pairs": pairs, "depth": depth, "lds_digit": digits[0],
                       "global_digit": digits[1], "global": t[GLOBAL], "lds": t.get(LDS), "outputs_equal": same(out[GLOBAL], out[LDS]) if LDS in out else True,
                       "groups_non_empty": int((out[GLOBAL][2] > 0).sum())}
                if LDS in t:
                    row["lds_not_slower"] = t[LDS]["median_us"] <= t[GLOBAL]["median_us"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            for b in (bA, bB, bS):
                b.free()
    # the rule: the largest swept pair count p such that at every swept row of at most p pairs the LDS path is not slower
    swept = sorted({r["pairs"] for r in rows if r["lds"]})
    auto = 0
    for p in swept:
        if all(r["lds_not_slower"] for r in rows if r["lds"] and r["pairs"] <= p):
            auto = p
    return {"workload": "paths", "rows": rows, "lds_cap": lds_cap, "kAutoLdsPairs_from_sweep": auto, "outputs_equal": all(r["outputs_equal"] for r in rows)}


def old_path(ctx, torch, runs, digits):
    from featurebase_amd import lib as L

    res = []
    for n_a, n_b, reps in ((4, 2, 5), (32, 32, 3)):
        n_sh, depth, fr = 128, 20, [(1, 2)]
        (bA, bB, bS), ra, rb, base = mutex_batches(ctx, torch, n_sh, n_a, n_b, depth, 331)
        idx = np.arange(n_sh)
        ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, fr)  # warm
        new_t, old_t = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            new = ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, fr)
            new_t.append(time.perf_counter() - t0)
            # the composition: AND of the two rows per group, the total, then the value at the rank computed from it
            t0 = time.perf_counter()
            old = (np.zeros((n_a, n_b, 1), np.int64), np.zeros((n_a, n_b, 1), np.uint64), np.zeros((n_a, n_b), np.uint64))
            for i in range(n_a):
                for j in range(n_b):
                    m, _ = ctx.setop(L.OP_AND, bA, ra[:, i], bB, rb[:, j])
                    _, _, n = ctx.bsi_quantiles(bS, base, depth, [], m, idx)
                    if n:
                        k = max(1, -(-n * fr[0][0] // fr[0][1])) - 1
                        v, c, _ = ctx.bsi_quantiles(bS, base, depth, [k], m, idx)
                        old[0][i, j, 0], old[1][i, j, 0] = v[0], c[0]
                    old[2][i, j] = n
                    m.free()
            old_t.append(time.perf_counter() - t0)
        ctx.set_option("time_kernels", 1)
        ctx.count_matrix_quantiles(bA, ra, bB, rb, bS, base, depth, fr)
        kernel_us = ctx.get_option("last_kernel_ns") / 1e3
        ctx.set_option("time_kernels", 0)
        for b in (bA, bB, bS):
            b.free()
        o = np.array(old_t) * 1e3
        res.append({"n_a": n_a, "n_b": n_b, "groups": n_a * n_b, "one_call_ms": round(float(np.median(new_t)) * 1e3, 2), "one_call_max_ms": round(max(new_t) * 1e3, 2),
                    "one_call_kernels_us": round(kernel_us, 1), "composition_ms": round(float(np.median(o)), 1), "composition_min_ms": round(float(o.min()), 1),
                    "composition_max_ms": round(float(o.max()), 1), "composition_calls": n_a * n_b * 3, "repetitions": reps,
                    "one_call_not_slower_beyond_spread": bool(np.median(new_t) * 1e3 <= np.median(o) + (o.max() - o.min())),
                    "speedup": round(float(np.median(o)) / (float(np.median(new_t)) * 1e3), 1), "outputs_equal": same(new, old)})
        print(json.dumps(res[-1]), flush=True)
    return {"workload": "old_path", "shards": 128, "depth": 20, "fraction": [1, 2], "lds_digit": digits[0], "global_digit": digits[1], "shapes": res,
            "outputs_equal": all(r["outputs_equal"] for r in res)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--tag", default="groupby_quantiles")
    ap.add_argument("--digits", default="8,8", help="the LDS and GLOBAL digit of the library in use (a label: the build decides)")
    a = ap.parse_args()
    digits = tuple(int(x) for x in a.digits.split(","))
    import torch

    if not os.environ.get("FBK_LIB_PATH"):
        import __graft_entry__ as g

        g.build()
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for name, fn in (("paths", paths), ("old", old_path)):
        if a.only and name != a.only:
            continue
        r = fn(ctx, torch, a.runs, digits)
        print(json.dumps({k: v for k, v in r.items() if k != "rows"}), flush=True)
        with open(os.path.join(a.out, f"{a.tag}_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
        ok = ok and r["outputs_equal"]
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
