"""GroupBy having / sort / offset / limit on the device (fbk_count_cube_select, fbk_count_matrix_select, fbk_count_matrix_sum_select)
against the path they replace, for docs/history/DESIGN_groupby_select_measurements.md; one JSON file per case under --out.

The replaced path is the full call — every group to the host — followed by the host selection of fbk_group_select_plan.h, reached
through fbk_select_groups with FBK_GROUPSEL_HOST (no device work).  The two forms alternate in one process (a round = one run of
each, after --warmup rounds), both timed by the host clock around calls that end in a device synchronise, and their outputs are
compared.  There is no pass mark: the numbers and their spread are what the document records.

Cases: a cube of 256^3 cells, a count matrix and a Sum (bit depth 8) of 4096 x 4096 cells, all over dense rows of one shard, and two
count matrices and Sums between 4096 and 2^17 cells (64 x 64 ... 512 x 256), where the new call is timed on both of its paths: the
host / device threshold of the stage (fbk_group_select_plan.h, kHostCells) is read from these.  Each with sort="count desc" at limit 10 and limit 1000, with a having only (count above its 99.9th percentile),
and with offset / limit only.
Usage: python scripts/bench_groupby_select.py --out profiles [--only NAME] [--rounds 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("cube_256x256x256", "cube", (256, 256, 256)), ("matrix_4096x4096", "matrix", (4096, 4096)), ("sum_4096x4096", "sum", (4096, 4096)),
         ("matrix_64x64", "matrix", (64, 64)), ("matrix_65x64", "matrix", (65, 64)), ("matrix_128x128", "matrix", (128, 128)), ("matrix_256x128", "matrix", (256, 128)),
         ("matrix_256x256", "matrix", (256, 256)), ("matrix_512x256", "matrix", (512, 256)), ("sum_128x128", "sum", (128, 128)), ("sum_256x256", "sum", (256, 256))]
DEPTH = 8


def dense_batch(ctx, torch, rows, seed):
    """dense rows generated on the device (torch), handed to fbk_batch_upload_dense by device pointer"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-(1 << 62), 1 << 62, (rows, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
    torch.cuda.synchronize()
    b = ctx.upload_dense_device(t.data_ptr(), t.shape[0])
    torch.cuda.synchronize()
    del t
    return b


def stats(ts):
    us = np.array(ts, dtype=np.float64) * 1e6
    return {"median_us": round(float(np.median(us)), 1), "p10_us": round(float(np.percentile(us, 10)), 1), "p90_us": round(float(np.percentile(us, 90)), 1),
            "min_us": round(float(us.min()), 1), "max_us": round(float(us.max()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd.roaring import Context, GroupSelect

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for name, kind, shape in CASES:
        if a.only and name != a.only:
            continue
        batches = [dense_batch(ctx, torch, n, 31 + k) for k, n in enumerate(shape)]
        lists = [np.arange(n, dtype=np.uint32).reshape(1, n) for n in shape]
        bsi = dense_batch(ctx, torch, DEPTH + 2, 40) if kind == "sum" else None
        base = np.zeros(1, dtype=np.uint32)
        cells = int(np.prod(shape))
        if kind == "cube":
            full = lambda: (ctx.count_cube(batches[0], lists[0], batches[1], lists[1], batches[2], lists[2]).reshape(-1), None)
            new = lambda sel: ctx.count_cube_select(batches[0], lists[0], batches[1], lists[1], batches[2], lists[2], sel)
        elif kind == "matrix":
            full = lambda: (ctx.count_matrix(batches[0], lists[0], batches[1], lists[1]).reshape(-1), None)
            new = lambda sel: ctx.count_matrix_select(batches[0], lists[0], batches[1], lists[1], sel)
        else:
            def full():
                sums, counts = ctx.count_matrix_sum(batches[0], lists[0], batches[1], lists[1], bsi, base, DEPTH)
                return counts.reshape(-1), sums.reshape(-1)
            new = lambda sel: ctx.count_matrix_sum_select(batches[0], lists[0], batches[1], lists[1], bsi, base, DEPTH, sel)
        counts0, _ = full()
        thr = int(np.sort(counts0)[int(cells * 0.999)])
        selections = [("sort_count_desc_limit_10", dict(sort="count desc", limit=10)), ("sort_count_desc_limit_1000", dict(sort="count desc", limit=1000)),
                      ("having_only", dict(having=("count", ">", thr))), ("offset_limit_only", dict(offset=100, limit=1000))]
        paths = ["device", "host"] if cells <= (1 << 18) else [None]  # (around the threshold: the new call on both of its paths)
        for sname, spec in selections:
            t_new = {p: [] for p in paths}
            t_old, t_full, equal, n_out = [], [], True, 0
            for k in range(a.warmup + a.rounds):
                outs = []
                for p in paths:
                    t0 = time.perf_counter()
                    outs.append(new(GroupSelect(path=p, **spec)))
                    if k >= a.warmup:
                        t_new[p].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                c, s = full()
                t1 = time.perf_counter()
                old = ctx.select_groups(c, s, GroupSelect(path="host", **spec), cap=max(len(outs[0][0]), 1))
                t2 = time.perf_counter()
                for o in outs:
                    equal = equal and len(o) == len(old) and all(np.array_equal(x, y) for x, y in zip(o[:-1], old[:-1])) and o[-1] == old[-1]
                n_out = len(old[0])
                if k >= a.warmup:
                    t_old.append(t2 - t0)
                    t_full.append(t1 - t0)
            r = {"case": name, "selection": sname, "kind": kind, "shape": list(shape), "cells": cells, "shards": 1, "records": n_out, "matched": int(old[-1]),
                 "rounds": a.rounds, "warmup": a.warmup, "outputs_equal": equal, "replaced_path": stats(t_old), "of_which_full_call": stats(t_full)}
            for p in paths:
                r["select_call" + ("_" + p if p else "")] = stats(t_new[p])
            first = stats(t_new[paths[0]])
            r["speedup_median"] = round(r["replaced_path"]["median_us"] / first["median_us"], 2)
            print(json.dumps(r), flush=True)
            with open(os.path.join(a.out, f"groupby_select_{name}_{sname}.json"), "w") as f:
                json.dump(r, f, indent=1)
            ok = ok and equal
        for b in batches + ([bsi] if bsi is not None else []):
            b.free()
    ctx.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
