"""fbk_bsi_compare (the Row of SQL WHERE x < y over two int fields): timings for docs/history/DESIGN_compare_measurements.md, one
JSON file per workload under --out.

  (a) against the composition it replaces: fbk_extract_open over every column, fbk_extract_bsi for each field (16 bytes per column
      and field back to the host), the comparison in numpy, upload_dense of the row; the shards in windows of 32
  (b) against fbk_bsi_range on a field that has as many rows per shard (depth_x + depth_y + 2, at most 64: above that the field of
      depth 64 and bytes per second instead of time): the yardstick for achieved bytes/s
  (c) the two kernel instances against each other at base_x == base_y: the default (sign-magnitude) and FBK_COMPARE_PATH_OFFSET
      (general); the run-to-run spread of each is in the JSON (min / median / max)
The calls alternate in one process on the same seeded dense batches; outputs are compared before anything is timed.  Kernel times
are the library's own events (option time_kernels -> last_kernel_ns), wall times end in the call's synchronisation.
Usage: python scripts/bench_bsi_compare.py --out profiles [--shards 256] [--runs 30] [--cases 20x20,63x63] [--no-old] [--tag T]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12  # spec peak of the MI355X
WINDOW = 32
CASES = [(20, 20), (63, 63)]
ROW_BYTES = 1 << 17


def dense_field(ctx, torch, g, n_sh, depth):
    t = torch.randint(-(1 << 62), 1 << 62, (n_sh, depth + 2, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
    t[:, 0] |= torch.randint(-(1 << 62), 1 << 62, (n_sh, 16, 1024), dtype=torch.int64, device="cuda", generator=g)  # exists: ~3/4
    torch.cuda.synchronize()
    b = ctx.upload_dense_device(t.data_ptr(), n_sh * (depth + 2))
    torch.cuda.synchronize()
    del t
    return b, np.arange(n_sh, dtype=np.uint32) * (depth + 2)


def words_of(batch, n_sh):
    w = np.zeros((n_sh, 16, 1024), dtype=np.uint64)
    for s, row in enumerate(batch.download()):
        for k, c in row.items():
            w[s, k & 15] = c.words()
    return w


def old_path(ctx, L, ball, bx, rx, dx, by, ry, dy, op):
    """the row of value_x op value_y as a caller built it before fbk_bsi_compare -> (batch, seconds)"""
    n_sh = rx.size
    t0 = time.perf_counter()
    out = np.zeros((n_sh, 16, 1024), dtype=np.uint64)
    cmp = {L.BSI_LT: np.less, L.BSI_LTE: np.less_equal, L.BSI_GT: np.greater, L.BSI_GTE: np.greater_equal, L.BSI_EQ: np.equal, L.BSI_NEQ: np.not_equal}[op]
    for s0 in range(0, n_sh, WINDOW):
        s1 = min(n_sh, s0 + WINDOW)
        with ctx.extract(ball, np.zeros(s1 - s0, dtype=np.uint32), np.arange(s0, s1, dtype=np.uint64)) as ex:
            x, px = ex.bsi(bx, rx[s0:s1], dx)
            y, py = ex.bsi(by, ry[s0:s1], dy)
        bits = px & py & cmp(x, y)  # every column of the window, ascending: the row's bits in order
        out[s0:s1] = np.packbits(bits, bitorder="little").view(np.uint64).reshape(s1 - s0, 16, 1024)
    b = ctx.upload_dense(out.reshape(-1))
    return b, out, time.perf_counter() - t0


def stats(us):
    us = np.asarray(us, dtype=np.float64)
    return {"runs": int(us.size), "median_us": round(float(np.median(us)), 1), "min_us": round(float(us.min()), 1), "max_us": round(float(us.max()), 1)}


def rate(nbytes, st):
    return {"bytes": int(nbytes), "achieved_bytes_per_s": round(nbytes / (st["median_us"] * 1e-6)), "hbm_bound_us": round(nbytes / HBM_BPS * 1e6, 1),
            "fraction_of_hbm_bound": round(nbytes / HBM_BPS * 1e6 / st["median_us"], 3)}


def run_case(ctx, L, torch, n_sh, dx, dy, runs, with_old):
    g = torch.Generator(device="cuda").manual_seed(7000 * n_sh + 10 * dx + dy)
    bx, rx = dense_field(ctx, torch, g, n_sh, dx)
    by, ry = dense_field(ctx, torch, g, n_sh, dy)
    dr = min(dx + dy + 2, 64)
    br, rr = dense_field(ctx, torch, g, n_sh, dr)
    op = L.BSI_LT
    pred = (1 << (dr - 1)) // 3  # a predicate with mixed bits: the range scan reads every plane
    calls = {
        "compare": lambda: ctx.bsi_compare(bx, rx, dx, 0, by, ry, dy, 0, op),
        "compare_pinned_general": lambda: ctx.bsi_compare(bx, rx, dx, 0, by, ry, dy, 0, op, flags=L.COMPARE_PATH_OFFSET),
        "compare_offset_1": lambda: ctx.bsi_compare(bx, rx, dx, 1, by, ry, dy, 0, op),
        "compare_count_only": lambda: ctx.bsi_compare(bx, rx, dx, 0, by, ry, dy, 0, op, count_only=True),
        "range": lambda: ctx.bsi_range(br, rr, op, dr, pred),
    }
    # outputs before timing: the two instances agree bit for bit, the count-only form counts the same
    o1, c1 = calls["compare"]()
    o2, c2 = calls["compare_pinned_general"]()
    w1 = words_of(o1, n_sh)
    instances_equal = bool((w1 == words_of(o2, n_sh)).all() and (c1 == c2).all() and (calls["compare_count_only"]()[1] == c1).all())
    o1.free()
    o2.free()
    old_equal, old_s = None, None
    if with_old:
        ball = ctx.upload_dense(np.full(16 * 1024, np.uint64(0xFFFFFFFFFFFFFFFF)))
        bo, wo, old_s = old_path(ctx, L, ball, bx, rx, dx, by, ry, dy, op)
        old_equal = bool((wo == w1).all())
        bo.free()
        ball.free()
    del w1
    wall = {k: [] for k in calls}
    kern = {k: [] for k in calls}
    ctx.set_option("time_kernels", 1)
    try:
        for _ in range(3):
            for k, f in calls.items():
                out = f()[0]
                if out is not None:
                    out.free()
        for _ in range(runs):  # alternating
            for k, f in calls.items():
                t0 = time.perf_counter()
                out = f()[0]
                wall[k].append((time.perf_counter() - t0) * 1e6)
                kern[k].append(ctx.get_option("last_kernel_ns") / 1e3)
                if out is not None:
                    out.free()
    finally:
        ctx.set_option("time_kernels", 0)
    read_cmp = (dx + dy + 4) * ROW_BYTES * n_sh
    read_rng = (dr + 2) * ROW_BYTES * n_sh
    written = ROW_BYTES * n_sh
    res = {"shards": n_sh, "depth_x": dx, "depth_y": dy, "op": "LT", "selected_columns": int(c1.sum()), "instances_equal": instances_equal,
           "range_depth": dr, "range_predicate": pred}
    for k in calls:
        ks = stats(kern[k])
        nbytes = (read_rng if k == "range" else read_cmp) + (0 if k == "compare_count_only" else written)
        res[k] = {"kernel": ks, "call_wall": stats(wall[k]), **rate(nbytes, ks)}
    res["compare_vs_range_bytes_per_s"] = round(res["compare"]["achieved_bytes_per_s"] / res["range"]["achieved_bytes_per_s"], 3)
    res["pinned_general_over_default_kernel_time"] = round(res["compare_pinned_general"]["kernel"]["median_us"] / res["compare"]["kernel"]["median_us"], 3)
    if with_old:
        res["old_path_s"] = round(old_s, 2)
        res["old_path_equal"] = old_equal
        res["speedup_wall_over_old_path"] = round(old_s * 1e6 / res["compare"]["call_wall"]["median_us"], 1)
    for b in (bx, by, br):
        b.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--shards", type=int, default=256)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--tag", default="bsi_compare")
    ap.add_argument("--cases", default="", help="e.g. 20x20,63x63: only these depth pairs")
    ap.add_argument("--no-old", action="store_true", help="skip (a), the extract-and-compare composition")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for dx, dy in CASES:
        if a.cases and f"{dx}x{dy}" not in a.cases.split(","):
            continue
        r = run_case(ctx, L, torch, a.shards, dx, dy, a.runs, not a.no_old)
        print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, f"{a.tag}_{a.shards}sh_{dx}x{dy}.json"), "w") as f:
            json.dump(r, f, indent=1)
        ok = ok and r["instances_equal"] and r.get("old_path_equal") is not False
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
