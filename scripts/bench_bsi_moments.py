"""fbk_bsi_moments (SQL VAR / CORR in one pass) against what a caller did before it: timings for
docs/history/DESIGN_moments_measurements.md, one JSON file per case under --out.

  old  fbk_extract_open over the filter, fbk_extract_bsi for each field (16 bytes per selected column and field back to the
       host), the six sums in numpy (int64, i.e. modulo 2^64); the shards in windows of 128 so that the host arrays stay small
  new  fbk_bsi_moments: the call's wall time (it ends in its one synchronisation) and its kernels' time by the library's own
       events (option time_kernels -> last_kernel_ns)
Old and new alternate in one process on the same seeded dense batches; the outputs are compared modulo 2^64 in the same run.
Cases: 64 and 1024 shards; depths (20, 20), (32, 32), (64, 64) and the one-field form at 20; a dense filter of about half the
columns, exists_x and exists_y about three quarters each.  The old path at 1024 shards moves ~10 GB per field: it runs once
there, and only for the depth-20 cases.
Usage: python scripts/bench_bsi_moments.py --out profiles [--shards 64,1024] [--runs 30] [--cases 20x20,64x64] [--no-old] [--tag T]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12  # spec peak of the MI355X
WINDOW = 128
CASES = [(20, 20), (32, 32), (64, 64), (20, None)]


def dense_field(ctx, torch, g, n_sh, depth):
    t = torch.randint(-(1 << 62), 1 << 62, (n_sh, depth + 2, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
    t[:, 0] |= torch.randint(-(1 << 62), 1 << 62, (n_sh, 16, 1024), dtype=torch.int64, device="cuda", generator=g)  # exists: ~3/4
    torch.cuda.synchronize()
    b = ctx.upload_dense_device(t.data_ptr(), n_sh * (depth + 2))
    torch.cuda.synchronize()
    del t
    return b, np.arange(n_sh, dtype=np.uint32) * (depth + 2)


def old_path(ctx, bx, rx, dx, by, ry, dy, bf, rf):
    """(n, Σx, Σy, Σx², Σy², Σxy) modulo 2^64, as a caller computed them before fbk_bsi_moments"""
    acc = np.zeros(6, dtype=np.uint64)
    n_sh = rf.size
    for s0 in range(0, n_sh, WINDOW):
        w = slice(s0, min(n_sh, s0 + WINDOW))
        with ctx.extract(bf, rf[w], np.arange(s0, w.stop, dtype=np.uint64)) as ex:
            x, px = ex.bsi(bx, rx[w], dx)
            if by is not None:
                y, py = ex.bsi(by, ry[w], dy)
                keep = px & py
                x, y = x[keep], y[keep]
            else:
                x = x[px]
        with np.errstate(over="ignore"):
            part = [x.size, x.sum(), 0, np.dot(x, x), 0, 0]
            if by is not None:
                part[2], part[4], part[5] = y.sum(), np.dot(y, y), np.dot(x, y)
        acc += np.array([int(v) & ((1 << 64) - 1) for v in part], dtype=np.uint64)
    return [int(v) for v in acc]


def stats(us):
    us = np.asarray(us, dtype=np.float64)
    return {"runs": int(us.size), "median_us": round(float(np.median(us)), 1), "min_us": round(float(us.min()), 1), "max_us": round(float(us.max()), 1)}


def run_case(ctx, torch, n_sh, dx, dy, runs, old_rounds):
    g = torch.Generator(device="cuda").manual_seed(1000 * n_sh + 10 * dx + (dy or 0))
    bx, rx = dense_field(ctx, torch, g, n_sh, dx)
    by, ry = dense_field(ctx, torch, g, n_sh, dy) if dy is not None else (None, None)
    f = torch.randint(-(1 << 62), 1 << 62, (n_sh, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
    torch.cuda.synchronize()
    bf = ctx.upload_dense_device(f.data_ptr(), n_sh)
    torch.cuda.synchronize()
    del f
    rf = np.arange(n_sh, dtype=np.uint32)
    call = lambda: ctx.bsi_moments(bx, rx, dx, by, ry, dy or 0, bf, rf)
    for _ in range(3):
        m = call()
    wall, kern, old_ms, equal = [], [], [], None
    ctx.set_option("time_kernels", 1)
    try:
        rounds = max(old_rounds, 1)
        for r in range(rounds):  # old and new alternating
            if r < old_rounds:
                t0 = time.perf_counter()
                o = old_path(ctx, bx, rx, dx, by, ry, dy, bf, rf)
                old_ms.append((time.perf_counter() - t0) * 1e3)
                mask = (1 << 64) - 1
                equal = o == [m.n & mask, m.sum_x & mask, m.sum_y & mask, m.sum_xx & mask, m.sum_yy & mask, m.sum_xy & mask]
            for _ in range(-(-runs // rounds)):
                t0 = time.perf_counter()
                m2 = call()
                wall.append((time.perf_counter() - t0) * 1e6)
                kern.append(ctx.get_option("last_kernel_ns") / 1e3)
                assert m2 == m
    finally:
        ctx.set_option("time_kernels", 0)
    rows = dx + (dy + 2 if dy is not None else 0) + 3
    nbytes = rows * (1 << 17) * n_sh
    k = stats(kern)
    res = {"shards": n_sh, "depth_x": dx, "depth_y": dy, "filter": "dense, about half the columns", "selected_columns": m.n,
           "new_call_wall": stats(wall), "new_kernels": k, "plane_bytes_read_once": nbytes,
           "achieved_bytes_per_s": round(nbytes / (k["median_us"] * 1e-6)), "hbm_bound_us": round(nbytes / HBM_BPS * 1e6, 1),
           "fraction_of_hbm_bound": round(nbytes / HBM_BPS * 1e6 / k["median_us"], 3),
           "old_path_ms": [round(v, 1) for v in old_ms] or "not run", "outputs_equal_mod_2_64": equal}
    if old_ms:
        res["speedup_wall"] = round(min(old_ms) * 1e3 / res["new_call_wall"]["median_us"], 1)
    for b in (bx, by, bf):
        if b is not None:
            b.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--shards", default="64,1024")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--tag", default="bsi_moments")
    ap.add_argument("--cases", default="", help="e.g. 20x20,64x64,20xnone: only these depth pairs")
    ap.add_argument("--no-old", action="store_true", help="the new call only (A/B of two library builds: FBK_LIB_PATH, runs alternating)")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for n_sh in [int(s) for s in a.shards.split(",")]:
        for dx, dy in CASES:
            if a.cases and f"{dx}x{dy if dy is not None else 'none'}" not in a.cases.split(","):
                continue
            old_rounds = 0 if a.no_old else 3 if n_sh <= 128 else (1 if dx <= 20 else 0)
            r = run_case(ctx, torch, n_sh, dx, dy, a.runs, old_rounds)
            print(json.dumps(r), flush=True)
            name = f"{a.tag}_{n_sh}sh_{dx}x{dy if dy is not None else 'none'}.json"
            with open(os.path.join(a.out, name), "w") as f:
                json.dump(r, f, indent=1)
            ok = ok and r["outputs_equal_mod_2_64"] is not False
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
