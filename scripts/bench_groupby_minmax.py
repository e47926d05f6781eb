"""GroupBy with Min / Max per group (fbk_count_matrix_minmax): timings for DESIGN.md §6, one JSON file per workload under --out.
Rows are generated on the device; the time is the library's own events around the kernels of a call (option time_kernels ->
last_kernel_ns), warm runs, median and p10 / p90.  Every workload compares the two kernel paths' outputs with each other.

  sweep  128 shards, mutex-like rows (every column in one A row and one B row), values on three quarters of the columns; 64, 128,
         256, 512 and 1024 groups as 8 x 8 ... 32 x 32; the descent and the scatter (with counts) pinned, alternating in one
         process; at depth 20 (what fixes kMinmaxDescentCells: the largest swept group count at which the descent's median is
         not above the scatter's), 8 and 63.
  W1     1024 shards, 8 x 8, depth 20, FBK_MINMAX_AUTO.
  W2     1024 shards, 256 x 256 mutex-like, FBK_MINMAX_AUTO (the scatter), with and without counts.
  old    128 shards, 8 x 8 and 32 x 32: the one call against the per-group composition it replaces (fbk_setop AND per pair, then
         fbk_bsi_min and fbk_bsi_max per group, folded over the shards on the host), wall time of both in the same process,
         outputs compared.
Usage: python scripts/bench_groupby_minmax.py --out profiles [--only sweep|W1|W2|old] [--runs 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BPS = 8.0e12
# vector instructions per second of the chip: 256 CUs x 4 SIMDs, a wave64 instruction every 4 cycles at about 2.4 GHz
WAVE_INSTR_PS = 256 * 4 * 2.4e9 / 4
AUTO, DESCENT, SCATTER = 0, 1, 2
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


def pack(torch, mask):
    """[n, 2^20] bool on the device -> [n, 16, 1024] int64 words, bit c of a row = mask[row, c]"""
    sh = torch.arange(64, dtype=torch.int64, device=mask.device)
    return (mask.view(mask.shape[0], 16384, 64).to(torch.int64) << sh).sum(-1).view(mask.shape[0], 16, 1024)


def mutex_batches(ctx, torch, n_sh, n_a, n_b, depth, seed):
    """every column of a shard in exactly one A row and one B row; a value on three quarters of the columns: a magnitude below
    2^depth, 40 % negative"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for n in (n_a, n_b):
        t = torch.empty((n_sh * n, 16, 1024), dtype=torch.int64, device="cuda")
        ids = torch.arange(n, device="cuda")[:, None]
        for s in range(n_sh):
            t[s * n:(s + 1) * n] = pack(torch, torch.randint(0, n, (1 << 20,), device="cuda", generator=g)[None, :] == ids)
        torch.cuda.synchronize()
        out.append(ctx.upload_dense_device(t.data_ptr(), t.shape[0]))
        torch.cuda.synchronize()
        del t
    S = torch.empty((n_sh * (depth + 2), 16, 1024), dtype=torch.int64, device="cuda")
    for s in range(n_sh):
        mag = torch.randint(0, 1 << min(depth, 62), (1 << 20,), device="cuda", generator=g)
        rows = [torch.rand(1 << 20, device="cuda", generator=g) < 0.75, torch.rand(1 << 20, device="cuda", generator=g) < 0.4]
        rows += [((mag >> k) & 1).bool() for k in range(depth)]
        S[s * (depth + 2):(s + 1) * (depth + 2)] = pack(torch, torch.stack(rows))
    torch.cuda.synchronize()
    out.append(ctx.upload_dense_device(S.data_ptr(), S.shape[0]))
    torch.cuda.synchronize()
    del S
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    return out, ra, rb, np.arange(n_sh, dtype=np.uint32) * (depth + 2)


def stats(ns):
    us = np.array(ns, dtype=np.float64) / 1e3
    return {"runs": len(ns), "median_us": round(float(np.median(us)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
            "p90_us": round(float(np.percentile(us, 90)), 1), "min_us": round(float(us.min()), 1), "max_us": round(float(us.max()), 1)}


def time_paths(ctx, args, depth, variants, runs):
    """variants: {name: (path, counts)}; the calls alternate, so that clocks and caches are shared fairly.  Returns
    ({name: stats}, {name: outputs})"""
    ns, out = {k: [] for k in variants}, {}
    ctx.set_option("time_kernels", 1)
    try:
        for r in range(3 + runs):
            for name, (path, counts) in variants.items():
                out[name] = ctx.count_matrix_minmax(*args, depth, counts=counts, path=path)
                if r >= 3:
                    ns[name].append(ctx.get_option("last_kernel_ns"))
    finally:
        ctx.set_option("time_kernels", 0)
    return {k: stats(v) for k, v in ns.items()}, out


def same(a, b, counts=True):
    return bool(all(np.array_equal(a[k], b[k]) for k in range(4 if counts else 2)))


def models(n_sh, n_a, n_b, depth):
    """the work terms of the two kernels (fbk_matrix_minmax.hip.h) as times"""
    tiles = -(-n_a * n_b // 64)
    words = n_sh * 16384
    d_bytes = (tiles * (n_a + n_b) + tiles * (depth + 2)) * 128 * 1024 * n_sh  # a tile's lanes read their rows; every tile the planes
    d_instr = tiles * words * (2 * depth * 10 + 40)                            # two scans of depth steps, ~10 vector instructions each
    s_bytes = (n_a + n_b + depth + 2) * 128 * 1024 * n_sh
    s_updates = n_sh * (1 << 20) * 0.75                                          # mutex-like: one group per column with a value
    return {"descent_algorithmic_bytes": d_bytes, "descent_hbm_bound_us": round(d_bytes / HBM_BPS * 1e6, 1), "descent_wave_instructions": d_instr,
            "descent_valu_bound_us": round(d_instr / WAVE_INSTR_PS * 1e6, 1), "scatter_algorithmic_bytes": s_bytes,
            "scatter_hbm_bound_us": round(s_bytes / HBM_BPS * 1e6, 1), "scatter_updates_per_walk": int(s_updates)}


def sweep(ctx, torch, runs):
    rows = []
    for depth in (20, 8, 63):
        for side in ((8, 8), (8, 16), (16, 16), (16, 32), (32, 32)):
            n_sh, (n_a, n_b) = 128, side
            (bA, bB, bS), ra, rb, base = mutex_batches(ctx, torch, n_sh, n_a, n_b, depth, 100 + depth)
            t, out = time_paths(ctx, (bA, ra, bB, rb, bS, base), depth, {"descent": (DESCENT, True), "scatter": (SCATTER, True)}, runs)
            rows.append({"shards": n_sh, "n_a": n_a, "n_b": n_b, "groups": n_a * n_b, "depth": depth, "descent": t["descent"], "scatter_with_counts": t["scatter"],
                         "descent_not_slower": t["descent"]["median_us"] <= t["scatter"]["median_us"], "outputs_equal": same(out["descent"], out["scatter"]),
                         **models(n_sh, n_a, n_b, depth)})
            print(json.dumps(rows[-1]), flush=True)
            for b in (bA, bB, bS):
                b.free()
    wins = [r["groups"] for r in rows if r["depth"] == 20 and r["descent_not_slower"]]
    return {"workload": "sweep", "rows": rows, "kMinmaxDescentCells_from_sweep": max(wins) if wins else 64, "outputs_equal": all(r["outputs_equal"] for r in rows)}


def w1(ctx, torch, runs):
    n_sh, n_a, n_b, depth = 1024, 8, 8, 20
    (bA, bB, bS), ra, rb, base = mutex_batches(ctx, torch, n_sh, n_a, n_b, depth, 21)
    t, out = time_paths(ctx, (bA, ra, bB, rb, bS, base), depth, {"auto": (AUTO, True), "scatter": (SCATTER, True)}, runs)
    for b in (bA, bB, bS):
        b.free()
    return {"workload": "W1", "shards": n_sh, "n_a": n_a, "n_b": n_b, "depth": depth, "auto": t["auto"], "scatter_pinned": t["scatter"],
            "outputs_equal": same(out["auto"], out["scatter"]), **models(n_sh, n_a, n_b, depth)}


def w2(ctx, torch, runs):
    n_sh, n_a, n_b, depth = 1024, 256, 256, 20
    (bA, bB, bS), ra, rb, base = mutex_batches(ctx, torch, n_sh, n_a, n_b, depth, 22)
    t, out = time_paths(ctx, (bA, ra, bB, rb, bS, base), depth, {"auto_counts": (AUTO, True), "auto_no_counts": (AUTO, False), "scatter": (SCATTER, True)}, runs)
    for b in (bA, bB, bS):
        b.free()
    return {"workload": "W2", "shards": n_sh, "n_a": n_a, "n_b": n_b, "depth": depth, "auto_with_counts": t["auto_counts"], "auto_without_counts": t["auto_no_counts"],
            "outputs_equal": same(out["auto_counts"], out["scatter"]) and same(out["auto_counts"], out["auto_no_counts"], counts=False),
            "groups_non_empty": int((out["auto_counts"][2] > 0).sum()), **models(n_sh, n_a, n_b, depth)}


def old_path(ctx, torch, runs):
    from featurebase_amd import lib as L

    res = []
    for n_a, n_b in ((8, 8), (32, 32)):
        n_sh, depth = 128, 20
        (bA, bB, bS), ra, rb, base = mutex_batches(ctx, torch, n_sh, n_a, n_b, depth, 31)
        new_t = []
        for _ in range(5):
            t0 = time.perf_counter()
            new = ctx.count_matrix_minmax(bA, ra, bB, rb, bS, base, depth)
            new_t.append(time.perf_counter() - t0)
        # the composition: AND of the two rows per pair, fbk_bsi_min and fbk_bsi_max over it per shard, ValCount.Smaller / Larger
        t0 = time.perf_counter()
        old = (np.full((n_a, n_b), INT64_MAX, np.int64), np.full((n_a, n_b), INT64_MIN, np.int64), np.zeros((n_a, n_b), np.uint64), np.zeros((n_a, n_b), np.uint64))
        idx = np.arange(n_sh)
        for i in range(n_a):
            for j in range(n_b):
                m, _ = ctx.setop(L.OP_AND, bA, ra[:, i], bB, rb[:, j])
                vmin, cmin = ctx.bsi_min(bS, base, depth, m, idx)
                vmax, cmax = ctx.bsi_max(bS, base, depth, m, idx)
                m.free()
                if (cmin > 0).any():
                    lo, hi = vmin[cmin > 0].min(), vmax[cmax > 0].max()
                    old[0][i, j], old[1][i, j] = lo, hi
                    old[2][i, j], old[3][i, j] = cmin[(cmin > 0) & (vmin == lo)].sum(), cmax[(cmax > 0) & (vmax == hi)].sum()
        old_s = time.perf_counter() - t0
        for b in (bA, bB, bS):
            b.free()
        res.append({"n_a": n_a, "n_b": n_b, "one_call_ms": round(float(np.median(new_t)) * 1e3, 2), "one_call_min_ms": round(min(new_t) * 1e3, 2),
                    "composition_ms": round(old_s * 1e3, 1), "speedup": round(old_s / float(np.median(new_t)), 1), "composition_calls": n_a * n_b * 3,
                    "outputs_equal": same(new, old)})
        print(json.dumps(res[-1]), flush=True)
    return {"workload": "old_path", "shards": 128, "depth": 20, "shapes": res, "outputs_equal": all(r["outputs_equal"] for r in res)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--tag", default="groupby_minmax")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for name, fn in (("sweep", sweep), ("W1", w1), ("W2", w2), ("old", old_path)):
        if a.only and name != a.only:
            continue
        r = fn(ctx, torch, a.runs)
        print(json.dumps({k: v for k, v in r.items() if k != "rows"}), flush=True)
        with open(os.path.join(a.out, f"{a.tag}_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
        ok = ok and r["outputs_equal"]
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
