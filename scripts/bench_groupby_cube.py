"""GroupBy over three fields (fbk_count_cube): the one-call form against the path it replaces, for DESIGN.md §6; one JSON file per
case under --out.

The parent path is Executor::group_by_rec's loop before this call existed, with the same library: per row of the leading field one
fbk_setop(AND) that materialises filter ∩ row (FBK_SETOP_OPTIMIZE, as the mirror asks for), one fbk_count over it, one
fbk_count_matrix with that row as the filter, and the download.  The two forms alternate in one process (a round = one run of
each, after --warmup rounds), both timed by the host clock around calls that end in a device synchronise, and their outputs are
compared.  Acceptance: p90 of the one-call form below p10 of the parent path wherever n_p >= 2.

Cases: the reference benchmark's 4 x 4 x 4 rows on 1 shard; 8 x 32 x 32 and 32 x 32 x 32 dense rows on 64 and 1024 shards;
4 x 32 x 32 on 1024 shards (the 4-row form of the kernel: twice its time is what 8 rows would cost in blocks of 4); 8 x 32 x 32
on config 3's mixed rows (tests/datagen.py config3_flat: P = rows 0..7, A = rows 0..31, B = rows 32..63, its filter).
Usage: python scripts/bench_groupby_cube.py --out profiles [--only NAME] [--rounds 20]"""
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
I8_MACS = 2.5e15  # i8 matrix-core peak of the MI355X, dense: about 5 POPS = 2.5e15 multiply-adds per second

DENSE = [("ref_4x4x4_1", 4, 4, 4, 1), ("8x32x32_64", 8, 32, 32, 64), ("32x32x32_64", 32, 32, 32, 64), ("8x32x32_1024", 8, 32, 32, 1024),
         ("32x32x32_1024", 32, 32, 32, 1024), ("4x32x32_1024", 4, 32, 32, 1024)]


def dense_batches(ctx, torch, n_sh, ns, seed):
    """dense rows generated on the device (torch), handed to fbk_batch_upload_dense by device pointer"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for n in ns:
        t = torch.randint(-(1 << 62), 1 << 62, (n_sh * n, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
        torch.cuda.synchronize()
        out.append(ctx.upload_dense_device(t.data_ptr(), t.shape[0]))
        torch.cuda.synchronize()
        del t
    return out


def parent_path(ctx, L, bP, rp, bA, ra, bB, rb, bF, rf):
    n_sh, n_p = rp.shape
    ids = np.arange(n_sh, dtype=np.uint32)
    out = np.zeros((n_p, ra.shape[1], rb.shape[1]), dtype=np.uint64)
    for p in range(n_p):
        pf, _ = ctx.setop(L.OP_AND, bP, rp[:, p], bF, rf, flags=L.SETOP_OPTIMIZE)
        try:
            if int(pf.count(ids).sum()):
                out[p] = ctx.count_matrix(bA, ra, bB, rb, pf, ids)
        finally:
            pf.free()
    return out


def stats(ts):
    us = np.array(ts, dtype=np.float64) * 1e6
    return {"median_us": round(float(np.median(us)), 1), "p10_us": round(float(np.percentile(us, 10)), 1), "p90_us": round(float(np.percentile(us, 90)), 1),
            "min_us": round(float(us.min()), 1), "max_us": round(float(us.max()), 1)}


def run_case(ctx, L, name, batches, lists, rounds, warmup, extra):
    bP, bA, bB, bF = batches
    rp, ra, rb, rf = lists
    new_t, old_t, equal = [], [], True
    for k in range(warmup + rounds):
        t0 = time.perf_counter()
        cube = ctx.count_cube(bP, rp, bA, ra, bB, rb, bF, rf)
        t1 = time.perf_counter()
        old = parent_path(ctx, L, bP, rp, bA, ra, bB, rb, bF, rf)
        t2 = time.perf_counter()
        equal = equal and bool(np.array_equal(cube, old))
        if k >= warmup:
            new_t.append(t1 - t0)
            old_t.append(t2 - t1)
    n_sh, n_p = rp.shape
    n_a, n_b = ra.shape[1], rb.shape[1]
    pt = 4 if n_p <= 4 else 8
    nbytes = (n_p + n_a + n_b + 1) * 128 * 1024 * n_sh
    macs = 32 * 32 * (1 << 20) * n_sh * pt * (-(-n_p // pt)) * (-(-n_a // 32)) * (-(-n_b // 32))
    new, old = stats(new_t), stats(old_t)
    return {"case": name, "shards": n_sh, "n_p": n_p, "n_a": n_a, "n_b": n_b, "filter": True, "rounds": rounds, "warmup": warmup, "outputs_equal": equal,
            "one_call": new, "parent_path": old, "parent_calls": 3 * n_p, "speedup_median": round(old["median_us"] / new["median_us"], 2),
            "accepted": bool(n_p < 2 or new["p90_us"] < old["p10_us"]), "p_rows_per_block": pt, "algorithmic_bytes": nbytes,
            "hbm_bound_us": round(nbytes / HBM_BPS * 1e6, 1), "i8_mfma_bound_us": round(macs / I8_MACS * 1e6, 1), **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config3-shards", type=int, default=256)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    ok = True

    def emit(r):
        nonlocal ok
        print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, f"groupby_cube_{r['case']}.json"), "w") as f:
            json.dump(r, f, indent=1)
        ok = ok and r["outputs_equal"]

    for name, n_p, n_a, n_b, n_sh in DENSE:
        if a.only and name != a.only:
            continue
        batches = dense_batches(ctx, torch, n_sh, (n_p, n_a, n_b, 1), 21)
        lists = [np.arange(n_sh * n, dtype=np.uint32).reshape(n_sh, n) for n in (n_p, n_a, n_b)] + [np.arange(n_sh, dtype=np.uint32)]
        emit(run_case(ctx, L, name, batches, lists, a.rounds, a.warmup, {"layout": "dense"}))
        for b in batches:
            b.free()
    if not a.only or a.only == "config3":
        import cube_ref as R
        import datagen as D

        n_sh = a.config3_shards
        d, p, nr, groups, fd, fp, enc = D.config3_flat_subprocess(n_sh)
        batch, F = ctx.upload_flat(d, p, nr), ctx.upload_flat(fd, fp, n_sh)
        f_dense = len(fd) == n_sh * 16 and bool((fd["type"] == 2).all()) and bool((fd["off"] == (fd["row"].astype(np.uint64) * 16 + (fd["key"] & 15)) * 8192).all())
        groups = np.ascontiguousarray(groups, dtype=np.uint32)
        lists = [np.ascontiguousarray(groups[:, :8]), np.ascontiguousarray(groups[:, :32]), np.ascontiguousarray(groups[:, 32:]), np.arange(n_sh, dtype=np.uint32)]
        extra = {"layout": "config 3 mixed rows", "encoded_bytes_rows": int(enc), "filter_dense": f_dense,
                 "densify_chunk_shards": R.chunk(n_sh, 8, 32, 32, False, False, False, f_dense)}
        emit(run_case(ctx, L, f"8x32x32_config3_{n_sh}", (batch, batch, batch, F), lists, a.rounds, a.warmup, extra))
        batch.free()
        F.free()
    ctx.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
