"""GroupBy with aggregate=Sum (fbk_count_matrix_sum): timings for DESIGN.md §6, one JSON file per workload under --out.

  W1  1024 shards, 32 x 32 dense rows + a dense filter, a dense depth-20 BSI field: the prepared query's run, timed by the
      library's own events (option time_kernels -> last_kernel_ns) over --runs warm runs; algorithmic bytes, the fractions of
      the HBM bound (8 TB/s) and of the i8 matrix-core bound (4 products of 32 x 32 x 2^20 per shard).
  W2  the same shape on config 3's mixed rows (tests/datagen.py config3_flat: A = rows 0..31, B = rows 32..63, its filter) and
      a BSI field built as optimize() encodes it (values on a third of the columns): the densify + matrix run, scratch bytes.
  old 128 shards, 32 x 32 dense: the one-shot call against the per-group path it replaces (fbk_setop AND per pair + fbk_bsi_sum
      per group), outputs compared in the same run.
Usage: python scripts/bench_groupby_sum.py --out profiles [--only W1|W2|old] [--runs 50]"""
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
# i8 matrix-core peak of the MI355X, dense: about 5 POPS = 2.5e15 multiply-adds per second
I8_MACS = 2.5e15


def dense_batches(ctx, torch, n_sh, n_a, n_b, depth, seed):
    """dense rows generated on the device (torch), handed to fbk_batch_upload_dense by device pointer"""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rows(n, p_half_ands=0):
        t = torch.randint(-(1 << 62), 1 << 62, (n, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
        for _ in range(p_half_ands):
            t &= torch.randint(-(1 << 62), 1 << 62, (n, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
        return t

    A, Bt, F = rows(n_sh * n_a), rows(n_sh * n_b), rows(n_sh)
    S = rows(n_sh * (depth + 2))
    S.view(n_sh, depth + 2, 16, 1024)[:, 0] &= rows(n_sh).view(n_sh, 16, 1024)  # exists on about a quarter of the columns
    torch.cuda.synchronize()
    out = [ctx.upload_dense_device(t.data_ptr(), t.shape[0]) for t in (A, Bt, F, S)]
    torch.cuda.synchronize()
    del A, Bt, F, S
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    return out, ra, rb, np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint32) * (depth + 2)


def time_query(ctx, q, runs):
    ctx.set_option("time_kernels", 1)
    try:
        for _ in range(3):
            q.run()
        q.read()
        ns = []
        for _ in range(runs):
            q.run()
            q.read()
            ns.append(ctx.get_option("last_kernel_ns"))
    finally:
        ctx.set_option("time_kernels", 0)
    us = np.array(ns, dtype=np.float64) / 1e3
    return {"runs": runs, "median_us": round(float(np.median(us)), 1), "min_us": round(float(us.min()), 1), "max_us": round(float(us.max()), 1),
            "p10_us": round(float(np.percentile(us, 10)), 1), "p90_us": round(float(np.percentile(us, 90)), 1)}


def bounds(n_sh, n_a, n_b, depth, filt, us):
    rows = n_a + n_b + (1 if filt else 0) + depth + 2
    nbytes = rows * 128 * 1024 * n_sh
    chunks = -(-depth // 7)
    chunk_bytes = 2 * chunks * (1 << 20) * n_sh  # written by the transpose, read by the matrix kernel
    macs = (chunks + 1) * 32 * 32 * (1 << 20) * n_sh * (-(-n_a // 32)) * (-(-n_b // 32))
    hbm_us, mfma_us = nbytes / HBM_BPS * 1e6, macs / I8_MACS * 1e6
    return {"algorithmic_bytes": nbytes, "chunk_scratch_traffic_bytes": chunk_bytes, "hbm_bound_us": round(hbm_us, 1), "i8_mfma_bound_us": round(mfma_us, 1),
            "fraction_of_hbm_bound": round(hbm_us / us, 3), "fraction_of_mfma_bound": round(mfma_us / us, 3),
            "larger_bound": "hbm" if hbm_us >= mfma_us else "matrix cores"}  # which bound is larger, not what the run is limited by


def w1(ctx, torch, runs):
    n_sh, n_a, n_b, depth = 1024, 32, 32, 20
    (bA, bB, bF, bS), ra, rb, rf, base = dense_batches(ctx, torch, n_sh, n_a, n_b, depth, 11)
    q = ctx.query_count_matrix_sum(bA, ra, bB, rb, bS, base, depth, bF, rf)
    t = time_query(ctx, q, runs)
    res = {"workload": "W1", "shards": n_sh, "n_a": n_a, "n_b": n_b, "depth": depth, "filter": True, "layout": "dense", **t,
           **bounds(n_sh, n_a, n_b, depth, True, t["median_us"])}
    q.free()
    for b in (bA, bB, bF, bS):
        b.free()
    return res


def bsi_flat(D, n_frag, depth, seed):
    """n_frag BSI fragments as optimize() encodes them: values on about a third of the columns, magnitudes < 2^depth, 40 %
    negative"""
    rows = D.FlatRows()
    rng = D.rng_for(seed)
    for f in range(n_frag):
        r0 = f * (depth + 2)
        for sl in range(16):
            cols = D.vals_density(rng, 0.3) if sl % 4 else D.vals_runs(rng, 64, 0.5)
            mag = rng.integers(0, 1 << depth, cols.size, dtype=np.int64)
            neg = rng.random(cols.size) < 0.4
            rows.add_vals(r0, r0 * 16 + sl, cols)
            rows.add_vals(r0 + 1, (r0 + 1) * 16 + sl, cols[neg])
            for k in range(depth):
                rows.add_vals(r0 + 2 + k, (r0 + 2 + k) * 16 + sl, cols[((mag >> k) & 1) == 1])
    rows.n_rows = n_frag * (depth + 2)
    return rows


def w2(ctx, torch, runs):
    import datagen as D

    n_sh, depth, n_frag = 1024, 20, 128
    d, p, nr, groups, fd, fp, enc = D.config3_flat_subprocess(n_sh)
    batch, F = ctx.upload_flat(d, p, nr), ctx.upload_flat(fd, fp, n_sh)
    bs = bsi_flat(D, n_frag, depth, 9100)
    S = ctx.upload_flat(bs.descs(), bs.payload(), bs.n_rows)
    base = (np.arange(n_sh, dtype=np.uint32) % n_frag) * (depth + 2)  # 128 distinct fragments, each read by 8 shards
    rf = np.arange(n_sh, dtype=np.uint32)
    q = ctx.query_count_matrix_sum(batch, groups[:, :32], batch, groups[:, 32:], S, base, depth, F, rf)
    t = time_query(ctx, q, runs)
    # a batch is dense when every row holds 16 bitmap containers at (row * 16 + slot) * 8192 (fbk_batch_upload): config 3's
    # filter (density 0.5) is; the rows and the BSI are not, so A, B and the BSI rows are densified
    f_dense = len(fd) == n_sh * 16 and bool((fd["type"] == 2).all()) and bool((fd["off"] == (fd["row"].astype(np.uint64) * 16 + (fd["key"] & 15)) * 8192).all())
    per_shard = -(-depth // 7) * (1 << 20) + 16 * 32 * 32 + (1 << 17) * (32 + 32 + (0 if f_dense else 1) + depth + 2)
    most = max(1, min(n_sh, (1 << 30) // per_shard))
    chunk = -(-n_sh // -(-n_sh // most))  # the shards dealt evenly over the fewest chunks (include/fbk.h)
    res = {"workload": "W2", "shards": n_sh, "n_a": 32, "n_b": 32, "depth": depth, "filter": True, "layout": "config 3 mixed rows + optimize()d BSI",
           "bsi_fragments_distinct": n_frag, "encoded_bytes_rows": int(enc), "encoded_bytes_bsi": int(bs.bytes), "filter_dense": f_dense, "densify_chunk_shards": chunk,
           "scratch_bytes": chunk * per_shard, **t, "note": "median_us covers densify + chunk pass + matrix kernel; the per-kernel split: rocprofv3 --kernel-trace --stats of this workload (profiles/groupby_sum_W2_kernel_trace_stats.txt)"}
    q.free()
    for b in (batch, F, S):
        b.free()
    return res


def old_path(ctx, torch, runs):
    from featurebase_amd import lib as L

    n_sh, n_a, n_b, depth = 128, 32, 32, 20
    (bA, bB, bF, bS), ra, rb, rf, base = dense_batches(ctx, torch, n_sh, n_a, n_b, depth, 12)
    new_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        sums, counts = ctx.count_matrix_sum(bA, ra, bB, rb, bS, base, depth, bF, rf)
        new_t.append(time.perf_counter() - t0)
    # the per-group path of the executor before this change: AND of the two rows (and the filter) per pair, fbk_bsi_sum over it
    t0 = time.perf_counter()
    osum = np.zeros((n_a, n_b), dtype=np.int64)
    ocnt = np.zeros((n_a, n_b), dtype=np.uint64)
    for i in range(n_a):
        for j in range(n_b):
            m, _ = ctx.setop(L.OP_AND, bA, ra[:, i], bB, rb[:, j])
            m2, _ = ctx.setop(L.OP_AND, m, np.arange(n_sh), bF, rf)
            s, c = ctx.bsi_sum(bS, base, depth, m2, np.arange(n_sh))
            osum[i, j] = int(np.sum(s.astype(np.uint64), dtype=np.uint64).astype(np.int64))
            ocnt[i, j] = int(c.sum())
            m.free()
            m2.free()
    old_s = time.perf_counter() - t0
    equal = bool(np.array_equal(osum, sums) and np.array_equal(ocnt, counts))
    for b in (bA, bB, bF, bS):
        b.free()
    return {"workload": "old_path", "shards": n_sh, "n_a": n_a, "n_b": n_b, "depth": depth, "filter": True, "one_shot_call_ms": round(min(new_t) * 1e3, 2),
            "per_group_path_ms": round(old_s * 1e3, 1), "speedup": round(old_s / min(new_t), 1), "outputs_equal": equal,
            "per_group_calls": n_a * n_b * 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--tag", default="groupby_sum")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    for name, fn in (("W1", w1), ("W2", w2), ("old", old_path)):
        if a.only and name != a.only:
            continue
        r = fn(ctx, torch, a.runs)
        print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, f"{a.tag}_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
        if name == "old" and not r["outputs_equal"]:
            sys.exit(1)
    ctx.close()


if __name__ == "__main__":
    main()
