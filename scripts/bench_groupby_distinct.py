"""GroupBy with aggregate=Count(Distinct(field)) (fbk_count_matrix_distinct): timings for DESIGN.md §6, one JSON file per
workload under --out.  The call is synchronous (two host reads of the distinct-value count inside it): each workload times the
whole call, wall clock, over --runs warm runs.  The per-kernel split comes from a separate rocprofv3 --kernel-trace --stats run
of one workload.

  D1  the SQL shape: 1024 shards, A a 64-row categorical field (every column in exactly one row, chosen by a hash), B a
      16-row categorical field, a depth-20 BSI field with a value on every column, uniform in [0, 50000); no filter.  Dense
      rows generated on the device with torch.
  D2  dense worst case: 128 shards, 32 x 32 dense random rows + a filter, depth 20 (bench_groupby_sum.dense_batches): the
      one-pass call against the per-group path it replaces (fbk_setop AND per group + fbk_bsi_distinct), outputs compared.
  D3  encoded rows: config 3's mixed rows (tests/datagen.py config3_flat, A = rows 0..31, B = rows 32..63, its filter) and an
      optimize()d depth-20 BSI field (bench_groupby_sum.bsi_flat), 1024 shards: the densify path.
Usage: python scripts/bench_groupby_distinct.py --out profiles [--only D1|D2|D3] [--runs 5]"""
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

from bench_groupby_sum import bsi_flat, dense_batches  # noqa: E402

HBM_BPS = 8.0e12


def time_call(fn, runs):
    out = fn()  # warm: allocations, code objects
    s = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        s.append(time.perf_counter() - t0)
    ms = np.array(s) * 1e3
    return out, {"runs": runs, "median_ms": round(float(np.median(ms)), 2), "min_ms": round(float(ms.min()), 2), "max_ms": round(float(ms.max()), 2)}


def categorical(torch, n_sh, n_rows, salt):
    """[n_sh * n_rows, 16, 1024] int64 words: column c of shard s in row hash(s, c) mod n_rows only"""
    cols = torch.arange(1 << 20, device="cuda", dtype=torch.int64)
    shifts = torch.arange(64, device="cuda", dtype=torch.int64)
    out = torch.empty((n_sh, n_rows, 1 << 14), dtype=torch.int64, device="cuda")
    for s in range(n_sh):
        h = ((cols * 2654435761 + (s * 40503 + salt) * 97) ^ (cols >> 7)) % n_rows
        onehot = (h.view(1, -1) == torch.arange(n_rows, device="cuda").view(-1, 1)).view(n_rows, 1 << 14, 64).to(torch.int64)
        out[s] = (onehot << shifts).sum(-1)
    return out.view(n_sh * n_rows, 16, 1024)


def d1(ctx, torch, runs):
    n_sh, n_a, n_b, depth, n_vals = 1024, 64, 16, 20, 50000
    A, Bt = categorical(torch, n_sh, n_a, 1), categorical(torch, n_sh, n_b, 2)
    g = torch.Generator(device="cuda").manual_seed(21)
    S = torch.zeros((n_sh, depth + 2, 1 << 14), dtype=torch.int64, device="cuda")
    shifts = torch.arange(64, device="cuda", dtype=torch.int64)
    for s in range(n_sh):
        v = torch.randint(0, n_vals, (1 << 20,), device="cuda", generator=g).view(1 << 14, 64)
        S[s, 0] = -1  # exists: every column
        for k in range(depth):
            S[s, 2 + k] = (((v >> k) & 1) << shifts).sum(-1)
    torch.cuda.synchronize()
    bA, bB, bS = (ctx.upload_dense_device(t.data_ptr(), t.numel() // (1 << 14)) for t in (A, Bt, S))
    torch.cuda.synchronize()
    del A, Bt, S
    ra = np.arange(n_sh * n_a, dtype=np.uint32).reshape(n_sh, n_a)
    rb = np.arange(n_sh * n_b, dtype=np.uint32).reshape(n_sh, n_b)
    base = np.arange(n_sh, dtype=np.uint32) * (depth + 2)
    (dist, counts), t = time_call(lambda: ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, depth), runs)
    nbytes = (n_a + n_b + depth + 2) * (128 << 10) * n_sh + (depth + 2) * (128 << 10) * n_sh  # stage 2 operands + stage 1's planes
    res = {"workload": "D1", "shards": n_sh, "n_a": n_a, "n_b": n_b, "depth": depth, "filter": False, "layout": "dense, categorical A / B",
           "values": n_sh << 20, "distinct_total": int(dist.sum()), "groups_with_values": int((counts > 0).sum()), **t,
           "operand_bytes": nbytes, "hbm_bound_ms": round(nbytes / HBM_BPS * 1e3, 2), "scatter_atomics": n_sh << 20}
    for b in (bA, bB, bS):
        b.free()
    return res


def d2(ctx, torch, runs):
    from featurebase_amd import lib as L

    n_sh, n_a, n_b, depth = 128, 32, 32, 20
    (bA, bB, bF, bS), ra, rb, rf, base = dense_batches(ctx, torch, n_sh, n_a, n_b, depth, 12)
    (dist, counts), t = time_call(lambda: ctx.count_matrix_distinct(bA, ra, bB, rb, bS, base, depth, bF, rf), runs)
    t0 = time.perf_counter()
    old = np.zeros((n_a, n_b), dtype=np.uint64)
    ident = np.arange(n_sh, dtype=np.uint32)
    for i in range(n_a):
        for j in range(n_b):
            m, _ = ctx.setop(L.OP_AND, bA, ra[:, i], bB, rb[:, j])
            m2, _ = ctx.setop(L.OP_AND, m, ident, bF, rf)
            old[i, j] = len(ctx.bsi_distinct(bS, base, depth, m2, ident))
            m.free()
            m2.free()
    old_s = time.perf_counter() - t0
    equal = bool(np.array_equal(old, dist))
    for b in (bA, bB, bF, bS):
        b.free()
    return {"workload": "D2", "shards": n_sh, "n_a": n_a, "n_b": n_b, "depth": depth, "filter": True, "layout": "dense random", **t,
            "per_group_path_ms": round(old_s * 1e3, 1), "speedup": round(old_s * 1e3 / t["median_ms"], 1), "outputs_equal": equal,
            "per_group_calls": n_a * n_b * 3, "distinct_max": int(dist.max()), "group_column_pairs": int(counts.sum())}


def d3(ctx, torch, runs):
    import datagen as D

    n_sh, depth, n_frag = 1024, 20, 128
    d, p, nr, groups, fd, fp, enc = D.config3_flat_subprocess(n_sh)
    batch, F = ctx.upload_flat(d, p, nr), ctx.upload_flat(fd, fp, n_sh)
    bs = bsi_flat(D, n_frag, depth, 9100)
    S = ctx.upload_flat(bs.descs(), bs.payload(), bs.n_rows)
    base = (np.arange(n_sh, dtype=np.uint32) % n_frag) * (depth + 2)
    rf = np.arange(n_sh, dtype=np.uint32)
    (dist, counts), t = time_call(lambda: ctx.count_matrix_distinct(batch, groups[:, :32], batch, groups[:, 32:], S, base, depth, F, rf), runs)
    res = {"workload": "D3", "shards": n_sh, "n_a": 32, "n_b": 32, "depth": depth, "filter": True, "layout": "config 3 mixed rows + optimize()d BSI",
           "bsi_fragments_distinct": n_frag, "encoded_bytes_rows": int(enc), "distinct_max": int(dist.max()), **t}
    for b in (batch, F, S):
        b.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tag", default="groupby_distinct")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    for name, fn in (("D1", d1), ("D2", d2), ("D3", d3)):
        if a.only and name != a.only:
            continue
        r = fn(ctx, torch, a.runs)
        print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, f"{a.tag}_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
        if name == "D2" and not r["outputs_equal"]:
            sys.exit(1)
    ctx.close()


if __name__ == "__main__":
    main()
