"""Distinct() of an int field as a device Row (fbk_bsi_distinct_rows) against the path it replaces for a join — fbk_bsi_distinct (sorted
values to the host), the containers of the row built on the host with numpy, fbk_batch_upload — alternating in one process, the two
resulting batches downloaded and compared.  Timings for DESIGN.md §6, one JSON file per case under --out.  Both paths are synchronous
calls that end with a device batch: each run times the whole path, wall clock, over --runs warm runs.

  FK        a foreign key: 256 shards, every column holds a value, depth 24, values uniform in [0, 2^20): ~2^20 distinct parents,
            256 child records per parent.
  UNIQUE    a unique key: 256 shards, the value of a column is its id (depth 28): every value distinct, the scatter pass issues one
            atomic per column.
  FILTERED  FK's field under a filter of about 1 % of the columns (seven random words ANDed: 2^-7).
Usage: python scripts/bench_distinct_rows.py --out profiles [--only FK|UNIQUE|FILTERED] [--runs 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_SH = 256


def planes(torch, values_of_shard, depth):
    """[N_SH * (depth + 2), 16, 1024] int64 words on the device: exists on every column, no sign, the magnitude planes"""
    shifts = torch.arange(64, device="cuda", dtype=torch.int64)
    S = torch.zeros((N_SH, depth + 2, 1 << 14), dtype=torch.int64, device="cuda")
    for s in range(N_SH):
        v = values_of_shard(s).view(1 << 14, 64)
        S[s, 0] = -1
        for k in range(depth):
            S[s, 2 + k] = (((v >> k) & 1) << shifts).sum(-1)
    torch.cuda.synchronize()
    return S


def host_row_batch(ctx, values):
    """sorted distinct non-negative values -> the batch of Pos's shard rows (bitmap containers) and an empty row, built on the host"""
    import datagen as D

    sh = values >> 20
    shards = np.unique(sh)
    bits = np.zeros(max(shards.size, 1) << 20, dtype=np.uint8)
    bits[(np.searchsorted(shards, sh) << 20) | (values & 0xFFFFF)] = 1
    n = bits.reshape(-1, 65536).sum(axis=1, dtype=np.int64)
    words = np.packbits(bits, bitorder="little").reshape(-1, 8192)
    live = np.nonzero(n)[0]
    descs = np.zeros(live.size, dtype=D.DESC_DTYPE)
    descs["key"] = shards[live >> 4] * 16 + (live & 15)
    descs["off"] = np.arange(live.size, dtype=np.uint64) * 8192
    descs["row"] = live >> 4
    descs["len"] = 1024
    descs["n"] = n[live]
    descs["type"] = 2
    return ctx.upload_flat(descs, np.ascontiguousarray(words[live]).reshape(-1), shards.size + 1), shards


def same_rows(a, b):
    """two batches of bitmap containers hold the same rows"""
    (da, pa, na), (db, pb, nb) = a.download_flat(), b.download_flat()
    if na != nb or da.size != db.size or any(not np.array_equal(da[f], db[f]) for f in ("key", "row", "n", "type")):
        return False
    ga = pa.reshape(-1)[(da["off"][:, None] + np.arange(8192, dtype=np.uint64)[None, :]).astype(np.int64)]
    gb = pb.reshape(-1)[(db["off"][:, None] + np.arange(8192, dtype=np.uint64)[None, :]).astype(np.int64)]
    return bool(np.array_equal(ga, gb))


def run_case(ctx, name, bS, depth, bF, runs, note):
    from featurebase_amd import lib as L

    base = np.arange(N_SH, dtype=np.uint32) * (depth + 2)
    rf = np.arange(N_SH, dtype=np.uint32)
    n_distinct = ctx.bsi_distinct(bS, base, depth, bF, rf if bF is not None else None).size  # (also warms the old path)
    vals, cnt = np.zeros(max(n_distinct, 1), dtype=np.int64), C.c_uint64()

    def old():
        L.check(ctx.lib.fbk_bsi_distinct(ctx.h, bS.h, base.ctypes.data, N_SH, depth, bF.h if bF is not None else None,
                                         rf.ctypes.data if bF is not None else None, vals.ctypes.data, vals.size, C.byref(cnt)))
        return host_row_batch(ctx, vals[: cnt.value])

    def new():
        return ctx.bsi_distinct_rows(bS, base, depth, 0, bF, rf if bF is not None else None, cap=4096)

    ob, oshards = old()
    nb = new()
    equal = bool(np.array_equal(oshards, nb[1])) and nb[2].size == 0 and same_rows(ob, nb[0])
    rows, n_values = int(nb[1].size), int(nb[3].sum())
    ob.free()
    nb[0].free()
    t_old, t_new = [], []
    for _ in range(runs):  # alternating: both paths see the same machine state
        t0 = time.perf_counter()
        ob, _ = old()
        t1 = time.perf_counter()
        nb = new()
        t2 = time.perf_counter()
        t_old.append(t1 - t0)
        t_new.append(t2 - t1)
        ob.free()
        nb[0].free()
    o, n = np.array(t_old) * 1e3, np.array(t_new) * 1e3
    return {"case": name, "note": note, "shards": N_SH, "depth": depth, "filter": bF is not None, "distinct_values": n_values, "output_rows": rows,
            "runs": runs, "old_path_median_ms": round(float(np.median(o)), 2), "old_path_min_ms": round(float(o.min()), 2),
            "new_call_median_ms": round(float(np.median(n)), 2), "new_call_min_ms": round(float(n.min()), 2),
            "old_over_new": round(float(np.median(o) / np.median(n)), 2), "outputs_equal": equal,
            "plane_bytes": (depth + 2 + (bF is not None)) * (128 << 10) * N_SH}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tag", default="distinct_rows")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(31)
    cols = torch.arange(1 << 20, device="cuda", dtype=torch.int64)

    def fk(_s):
        return torch.randint(0, 1 << 20, (1 << 20,), device="cuda", generator=gen)

    def unique(s):
        return cols + (s << 20)

    ok = True
    for name, depth, values, filtered, note in (("FK", 24, fk, False, "uniform in [0, 2^20): 256 records per parent"),
                                                ("UNIQUE", 28, unique, False, "value = column id: one atomic per column"),
                                                ("FILTERED", 24, fk, True, "FK under a filter of 2^-7 of the columns")):
        if a.only and name != a.only:
            continue
        S = planes(torch, values, depth)
        bS = ctx.upload_dense_device(S.data_ptr(), N_SH * (depth + 2))
        bF = None
        if filtered:
            F = torch.full((N_SH, 1 << 14), -1, dtype=torch.int64, device="cuda")
            for _ in range(7):
                F &= torch.randint(-(1 << 63), (1 << 63) - 1, F.shape, device="cuda", generator=gen, dtype=torch.int64)
            torch.cuda.synchronize()
            bF = ctx.upload_dense_device(F.data_ptr(), N_SH)
        torch.cuda.synchronize()
        r = run_case(ctx, name, bS, depth, bF, a.runs, note)
        print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, f"{a.tag}_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
        ok = ok and r["outputs_equal"]
        bS.free()
        if bF is not None:
            bF.free()
        del S
    ctx.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
