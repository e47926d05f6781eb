"""Sort(filter, field=, sort-desc=, limit=, offset=) by an int field (fbk_bsi_sort): timings for DESIGN.md §6, one JSON file per case
under --out.  Every case runs the new call (synchronous, wall clock) and, in the same process and alternating with it, the only
path the ABI without fbk_bsi_sort offers for the same answer: an extract handle on the filter, fbk_extract_columns +
fbk_extract_bsi (17 bytes per filtered column over PCIe), then a stable argsort and the cut in numpy on one core.  Outputs of the
two paths are compared (bit-exact) before any time is reported.

  S1   the SQL shape (ORDER BY x LIMIT n): 64 shards (6.7 x 10^7 columns), all-ones filter, depth 20, uniform values, limit 1000,
       ascending and descending
  S1L  the same over 1024 distinct fragments (1.07 x 10^9 columns), new call only
  S2   deep page: S1 with offset 10^6
  S3   full sort: 32 shards, filter ~50 %, no limit (recorded only: the device radix sort and the download dominate)
  S4   S1 with an optimize()d (encoded) field and a sparse encoded filter
Every result carries the bytes a k_sort_hist pass reads (rows read x 128 KiB x shards) and the number of passes; the kernel times
come from the trace.
Usage: python scripts/bench_sort.py --out profiles [--only S1|S1L|S2|S3|S4] [--runs 5] [--no-old]
Kernel split: rocprofv3 --kernel-trace --stats -- python scripts/bench_sort.py --only S1 --runs 1 --no-old --out /tmp/x"""
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

HBM_BPS = 8.0e12
OLD_PATH = True  # --no-old: the new call only (kernel-trace runs)
ROW = 128 << 10
DIGIT_BITS = 11


def old_path(ctx, bS, base, depth, ids, bF, rf, desc, offset, limit):
    """the same answer with the parent ABI: every filtered column and its value cross the bus, one core sorts them"""
    with ctx.extract(bF, rf, ids) as h:
        cols = h.columns()
        vals, pres = h.bsi(bS, base, depth)
    keep = pres & (vals != 0)  # the reference's Sort never sees a stored zero
    cols, vals = cols[keep], vals[keep]
    order = np.argsort(~vals if desc else vals, kind="stable")  # columns are ascending: ties stay in column order
    total = order.size
    lo = min(offset, total)
    hi = total if limit is None else min(total, lo + limit)
    order = order[lo:hi]
    return cols[order], vals[order], total


def new_path(ctx, bS, base, depth, ids, bF, rf, desc, offset, limit):
    return ctx.bsi_sort(bS, base, depth, ids, bF, rf, desc=desc, offset=offset, limit=limit)


def compare(ctx, args, runs, old_runs):
    """alternating: new, old, new, old, ...; medians; outputs compared"""
    new_path(ctx, *args)  # warm
    old_runs = old_runs if OLD_PATH else 0
    new_t, old_t, equal, got = [], [], True, None
    for r in range(runs):
        t0 = time.perf_counter()
        got = new_path(ctx, *args)
        new_t.append((time.perf_counter() - t0) * 1e3)
        if r < old_runs:
            t0 = time.perf_counter()
            exp = old_path(ctx, *args)
            old_t.append((time.perf_counter() - t0) * 1e3)
            equal = equal and np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[2] == exp[2]
    new = round(float(np.median(new_t)), 3)
    old = round(float(np.median(old_t)), 1) if old_t else None
    return got, {"runs": runs, "new_ms": new, "new_min_ms": round(min(new_t), 3), "old_path_ms": old, "old_runs": old_runs,
                 "speedup": round(old / new, 1) if old_t else None, "outputs_equal": equal if old_t else None}


def describe(case, n_sh, depth, got, t, desc, offset, limit, filter_rows=1, **extra):
    passes = -(-(depth + 1 if depth <= 62 else 64) // DIGIT_BITS)
    per_pass = n_sh * (depth + 2 + filter_rows) * ROW
    return {"case": case, "shards": n_sh, "depth": depth, "desc": desc, "offset": offset, "limit": limit, "records": int(got[0].size), "total": int(got[2]), **t,
            "hist_passes": passes if limit is not None else 1, "pass_bytes": per_pass, "pass_hbm_bound_us": round(per_pass / HBM_BPS * 1e6, 1),
            "walks": (passes if limit is not None else 1) + 2, **extra}


def dense_field(ctx, torch, n_frag, depth, seed, filter_ands=None):
    """n_frag fragments of uniform values on every column (exists all ones, random sign and planes), and a filter: all ones, or
    random words ANDed filter_ands times"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    S = torch.empty((n_frag, depth + 2, 16, 1024), dtype=torch.int64, device="cuda")
    for f0 in range(0, n_frag, 64):  # (a block at a time: randint makes temporaries)
        f1 = min(n_frag, f0 + 64)
        S[f0:f1] = torch.randint(-(1 << 62), 1 << 62, (f1 - f0, depth + 2, 16, 1024), dtype=torch.int64, device="cuda", generator=g) * 2 + \
            torch.randint(0, 2, (f1 - f0, depth + 2, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
    S[:, 0] = -1
    if filter_ands is None:
        F = torch.full((n_frag, 16, 1024), -1, dtype=torch.int64, device="cuda")
    else:
        F = torch.randint(-(1 << 62), 1 << 62, (n_frag, 16, 1024), dtype=torch.int64, device="cuda", generator=g) * 2
        for _ in range(filter_ands):
            F &= torch.randint(-(1 << 62), 1 << 62, (n_frag, 16, 1024), dtype=torch.int64, device="cuda", generator=g) * 2 + 1
    torch.cuda.synchronize()
    bS, bF = ctx.upload_dense_device(S.data_ptr(), n_frag * (depth + 2)), ctx.upload_dense_device(F.data_ptr(), n_frag)
    torch.cuda.synchronize()
    del S, F
    return bS, bF


def s1_s2(ctx, torch, runs, want):
    n_sh, depth = 64, 20
    bS, bF = dense_field(ctx, torch, n_sh, depth, 41)
    rf, ids = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint64)
    base = rf * (depth + 2)
    out = []
    for case, off in (("S1", 0), ("S2", 10**6)):
        if case not in want:
            continue
        for desc in (False, True):
            got, t = compare(ctx, (bS, base, depth, ids, bF, rf, desc, off, 1000), runs, 1)
            out.append((f"{case}_{'desc' if desc else 'asc'}", describe(case, n_sh, depth, got, t, desc, off, 1000)))
    bS.free()
    bF.free()
    return out


def s1l(ctx, torch, runs):
    n_sh, depth = 1024, 20
    bS, bF = dense_field(ctx, torch, n_sh, depth, 43)
    rf, ids = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint64)
    base = rf * (depth + 2)
    out = []
    for desc in (False, True):
        got, t = compare(ctx, (bS, base, depth, ids, bF, rf, desc, 0, 1000), runs, 0)
        assert (np.diff(got[1]) <= 0).all() if desc else (np.diff(got[1]) >= 0).all()
        out.append((f"S1L_{'desc' if desc else 'asc'}", describe("S1L", n_sh, depth, got, t, desc, 0, 1000)))
    bS.free()
    bF.free()
    return out


def s3(ctx, torch, runs):
    n_sh, depth = 32, 20
    bS, bF = dense_field(ctx, torch, n_sh, depth, 47, filter_ands=0)
    rf, ids = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint64)
    base = rf * (depth + 2)
    # (the wrapper's first call reports the size, the second fetches: the capacity protocol is part of the call's cost without a limit)
    got, t = compare(ctx, (bS, base, depth, ids, bF, rf, False, 0, None), min(runs, 3), 1)
    bS.free()
    bF.free()
    return [("S3", describe("S3", n_sh, depth, got, t, False, 0, None))]


def s4(ctx, runs, data):
    from featurebase_amd.roaring import Container

    bs, n_sh, depth, filt_rows = data
    bS = ctx.upload_flat(bs.descs(), bs.payload(), bs.n_rows)
    bF = ctx.upload([{sl: Container.array(v) for sl, v in enumerate(row)} for row in filt_rows])
    rf, ids = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint64)
    base = rf * (depth + 2)
    out = []
    for desc in (False, True):
        got, t = compare(ctx, (bS, base, depth, ids, bF, rf, desc, 0, 1000), runs, 1)
        out.append((f"S4_{'desc' if desc else 'asc'}", describe("S4", n_sh, depth, got, t, desc, 0, 1000, layout="optimize()d field, array-container filter at 1/64",
                                                                 encoded_bytes=int(bs.payload().size))))
    bS.free()
    bF.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-old", action="store_true")
    a = ap.parse_args()
    global OLD_PATH
    OLD_PATH = not a.no_old
    want = a.only.split(",") if a.only else ["S1", "S1L", "S2", "S3", "S4"]
    data = None
    if "S4" in want:  # generated before the device is opened (host only)
        import datagen as D
        from bench_groupby_sum import bsi_flat

        n_sh, depth = 64, 20
        rng = D.rng_for(5100, 0x54)
        filt = [[np.sort(rng.choice(65536, size=1024, replace=False)).astype(np.int64) for _ in range(16)] for _ in range(n_sh)]
        data = (bsi_flat(D, n_sh, depth, 9400), n_sh, depth, filt)
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    results = []
    if "S1" in want or "S2" in want:
        results += s1_s2(ctx, torch, a.runs, want)
    if "S1L" in want:
        results += s1l(ctx, torch, a.runs)
    if "S3" in want:
        results += s3(ctx, torch, a.runs)
    if "S4" in want:
        results += s4(ctx, a.runs, data)
    ok = True
    for name, r in results:
        print(json.dumps(r), flush=True)
        ok = ok and r["outputs_equal"] is not False
        with open(os.path.join(a.out, f"sort_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
