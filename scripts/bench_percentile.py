"""Percentile(field=, nth=, filter=) of an int field (fbk_bsi_percentile): timings for DESIGN.md §6, one JSON file per case under
--out.  Every case runs the new call (synchronous, wall clock) and, in the same process, on the same resident batches and
alternating with it, the path it replaces: Executor::PercentileBySearch's call sequence driven through ctypes — the total
(fbk_count of the exists rows, after fbk_setop(AND) with a filter), fbk_bsi_min, fbk_bsi_max, then the reference's bisection with
one or two fbk_bsi_range calls per step, each followed by fbk_setop(AND) with the filter and fbk_count.  Outputs of the two paths
are compared before any time is reported.

  P1  96 shards (1.0 x 10^8 columns), bit depth 64, dense field, no filter, nth = 50
  P2  the same under a filter of about half the columns
  P3  64 shards, bit depth 20, optimize()d (encoded) field, nth = 50
  P4  P1 with nine nth values in ONE call, against nine searches
Every result carries the bytes one walk over the planes reads (rows read x 128 KiB x shards), the number of passes and what that
many walks cost at the HBM peak; the kernel times come from the trace.
Usage: python scripts/bench_percentile.py --out profiles [--only P1,P2,P3,P4] [--runs 20] [--no-old]
Kernel split: rocprofv3 --kernel-trace --stats -- python scripts/bench_percentile.py --only P1 --runs 1 --no-old --out /tmp/x"""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HBM_BPS = 8.0e12
OLD_PATH = True  # --no-old: the new call only (kernel-trace runs)
ROW = 128 << 10
DIGIT_BITS = 11
WARM = 3
NINE = [1, 5, 10, 25, 50, 75, 90, 95, 99]


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def search_path(ctx, L, bS, base, depth, bF, rf, nth):
    """Executor::PercentileBySearch (Base 0): (value, count) or None, and the number of fbk_bsi_range calls it took"""
    lib, n = ctx.lib, base.size
    counts = np.zeros(n, dtype=np.uint64)
    ranges = 0

    def count_of(batch, rows, owned):
        if bF is not None:
            h = C.c_void_p()
            L.check(lib.fbk_setop(ctx.h, L.OP_AND, batch, rows.ctypes.data, bF.h, rf.ctypes.data, n, L.SETOP_OPTIMIZE, C.byref(h), None))
            L.check(lib.fbk_count(ctx.h, h, np.arange(n, dtype=np.uint32).ctypes.data, n, counts.ctypes.data))
            lib.fbk_batch_free(ctx.h, h)
        else:
            L.check(lib.fbk_count(ctx.h, batch, rows.ctypes.data, n, counts.ctypes.data))
        if owned:
            lib.fbk_batch_free(ctx.h, batch)
        return int(counts.sum())

    def range_count(op, value):
        nonlocal ranges
        ranges += 1
        h = C.c_void_p()
        L.check(lib.fbk_bsi_range(ctx.h, bS.h, base.ctypes.data, n, op, depth, C.c_int64(value), L.SETOP_OPTIMIZE, C.byref(h), None))
        return count_of(h, np.arange(n, dtype=np.uint32), True)

    def fold(fn, smaller):
        vals, cnts = fn(bS, base, depth, bF, rf)
        best = None
        for v, c in zip(vals.tolist(), cnts.tolist()):
            if c and (best is None or (v < best[0] if smaller else v > best[0])):
                best = [v, c]
            elif c and v == best[0]:
                best[1] += c
        return best

    total = count_of(bS.h, base, False)
    if total == 0:
        return None, ranges
    less = float(total) * nth
    less = int(less / 100.0)
    more = float(total) * (100 - nth)
    more = int(more / 100.0)
    mn = None
    if more != 0:
        mn = fold(ctx.bsi_min, True)
        if less == 0:
            return tuple(mn), ranges
    mx = fold(ctx.bsi_max, False)
    if more == 0:
        return tuple(mx), ranges
    lo, hi, guess = mn[0], mx[0], mn[0]
    while lo < hi:
        guess = _tdiv(lo, 2) + _tdiv(hi, 2) + _tdiv((lo - 2 * _tdiv(lo, 2)) + (hi - 2 * _tdiv(hi, 2)), 2)
        if range_count(L.BSI_LT, guess) > less:
            hi = guess - 1
            continue
        if range_count(L.BSI_GT, guess) > more:
            lo = guess + 1
            continue
        break
    return (guess, 1), ranges


def dense_field(ctx, torch, n_frag, depth, seed):
    """n_frag fragments of uniform values on every column (exists all ones, random sign and planes; at depth 64 the top plane is
    clear, so that every magnitude is below 2^63 and the range search and the select read the same int64), and a filter of random
    words (about half the columns)"""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def words(shape):
        return torch.randint(-(1 << 62), 1 << 62, shape, dtype=torch.int64, device="cuda", generator=g) * 2 + \
            torch.randint(0, 2, shape, dtype=torch.int64, device="cuda", generator=g)

    S = torch.empty((n_frag, depth + 2, 16, 1024), dtype=torch.int64, device="cuda")
    for f0 in range(0, n_frag, 32):  # (a block at a time: randint makes temporaries)
        f1 = min(n_frag, f0 + 32)
        S[f0:f1] = words((f1 - f0, depth + 2, 16, 1024))
    S[:, 0] = -1
    if depth == 64:
        S[:, 65] = 0
    F = words((n_frag, 16, 1024))
    torch.cuda.synchronize()
    bS, bF = ctx.upload_dense_device(S.data_ptr(), n_frag * (depth + 2)), ctx.upload_dense_device(F.data_ptr(), n_frag)
    torch.cuda.synchronize()
    del S, F
    return bS, bF


def new_path(ctx, bS, base, depth, bF, rf, nths):
    v, c, total = ctx.bsi_percentile(bS, base, depth, nths, 0, bF, rf)
    return [(int(a), int(b)) if b else None for a, b in zip(v, c)], total


def old_path(ctx, L, bS, base, depth, bF, rf, nths):
    out, ranges = [], 0
    for nth in nths:
        r, k = search_path(ctx, L, bS, base, depth, bF, rf, float(nth))
        out.append(r)
        ranges += k
    return out, ranges


def stats(ts):
    a = np.array(ts)
    return {"median_ms": round(float(np.median(a)), 3), "p10_ms": round(float(np.percentile(a, 10)), 3), "p90_ms": round(float(np.percentile(a, 90)), 3)}


def compare(ctx, L, args, runs):
    """alternating: new, old, new, old, ... after WARM warm-ups of each; outputs compared first"""
    got, total = new_path(ctx, *args)
    equal, ranges = None, None
    if OLD_PATH:
        exp, ranges = old_path(ctx, L, *args)
        equal = got == exp
        if not equal:
            return got, total, {"outputs_equal": False, "new": got, "old": exp}
    for _ in range(WARM - 1):
        new_path(ctx, *args)
        if OLD_PATH:
            old_path(ctx, L, *args)
    new_t, old_t = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        new_path(ctx, *args)
        new_t.append((time.perf_counter() - t0) * 1e3)
        if OLD_PATH:
            t0 = time.perf_counter()
            old_path(ctx, L, *args)
            old_t.append((time.perf_counter() - t0) * 1e3)
    t = {"runs": runs, "warmups": WARM, "new": stats(new_t), "old_path": stats(old_t) if old_t else None, "old_path_range_calls": ranges,
         "speedup_of_medians": round(float(np.median(old_t) / np.median(new_t)), 1) if old_t else None, "outputs_equal": equal}
    return got, total, t


def describe(case, n_sh, depth, nths, got, total, t, filter_rows, **extra):
    passes = -(-(depth + 1 if depth <= 62 else 64) // DIGIT_BITS)
    walk = n_sh * (depth + 2 + filter_rows) * ROW
    return {"case": case, "shards": n_sh, "depth": depth, "nth": [float(x) for x in nths], "total": int(total), "result": got, **t, "passes": passes,
            "walk_bytes": walk, "walk_hbm_bound_us": round(walk / HBM_BPS * 1e6, 1), "passes_hbm_bound_us": round(passes * walk / HBM_BPS * 1e6, 1), **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-old", action="store_true")
    a = ap.parse_args()
    global OLD_PATH
    OLD_PATH = not a.no_old
    want = a.only.split(",") if a.only else ["P1", "P2", "P3", "P4"]
    data = None
    if "P3" in want:  # generated before the device is opened (host only)
        import datagen as D
        from bench_groupby_sum import bsi_flat

        data = bsi_flat(D, 64, 20, 9400)
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    results = []
    if {"P1", "P2", "P4"} & set(want):
        n_sh, depth = 96, 64
        bS, bF = dense_field(ctx, torch, n_sh, depth, 51)
        rf = np.arange(n_sh, dtype=np.uint32)
        base = rf * (depth + 2)
        for case, filt, nths in (("P1", None, [50]), ("P2", bF, [50]), ("P4", None, NINE)):
            if case in want:
                got, total, t = compare(ctx, L, (bS, base, depth, filt, rf if filt is not None else None, nths), a.runs)
                results.append((case, describe(case, n_sh, depth, nths, got, total, t, 1 if filt is not None else 0)))
        bS.free()
        bF.free()
    if "P3" in want:
        n_sh, depth = 64, 20
        bS = ctx.upload_flat(data.descs(), data.payload(), data.n_rows)
        base = np.arange(n_sh, dtype=np.uint32) * (depth + 2)
        got, total, t = compare(ctx, L, (bS, base, depth, None, None, [50]), a.runs)
        results.append(("P3", describe("P3", n_sh, depth, [50], got, total, t, 0, layout="optimize()d field", encoded_bytes=int(data.payload().size))))
        bS.free()
    ok = True
    for name, r in results:
        print(json.dumps(r), flush=True)
        ok = ok and r["outputs_equal"] is not False
        with open(os.path.join(a.out, f"percentile_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
