"""Extract(Limit(filter, limit=, offset=), Rows(int field), Rows(set field)) (fbk_extract_*): timings for DESIGN.md §6, one JSON
file per case under --out.  Every case runs the new calls (open, columns, bsi, rows — each synchronous, wall clock) and, in the
same process and alternating with them, what the ABI without fbk_extract_* can do for the same answer — the reference's
procedure: the filter's columns from its downloaded rows (for a limit: fbk_count per shard, the span's rows downloaded, cut on
the host, uploaded again), then per bit plane / per field row ONE fbk_setop(AND) with the filter and a download, and the rotation
in numpy.  Outputs of the two paths are compared (bit-exact) in every case.

  E1  full extraction: 32 shards, dense random filter at ~50 %, a depth-20 int field, a set field of 64 rows (density 1/16)
  E2  the SQL shape: 1024 shards, filter = an all-ones existence row per shard, limit = 1000 at offset 0 and at half the count; the
      fields of E1 (shard s uses fragment s mod 32).  Asserted, not timed: the handle's span is ONE shard, and E2 at offset 0
      takes less than 1024 x E1's per-shard time.
  E3  encoded batches: 8 shards of 256 field rows at log-uniform densities in [0.001, 0.5] (tests/datagen.py, BASELINE's
      generator), its 0.5 filter, an optimize()d depth-20 int field.
Usage: python scripts/bench_extract.py --out profiles [--only E1|E2|E3] [--runs 3] [--no-old]
Kernel split: rocprofv3 --kernel-trace --stats -- python scripts/bench_extract.py --only E1 --runs 1 --no-old --out /tmp/x"""
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
OLD_PATH = True  # --no-old: the new calls only (kernel-trace runs)
ROW = 128 << 10


def words_of_batch(batch):
    """a downloaded batch as dense words [n_rows, 16, 1024] (slot = key & 15)"""
    descs, payload, n_rows = batch.download_flat()
    w = np.zeros((n_rows, 16, 1024), dtype=np.uint64)
    for d in descs:
        off, ln, slot = int(d["off"]), int(d["len"]), int(d["key"]) & 15
        if d["type"] == 2:
            w[d["row"], slot] = payload[off:off + 8192].view(np.uint64)
            continue
        bits = np.zeros(65536, dtype=np.uint8)
        if d["type"] == 1:
            bits[payload[off:off + 2 * ln].view(np.uint16)] = 1
        else:
            for a, b in payload[off:off + 4 * ln].view(np.uint16).reshape(-1, 2).astype(np.int64):
                bits[a:b + 1] = 1
        w[d["row"], slot] = np.packbits(bits, bitorder="little").view(np.uint64)
    return w


def unpack(w):
    return np.unpackbits(np.ascontiguousarray(w).view(np.uint8).reshape(-1), bitorder="little")


def old_path(ctx, L, bF, rf, ids, bS, base, depth, bA, ra, offset=0, limit=None):
    """the same answer without fbk_extract_*; returns (columns, values, present, offsets, items)"""
    n_sh = rf.size
    counts = bF.count(rf).astype(np.int64)
    pre = np.concatenate(([0], np.cumsum(counts)))
    lo = min(offset, int(pre[-1]))
    hi = int(pre[-1]) if limit is None else min(int(pre[-1]), lo + limit)
    if hi == lo:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(1, np.uint64), np.zeros(0, np.uint32)
    s0, s1 = int(np.searchsorted(pre, lo, "right")) - 1, int(np.searchsorted(pre, hi, "left")) - 1
    span = np.arange(s0, s1 + 1)
    same, _ = ctx.setop(L.OP_AND, bF, rf[span], bF, rf[span])
    fw = words_of_batch(same)
    same.free()
    pos = []
    for k, s in enumerate(span):  # the cut, on the host
        p = np.nonzero(unpack(fw[k]))[0]
        p = p[max(0, lo - int(pre[s])):max(0, hi - int(pre[s]))]
        pos.append(p)
        bits = np.zeros(1 << 20, dtype=np.uint8)
        bits[p] = 1
        fw[k] = np.packbits(bits, bitorder="little").view(np.uint64).reshape(16, 1024)
    cut = ctx.upload_dense(fw.reshape(-1))
    ident = np.arange(span.size, dtype=np.uint32)
    cols = np.concatenate([(np.uint64(ids[s]) << np.uint64(20)) + p.astype(np.uint64) for s, p in zip(span, pos)])

    def gathered(batch, rows):  # one set-op with the filter and a download, then the bits at the selected positions
        out, _ = ctx.setop(L.OP_AND, batch, rows, cut, ident)
        w = words_of_batch(out)
        out.free()
        return np.concatenate([unpack(w[k])[p] for k, p in enumerate(pos)])

    pres = gathered(bS, base[span]).astype(bool)
    neg = gathered(bS, base[span] + 1).astype(bool)
    mag = np.zeros(cols.size, dtype=np.uint64)
    for b in range(depth):
        mag |= gathered(bS, base[span] + 2 + b).astype(np.uint64) << np.uint64(b)
    vals = np.where(pres, np.where(neg, ~mag + np.uint64(1), mag), 0).view(np.int64)
    member = np.stack([gathered(bA, ra[span, i]) for i in range(ra.shape[1])], axis=1).astype(bool)
    offs = np.concatenate(([0], np.cumsum(member.sum(axis=1)))).astype(np.uint64)
    cut.free()
    return cols, vals, pres, offs, np.nonzero(member)[1].astype(np.uint32)


def new_path(ctx, bF, rf, ids, bS, base, depth, bA, ra, offset=0, limit=None):
    t = {}
    t0 = time.perf_counter()
    h = ctx.extract(bF, rf, ids, offset, limit)
    t["open_ms"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    cols = h.columns()
    t["columns_ms"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    vals, pres = h.bsi(bS, base, depth)
    t["bsi_ms"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    offs, items = h.rows(bA, ra, cap=max(1, h.n) * ra.shape[1] // 8)
    t["rows_ms"] = time.perf_counter() - t0
    span = h.span()
    h.close()
    return (cols, vals, pres, offs, items), {k: v * 1e3 for k, v in t.items()}, span


def compare(ctx, L, args, runs, old_runs, **kw):
    """alternating: new, old, new, old, ...; medians; outputs compared"""
    new_path(ctx, *args, **kw)  # warm
    old_runs = old_runs if OLD_PATH else 0
    new_t, old_t, equal, span = [], [], True, None
    for r in range(runs):
        got, t, span = new_path(ctx, *args, **kw)
        new_t.append(t)
        if r < old_runs:
            t0 = time.perf_counter()
            exp = old_path(ctx, L, *args, **kw)
            old_t.append((time.perf_counter() - t0) * 1e3)
            equal = equal and all(np.array_equal(a, b) for a, b in zip(got, exp))
    med = {k: round(float(np.median([t[k] for t in new_t])), 3) for k in new_t[0]}
    med["total_ms"] = round(float(np.median([sum(t.values()) for t in new_t])), 3)
    old = round(float(np.median(old_t)), 1) if old_t else None
    return got, {"runs": runs, **med, "old_path_ms": old, "old_runs": old_runs, "speedup": round(old / med["total_ms"], 1) if old_t else None, "outputs_equal": equal,
                 "span": list(span)}


def dense_fields(ctx, torch, n_frag, depth, n_a, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rows(n, ands=0):
        t = torch.randint(-(1 << 62), 1 << 62, (n, 16, 1024), dtype=torch.int64, device="cuda", generator=g) * 2 + \
            torch.randint(0, 2, (n, 16, 1024), dtype=torch.int64, device="cuda", generator=g)
        for _ in range(ands):
            t &= torch.randint(-(1 << 62), 1 << 62, (n, 16, 1024), dtype=torch.int64, device="cuda", generator=g) * 2
        return t

    S, A = rows(n_frag * (depth + 2)), rows(n_frag * n_a, 3)
    torch.cuda.synchronize()
    bS, bA = ctx.upload_dense_device(S.data_ptr(), S.shape[0]), ctx.upload_dense_device(A.data_ptr(), A.shape[0])
    torch.cuda.synchronize()
    return bS, bA, rows


def e1_e2(ctx, torch, L, runs, want):
    n_frag, depth, n_a = 32, 20, 64
    bS, bA, rows = dense_fields(ctx, torch, n_frag, depth, n_a, 31)
    out = []
    F = rows(n_frag)
    bF = ctx.upload_dense_device(F.data_ptr(), n_frag)
    torch.cuda.synchronize()
    rf, ids = np.arange(n_frag, dtype=np.uint32), np.arange(n_frag, dtype=np.uint64)
    base, ra = rf * (depth + 2), np.arange(n_frag * n_a, dtype=np.uint32).reshape(n_frag, n_a)
    got, t = compare(ctx, L, (bF, rf, ids, bS, base, depth, bA, ra), runs, 1)
    n, m = int(got[0].size), int(got[4].size)
    moved = {"open": 2 * n_frag * ROW + n_frag * ROW, "columns": n_frag * ROW + 8 * n, "bsi": n_frag * (depth + 3) * ROW + 9 * n,
             "rows": 2 * n_frag * (n_a + 1) * ROW + 24 * n + 4 * m}
    e1 = {"case": "E1", "shards": n_frag, "depth": depth, "n_a": n_a, "columns": n, "items": m, **t, "device_bytes": moved,
          "hbm_bound_ms": {k: round(v / HBM_BPS * 1e3, 3) for k, v in moved.items()}, "per_shard_ms": round(t["total_ms"] / n_frag, 3)}
    out.append(("E1", e1))
    bF.free()
    if "E2" in want:
        n_sh = 1024
        ones = torch.full((n_sh, 16, 1024), -1, dtype=torch.int64, device="cuda")
        bF = ctx.upload_dense_device(ones.data_ptr(), n_sh)
        torch.cuda.synchronize()
        del ones
        rf, ids = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint64)
        base, ra = (rf % n_frag) * (depth + 2), (rf % n_frag)[:, None] * n_a + np.arange(n_a, dtype=np.uint32)[None, :]
        ra = np.ascontiguousarray(ra, dtype=np.uint32)
        for tag, off in (("E2_offset0", 0), ("E2_deep", (n_sh << 20) // 2)):
            got, t = compare(ctx, L, (bF, rf, ids, bS, base, depth, bA, ra), max(runs, 5), 2, offset=off, limit=1000)
            assert t["span"][1] == 1, t["span"]  # the per-field kernels are launched over ONE shard: grid = 1024 units of it
            r = {"case": tag, "shards": n_sh, "limit": 1000, "offset": off, "depth": depth, "n_a": n_a, "columns": int(got[0].size), **t,
                 "field_kernel_units": t["span"][1] * 1024, "e1_per_shard_ms_x_1024": round(e1["per_shard_ms"] * 1024, 1)}
            if off == 0:
                r["skip_works"] = bool(t["total_ms"] < e1["per_shard_ms"] * 1024)
                assert r["skip_works"], (t["total_ms"], e1["per_shard_ms"] * 1024)
            out.append((tag, r))
        bF.free()
    bS.free()
    bA.free()
    return out


def e3(ctx, L, runs, data):
    (rows, groups, filt), bs, n_sh, k, depth = data
    bA, bF = ctx.upload_flat(rows.descs(), rows.payload(), rows.n_rows), ctx.upload_flat(filt.descs(), filt.payload(), n_sh)
    bS = ctx.upload_flat(bs.descs(), bs.payload(), bs.n_rows)
    rf, ids = np.arange(n_sh, dtype=np.uint32), np.arange(n_sh, dtype=np.uint64)
    base = rf * (depth + 2)
    got, t = compare(ctx, L, (bF, rf, ids, bS, base, depth, bA, groups), runs, 1)
    r = {"case": "E3", "shards": n_sh, "depth": depth, "n_a": k, "layout": "log-uniform densities [0.001, 0.5], optimize()d encodings",
         "columns": int(got[0].size), "items": int(got[4].size), "encoded_bytes": int(rows.payload().size), **t}
    for b in (bA, bF, bS):
        b.free()
    return [("E3", r)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-old", action="store_true")
    a = ap.parse_args()
    global OLD_PATH
    OLD_PATH = not a.no_old
    want = [a.only] if a.only else ["E1", "E2", "E3"]
    data = None
    if "E3" in want:  # generated before the device is opened (host only)
        import datagen as D
        from bench_groupby_sum import bsi_flat

        n_sh, k, depth = 8, 256, 20
        dens = np.exp(D.rng_for(5000, 0xE3).uniform(np.log(0.001), np.log(0.5), k)).tolist()
        data = (D.config3_flat(n_sh, k, 5000, workers=1, densities=dens, run_frac=0.0), bsi_flat(D, n_sh, depth, 9300), n_sh, k, depth)
    import torch

    import __graft_entry__ as g

    g.build()
    from featurebase_amd import lib as L
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    os.makedirs(a.out, exist_ok=True)
    results = []
    if "E1" in want or "E2" in want:
        results += e1_e2(ctx, torch, L, a.runs, want)
    if "E3" in want:
        results += e3(ctx, L, a.runs, data)
    ok = True
    for name, r in results:
        print(json.dumps(r), flush=True)
        ok = ok and r["outputs_equal"]
        with open(os.path.join(a.out, f"extract_{name}.json"), "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
