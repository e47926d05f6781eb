"""TopK of a set field over a call tree in the tree's own launch (fbk_expr_topk) against the pair of calls it replaces (fbk_expr_eval,
then fbk_topk with that row as the filter): timings for DESIGN.md §6, one JSON file per case under --out.  The pair runs twice per
round, with flags 0 and with FBK_SETOP_OPTIMIZE, and the faster of the two medians is reported as "the pair".  The fused call and the
pairs ALTERNATE in one process on resident rows and their outputs are compared every round.  The yardstick is the pair — both of its
calls are the code paths of the commit before fbk_expr_topk — never the new call against itself.

Cases (tree b of bench_expr.py: Intersect(Union(r0, r1), Not(r2), Row(x > 5)), x a field of 64 dense planes):
  mixed_<n_a>_<shards>   config 3's mixed rows, n_a in {64, 1024}, shards in {96, 1024}.  A shard has 64 rows: n_a = 1024 lists them
                         16 times.  The BSI field is generated for 96 shards; beyond that shard s reads the fragment of shard s % 96.
  sparse_<n_a>_<shards>  a field of array containers only, 200 values each (400 bytes per row and slot), 96 shards.
  union64_<shards>       tree c of bench_expr.py (Union of the shard's 64 rows) through the new prologue: fbk_expr_row_counts with
                         n_a = 1, next to fbk_expr_count (k_expr_slot) — data for a later decision on that kernel, nothing else.

Per form: wall clock of the synchronous call(s) (median, min, max over --runs alternations after two warm-up rounds) and the kernel time
the library's own events report (option time_kernels; the pair: the sum of its two kernels).  Algorithmic bytes: every operand of the
tree once per block that evaluates it, the field's payload once; the pair evaluates the tree once, writes the filter row and reads it
back once per block.  Usage: python scripts/bench_expr_topk.py --out profiles [--only NAME] [--runs 200]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_expr as BE  # noqa: E402

V_SHARDS = 96
K = 10


class World(BE.World):
    """bench_expr.World with the BSI field generated for at most V_SHARDS shards (1024 shards of 66 dense rows are 8.6 GB)"""

    def __init__(self, ctx, n_sh):
        import datagen as D
        from featurebase_amd import lib as L

        self.ctx, self.n, self.L = ctx, n_sh, L
        d, p, nr, groups, fd, fp, enc = D.config3_flat_subprocess(n_sh)
        self.batch, self.F, self.groups = ctx.upload_flat(d, p, nr), ctx.upload_flat(fd, fp, n_sh), groups
        self.depth = 64
        nv = min(n_sh, V_SHARDS)
        w = D.dense_rows(nv * (self.depth + 2), 0.5, 5001).reshape(nv, self.depth + 2, 16, 1024)
        w[:, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
        self.V = ctx.upload_dense(w.reshape(-1))
        del w
        self.base = (np.arange(n_sh, dtype=np.uint32) % nv) * (self.depth + 2)
        self.idx = np.arange(n_sh, dtype=np.uint32)
        self.bsi_bytes = n_sh * (self.depth + 2) * 16 * 8192


def sparse_field(ctx, n_sh, n_a, per=200):
    """[n_sh * n_a] rows of 16 array containers, `per` sorted distinct values each"""
    import datagen as D

    rng = D.rng_for(7700, n_sh, n_a)
    nc = n_sh * n_a * 16
    vals = (np.cumsum(rng.integers(1, 65536 // per, size=(nc, per), dtype=np.int64), axis=1) - 1).astype(np.uint16)
    d = np.zeros(nc, dtype=D.DESC_DTYPE)
    d["key"] = np.arange(nc, dtype=np.uint64)
    d["off"] = np.arange(nc, dtype=np.uint64) * (2 * per)
    d["row"] = np.arange(nc, dtype=np.uint32) // 16
    d["len"], d["n"], d["type"] = per, per, 1
    return ctx.upload_flat(d, vals.reshape(-1).view(np.uint8), n_sh * n_a), nc * 2 * per


def kernel_resources():
    """(vector registers, blocks per CU by registers and LDS) of k_expr_rows_vs_filter from the built library's code object"""
    from featurebase_amd import lib as L

    llvm = "/opt/rocm/lib/llvm/bin"
    tmp = os.path.join(ROOT, "build", "bench_expr_topk")
    os.makedirs(tmp, exist_ok=True)
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
    subprocess.check_call([f"{llvm}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", L.LIB_PATH, fat])
    subprocess.check_call([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.check_output([f"{llvm}/llvm-readelf", "--notes", co], text=True)
    import re

    for blk in notes.split("  - .agpr_count:")[1:]:
        if "k_expr_rows_vs_filter" in blk:
            g = lambda k: int(re.search(r"\.%s:\s+(\S+)" % k, blk).group(1))  # noqa: E731
            vgpr, lds = g("vgpr_count"), g("group_segment_fixed_size")
            waves = min(8, 512 // max(vgpr, 1))
            return {"vgpr_count": vgpr, "static_lds_bytes": lds, "scratch_bytes": g("private_segment_fixed_size"),
                    "blocks_per_cu_without_saved_values": min(waves * 4 // 4, (160 * 1024) // lds)}
    return {}


def rows_per_block(n_a, n_shards, L):
    rnd = lambda r: max(64, (r + 63) & ~63)  # noqa: E731
    rpb = n_a
    while rpb > 64 and n_shards * 16 * ((n_a + rpb - 1) // rpb) < 2048:
        half = (rpb + 1) // 2
        if ((n_a + rnd(half) - 1) // rnd(half) - 1) * L > n_a:
            break
        rpb = half
    return rnd(rpb)


def kernel_us(ctx, fn, n):
    ctx.set_option("time_kernels", 1)
    try:
        out = [fn(lambda: ctx.get_option("last_kernel_ns")) for _ in range(n)]
    finally:
        ctx.set_option("time_kernels", 0)
    return round(float(np.median(out)) / 1e3, 1)


def case(w, name, what, tree, field, rows, field_bytes, tree_reads, runs):
    ctx, L = w.ctx, w.L
    leaves, prog = BE.leaves_and_program(w, tree)
    n_sh, n_a = rows.shape

    def fused():
        return ctx.expr_topk(leaves, prog, field, rows, K)

    def pair(flags, after=None):
        b, _ = ctx.expr_eval(leaves, prog, flags)
        k = after() if after else 0
        r = ctx.topk(field, rows, K, b, w.idx)
        k += after() if after else 0
        return r, b, k

    same = lambda a, b: a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()  # noqa: E731
    f = fused()
    row_bytes = {}
    for flags in (0, L.SETOP_OPTIMIZE):
        p, b, _ = pair(flags)
        assert same(f, p), f"{name}: the fused result differs from the pair's"
        row_bytes[flags] = BE.Rows(b, w.idx, True).nbytes()
        b.free()
    tree_bytes = BE.fused_bytes(w, tree)
    rpb_f = rows_per_block(n_a, n_sh, tree_reads)
    rpb_p = rows_per_block(n_a, n_sh, 0)
    chunks_f, chunks_p = (n_a + rpb_f - 1) // rpb_f, (n_a + rpb_p - 1) // rpb_p
    out = {"case": name, "what": what, "shards": n_sh, "n_a": n_a, "k": K, "runs": runs, "program_words": int(prog.size), "leaves": len(leaves),
           "operand_reads_per_block_estimate": tree_reads, "results": int(f[0].size), "outputs_equal_every_round": True, "kernel": kernel_resources(),
           "fused": {"calls": 1, "rows_per_block": rpb_f, "blocks_per_shard_slot": chunks_f, "algorithmic_bytes_read": tree_bytes * chunks_f + field_bytes,
                     "algorithmic_bytes_written": 0},
           "pairs": {}}
    names = {0: "flags_0", L.SETOP_OPTIMIZE: "setop_optimize"}
    for flags in (0, L.SETOP_OPTIMIZE):
        out["pairs"][names[flags]] = {"calls": 2, "rows_per_block": rpb_p, "blocks_per_shard_slot": chunks_p,
                                      "algorithmic_bytes_read": tree_bytes + field_bytes + row_bytes[flags] * chunks_p, "algorithmic_bytes_written": row_bytes[flags]}

    def fused_kernel(read):
        fused()
        return read()

    out["fused"]["kernel_us_median"] = kernel_us(ctx, fused_kernel, max(5, runs // 8))
    for flags in (0, L.SETOP_OPTIMIZE):
        def pair_kernels(read, flags=flags):
            _, b, k = pair(flags, read)
            b.free()
            return k

        out["pairs"][names[flags]]["kernels_us_median"] = kernel_us(ctx, pair_kernels, max(5, runs // 8))
    tf, tp = [], {0: [], L.SETOP_OPTIMIZE: []}
    for i in range(runs + 2):
        t0 = time.perf_counter()
        f = fused()
        t1 = time.perf_counter()
        if i >= 2:
            tf.append(t1 - t0)
        for flags in (0, L.SETOP_OPTIMIZE):
            t0 = time.perf_counter()
            p, b, _ = pair(flags)
            t1 = time.perf_counter()
            b.free()
            assert same(f, p), f"{name}: round {i} differs"
            if i >= 2:
                tp[flags].append(t1 - t0)
    out["fused"]["call"] = BE.stats(tf)
    for flags in (0, L.SETOP_OPTIMIZE):
        out["pairs"][names[flags]]["call"] = BE.stats(tp[flags])
    best = min(out["pairs"], key=lambda k: out["pairs"][k]["call"]["median_us"])
    out["pair"] = dict(out["pairs"][best], form="fbk_expr_eval (%s), then fbk_topk with the row as filter" % best)
    out["fused_over_pair_wall"] = round(out["fused"]["call"]["median_us"] / out["pair"]["call"]["median_us"], 3)
    out["fused_over_pair_kernels"] = round(out["fused"]["kernel_us_median"] / out["pair"]["kernels_us_median"], 3)
    return out


def union64(w, runs):
    """tree c through the new prologue: one row of the field, so the launch is the tree plus 16 containers per shard"""
    ctx = w.ctx
    tree = ("or", *[w.r(k) for k in range(64)])
    leaves, prog = BE.leaves_and_program(w, tree)
    rows = w.groups[:, :1].copy()

    def block(read):
        ctx.expr_row_counts(leaves, prog, w.batch, rows)
        return read()

    def wave(read):
        ctx.expr_count(leaves, prog)
        return read()

    tot, fc = ctx.expr_row_counts(leaves, prog, w.batch, rows, filter_counts=True)
    assert fc.tolist() == ctx.expr_count(leaves, prog).tolist()
    return {"case": f"union64_{w.n}", "what": "Union of the shard's 64 rows, n_a = 1", "shards": w.n, "operand_reads_per_block": 64,
            "k_expr_rows_vs_filter_us_median": kernel_us(ctx, block, runs), "k_expr_slot_count_only_us_median": kernel_us(ctx, wave, runs),
            "algorithmic_bytes_read": BE.fused_bytes(w, tree)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--shards", default="96,1024")
    ap.add_argument("--sparse-rows", type=int, default=256)
    a = ap.parse_args()
    from featurebase_amd import lib as L
    from featurebase_amd.roaring import Context

    os.makedirs(a.out, exist_ok=True)

    def emit(res):
        with open(os.path.join(a.out, f"expr_topk_{res['case']}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res), flush=True)

    want = lambda name: not a.only or a.only == name  # noqa: E731
    ctx = Context(0)
    what = "TopK(f, k = 10, filter = Intersect(Union(r0, r1), Not(r2), Row(x > 5)))"
    for n_sh in [int(x) for x in a.shards.split(",")]:
        names = [f"mixed_{n_a}_{n_sh}" for n_a in (64, 1024)] + [f"union64_{n_sh}"] + ([f"sparse_{a.sparse_rows}_{n_sh}"] if n_sh == 96 else [])
        if not any(want(n) for n in names):
            continue
        w = World(ctx, n_sh)
        tree = ("and", ("or", w.r(0), w.r(1)), ("not", w.exists(), w.r(2)), w.pred(L.BSI_GT, 5))
        # operand reads of the lowered tree: r0, r1, the existence row, r2 and the planes of the predicate's scan
        reads = sum(1 for x in ctx_plan_reads(ctx, w, tree))
        for n_a in (64, 1024):
            name = f"mixed_{n_a}_{n_sh}"
            if want(name):
                rows = np.ascontiguousarray(np.tile(w.groups, (1, n_a // 64)).astype(np.uint32))
                fb = BE.Rows(w.batch, rows.reshape(-1)).nbytes()
                emit(case(w, name, what + ", config 3's mixed rows", tree, w.batch, rows, fb, reads, a.runs))
        if want(f"union64_{n_sh}"):
            emit(union64(w, max(5, a.runs // 8)))
        name = f"sparse_{a.sparse_rows}_{n_sh}"
        if n_sh == 96 and want(name):
            field, fb = sparse_field(ctx, n_sh, a.sparse_rows)
            rows = np.arange(n_sh * a.sparse_rows, dtype=np.uint32).reshape(n_sh, a.sparse_rows)
            emit(case(w, name, what + ", array containers of 200 values", tree, field, rows, fb, reads, a.runs))
            field.free()
        for b in (w.batch, w.F, w.V):
            b.free()
    ctx.close()


def ctx_plan_reads(ctx, w, tree):
    """the containers one block reads for the tree: a ROW leaf is one, the predicate x > 5 scans the sign row and every plane (and
    the existence row): counted as depth + 2, the rows of the fragment"""
    def walk(t):
        if t[0] == "row":
            yield 1
        elif t[0] == "bsi":
            for _ in range(w.depth + 2):
                yield 1
        else:
            for c in t[1:]:
                yield from walk(c)

    return walk(tree)


if __name__ == "__main__":
    main()
