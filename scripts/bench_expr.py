"""A whole bitmap call tree in one launch (fbk_expr_eval) against the chain of existing calls it replaces: timings for DESIGN.md §6,
one JSON file per case under --out.  Both forms run ALTERNATING in one process on resident rows (config 3's mixed rows, 64 per
shard, with its density-0.5 filter row standing for the existence row; config 5's BSI field: 64 dense planes + exists + sign),
outputs compared on the device (XOR of the two results is empty, counts equal).  The yardstick is the chain, never the new call
against itself:

  a  Intersect(r0, r1, r2)                                         chain: 2 x fbk_setop (as Executor::eval folds); also fbk_fold_n
  b  Intersect(Union(r0, r1), Not(r2), Row(x > 5))                 chain: 4 x fbk_setop + fbk_bsi_range
  c  Union of the shard's 64 rows                                  chain: fbk_fold_n, the kernel tuned for exactly this shape
                                                                   (and the 63 x fbk_setop a node-by-node fold makes of it)
  d  Intersect(Union(Intersect(r0, Row(x > 5)), Xor(r1, r2)), Difference(r3, Row(x < -1000)))     chain: 5 x fbk_setop + 2 x fbk_bsi_range

Per form: wall clock of the synchronous call(s) (median, min, max over --runs alternations) and the algorithmic bytes; for the
fused call also the kernel time the library's own events report (option time_kernels).  Algorithmic bytes — every
operand's encoded payload once per read, every result's payload once per write; intermediates of the chain are written and read
again; a BSI predicate counts every row of its fragment once, in both forms.  Usage: python scripts/bench_expr.py --out profiles [--only a|b|c|d] [--runs 20] [--shards 96]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Rows:
    """rows of a batch, one per shard, with the payload bytes they hold"""

    def __init__(self, batch, rows, owned=False):
        self.batch, self.rows, self.owned = batch, np.ascontiguousarray(rows, dtype=np.uint32), owned
        self._bytes = None

    _resident = {}  # id(batch) -> payload bytes per row, for the batches that stay (the results of calls are freed: never cached)

    def nbytes(self):
        if self._bytes is None:
            by_row = None if self.owned else Rows._resident.get(id(self.batch))
            if by_row is None:
                d, _, n_rows = self.batch.download_flat()
                per = np.where(d["type"] == 1, 2 * d["len"].astype(np.int64), np.where(d["type"] == 3, 4 * d["len"].astype(np.int64), 8192))
                per = np.where(d["n"] == 0, 0, per)
                by_row = np.bincount(d["row"], weights=per, minlength=n_rows)
                if not self.owned:
                    Rows._resident[id(self.batch)] = by_row
            self._bytes = int(by_row[self.rows].sum())
        return self._bytes

    def free(self):
        if self.owned:
            self.batch.free()


class World:
    def __init__(self, ctx, n_sh):
        import datagen as D
        from featurebase_amd import lib as L

        self.ctx, self.n, self.L = ctx, n_sh, L
        d, p, nr, groups, fd, fp, enc = D.config3_flat_subprocess(n_sh)
        self.batch, self.F, self.groups = ctx.upload_flat(d, p, nr), ctx.upload_flat(fd, fp, n_sh), groups
        self.depth = 64
        w = D.dense_rows(n_sh * (self.depth + 2), 0.5, 5001).reshape(n_sh, self.depth + 2, 16, 1024)
        w[:, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)  # exists: every column has a value (config 5)
        self.V = ctx.upload_dense(w.reshape(-1))
        del w
        self.base = np.arange(n_sh, dtype=np.uint32) * (self.depth + 2)
        self.idx = np.arange(n_sh, dtype=np.uint32)
        self.bsi_bytes = n_sh * (self.depth + 2) * 16 * 8192  # every row of the fragment, once per predicate (both forms)

    def r(self, k):
        return ("row", self.batch, self.groups[:, k])

    def exists(self):
        return ("row", self.F, self.idx)

    def pred(self, op, value):
        return ("bsi", op, value)


def leaves_and_program(w, tree):
    from featurebase_amd import roaring as R

    cache = {}

    def conv(t):
        if t[0] == "row":
            key = (id(t[1]), t[2].tobytes())
            if key not in cache:
                cache[key] = R.row_leaf(t[1], t[2])
            return cache[key]
        if t[0] == "bsi":
            if t not in cache:
                cache[t] = R.bsi_leaf(w.V, w.base, t[1], w.depth, t[2])
            return cache[t]
        return (t[0], *[conv(c) for c in t[1:]])

    return R.compile_expr(conv(tree))


def fused_bytes(w, tree):
    if tree[0] == "row":
        return Rows(tree[1], tree[2]).nbytes()
    if tree[0] == "bsi":
        return w.bsi_bytes
    return sum(fused_bytes(w, c) for c in tree[1:])


class Chain:
    """the tree node by node through the existing calls, every node with FBK_SETOP_OPTIMIZE as Executor::eval asks for it"""

    def __init__(self, w, fold_plain_rows):
        self.w, self.fold = w, fold_plain_rows
        self.calls = self.read = self.written = 0

    def _after(self, out, read):
        self.calls += 1
        if self.count_bytes:
            self.read += read
            self.written += out.nbytes()

    def node(self, t):
        w, L = self.w, self.w.L
        if t[0] == "row":
            return Rows(t[1], t[2])
        if t[0] == "bsi":
            b, _ = w.ctx.bsi_range(w.V, w.base, t[1], w.depth, t[2], L.SETOP_OPTIMIZE)
            out = Rows(b, w.idx, True)
            self._after(out, w.bsi_bytes)
            return out
        op = {"and": L.OP_AND, "or": L.OP_OR, "xor": L.OP_XOR, "andnot": L.OP_ANDNOT, "not": L.OP_ANDNOT}[t[0]]
        kids = t[1:]
        if self.fold and len(kids) > 2 and all(k[0] == "row" and k[1] is kids[0][1] for k in kids):
            b, _ = w.ctx.fold_n(op, kids[0][1], np.stack([k[2] for k in kids], axis=1), L.SETOP_OPTIMIZE)
            out = Rows(b, w.idx, True)
            self._after(out, sum(Rows(k[1], k[2]).nbytes() for k in kids) if self.count_bytes else 0)
            return out
        acc = self.node(kids[0])
        for k in kids[1:]:
            rhs = self.node(k)
            b, _ = w.ctx.setop(op, acc.batch, acc.rows, rhs.batch, rhs.rows, L.SETOP_OPTIMIZE)
            out = Rows(b, w.idx, True)
            self._after(out, acc.nbytes() + rhs.nbytes() if self.count_bytes else 0)
            acc.free()
            rhs.free()
            acc = out
        return acc

    def run(self, tree, count_bytes=False):
        self.calls = self.read = self.written = 0
        self.count_bytes = count_bytes
        return self.node(tree)


def stats(xs):
    a = np.asarray(xs, dtype=np.float64) * 1e6
    return {"median_us": round(float(np.median(a)), 1), "min_us": round(float(a.min()), 1), "max_us": round(float(a.max()), 1)}


def case(w, name, what, tree, runs, fold_plain_rows=False, extra_chain=None):
    ctx, L = w.ctx, w.L
    leaves, prog = leaves_and_program(w, tree)
    chain = Chain(w, fold_plain_rows)
    # outputs compared, bytes counted (untimed)
    fo, fcnt = ctx.expr_eval(leaves, prog, L.SETOP_OPTIMIZE)
    co = chain.run(tree, count_bytes=True)
    res_bytes = Rows(fo, w.idx, True).nbytes()  # (owned: a call's result is never cached by id)
    x, xcnt = ctx.setop(L.OP_XOR, fo, w.idx, co.batch, co.rows)
    assert int(xcnt.sum()) == 0 and fcnt.tolist() == co.batch.count(co.rows).tolist(), f"case {name}: the fused result differs from the chain's"
    x.free()
    out = {"case": name, "what": what, "shards": w.n, "runs": runs, "program_words": int(prog.size), "leaves": len(leaves),
           "result_cardinality": int(fcnt.sum()), "outputs_equal": True,
           "fused": {"calls": 1, "algorithmic_bytes_read": fused_bytes(w, tree), "algorithmic_bytes_written": res_bytes},
           "chain": {"calls": chain.calls, "algorithmic_bytes_read": chain.read, "algorithmic_bytes_written": chain.written,
                     "form": "fbk_fold_n for the level of plain rows" if fold_plain_rows else "pairwise fbk_setop / fbk_bsi_range, node by node"}}
    fused_total = out["fused"]["algorithmic_bytes_read"] + res_bytes
    out["bytes_fused_over_chain"] = round(fused_total / max(1, chain.read + chain.written), 3)
    co.free()
    fo.free()
    # the fused kernel by the library's events
    ctx.set_option("time_kernels", 1)
    try:
        fk = []
        for _ in range(max(3, runs // 4)):
            b, _ = ctx.expr_eval(leaves, prog, L.SETOP_OPTIMIZE)
            fk.append(ctx.get_option("last_kernel_ns"))
            b.free()
    finally:
        ctx.set_option("time_kernels", 0)
    out["fused"]["kernel_us_median"] = round(float(np.median(fk)) / 1e3, 1)
    # wall clock of the synchronous calls, alternating
    tf, tc, te = [], [], []
    for i in range(runs + 2):
        t0 = time.perf_counter()
        b, _ = ctx.expr_eval(leaves, prog, L.SETOP_OPTIMIZE)
        t1 = time.perf_counter()
        c = chain.run(tree)
        t2 = time.perf_counter()
        b.free()
        c.free()
        if i >= 2:  # two warm-up rounds
            tf.append(t1 - t0)
            tc.append(t2 - t1)
        if extra_chain is not None and i >= 2 and i % 4 == 2:
            t0 = time.perf_counter()
            extra_chain.run(tree).free()
            te.append(time.perf_counter() - t0)
    out["fused"]["call"] = stats(tf)
    out["chain"]["call"] = stats(tc)
    if te:
        out["chain_pairwise"] = {"calls": extra_chain.calls, "call": stats(te), "form": "pairwise fbk_setop, node by node"}
    out["fused_over_chain_wall"] = round(out["fused"]["call"]["median_us"] / out["chain"]["call"]["median_us"], 3)
    # the prepared form: memset + one launch
    q = ctx.query_expr(leaves, prog, L.SETOP_OPTIMIZE)
    ctx.set_option("time_kernels", 1)
    try:
        ns = []
        for _ in range(runs + 3):
            q.run()
            q.read()
            ns.append(ctx.get_option("last_kernel_ns"))
    finally:
        ctx.set_option("time_kernels", 0)
    assert q.read().tolist() == fcnt.tolist()
    q.free()
    out["prepared_kernel_us_median"] = round(float(np.median(ns[3:])) / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--only", default="")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--shards", type=int, default=96)
    a = ap.parse_args()
    from featurebase_amd import lib as L
    from featurebase_amd.roaring import Context

    ctx = Context(0)
    w = World(ctx, a.shards)
    gt5, lt = w.pred(L.BSI_GT, 5), w.pred(L.BSI_LT, -1000)
    cases = {
        "a": ("Intersect(r0, r1, r2)", ("and", w.r(0), w.r(1), w.r(2)), {}),
        "b": ("Intersect(Union(r0, r1), Not(r2), Row(x > 5))", ("and", ("or", w.r(0), w.r(1)), ("not", w.exists(), w.r(2)), gt5), {}),
        "c": ("Union of 64 rows", ("or", *[w.r(k) for k in range(64)]), {"fold_plain_rows": True, "extra_chain": Chain(w, False)}),
        "d": ("Intersect(Union(Intersect(r0, Row(x > 5)), Xor(r1, r2)), Difference(r3, Row(x < -1000)))",
              ("and", ("or", ("and", w.r(0), gt5), ("xor", w.r(1), w.r(2))), ("andnot", w.r(3), lt)), {}),
    }
    os.makedirs(a.out, exist_ok=True)
    for name, (what, tree, kw) in cases.items():
        if a.only and name != a.only:
            continue
        res = case(w, name, what, tree, a.runs, **kw)
        if name == "a":  # the one-level form of the same tree
            res["chain_fold_n"] = case(w, "a", what, tree, a.runs, fold_plain_rows=True)["chain"]
        with open(os.path.join(a.out, f"expr_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res), flush=True)
    for b in (w.batch, w.F, w.V):
        b.free()
    ctx.close()


if __name__ == "__main__":
    main()
