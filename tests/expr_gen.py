"""Seeded generator of bitmap call trees for fbk_expr_* (shared by tests/test_expr_cpu.py and tests/test_gpu_expr.py), the numpy
model they are checked against, and the Python restatement of the planner's rules.

A World(it) is small on purpose: 1-3 shards, two set batches ("A": 5 rows per shard, "B": 4 rows per shard — row 0 the existence
row Not() subtracts from, row 3 EMPTY) and one BSI fragment per shard (batch "V").  The rows hold containers of all three
encodings plus nil and full ones, and shard 0's first row has an array of over 4096 values.  Trees over that world: depth 1 to
the limit, fan-out 1 to 64, repeated leaves, Not, predicates of bit depth 0 / 1 / 63 / 64 and BETWEEN.  FBK_TEST_SEED re-rolls
everything (datagen.SEED), FBK_FUZZ_ITERS runs more iterations.

The model: a row is [16, 1024] uint64 words per shard; the four operators are numpy's; a BSI leaf is what the oracle's
fragment.rangeOp / rangeBetween transcription gives (oracle.pybsi)."""
import os
import subprocess
from typing import Dict, List, Optional, Tuple

import numpy as np

import datagen as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = int(os.environ.get("FBK_FUZZ_ITERS", "24"))

# include/fbk.h
ROW, BSI, BETWEEN = 0, 1, 2
PUSH, AND, OR, XOR, ANDNOT = 0, 1, 2, 3, 4
MAX_LEAVES, MAX_PROG, MAX_DEPTH = 256, 1024, 8
OPCODE = {"and": AND, "or": OR, "xor": XOR, "andnot": ANDNOT, "not": ANDNOT}
BSI_OPS = [1, 2, 3, 4, 5, 6]  # FBK_BSI_EQ .. FBK_BSI_GTE (the oracle's numbering is the same)
RA, RB = 5, 4                 # rows per shard of the two set batches
DEPTHS = [0, 1, 63, 64, 5, 12]


class Leaf:
    """One leaf: kind ROW (batch "A" / "B", rows[s] = row ordinal) or BSI / BETWEEN over batch "V" (rows[s] = base row)."""

    def __init__(self, kind, batch, rows, op=0, bit_depth=0, lo=0, hi=0, has_batch=True):
        self.kind, self.batch, self.rows, self.op, self.bit_depth, self.lo, self.hi, self.has_batch = kind, batch, list(rows), op, bit_depth, lo, hi, has_batch

    def __repr__(self):
        if self.kind == ROW:
            return f"{self.batch}{self.rows}"
        return f"V(op={self.op}, d={self.bit_depth}, {self.lo}, {self.hi})" if self.kind == BSI else f"V(d={self.bit_depth}, {self.lo}..{self.hi})"


def postfix(tree) -> Tuple[List[Leaf], List[int]]:
    """nested tuples -> (leaves, program words).  An operator folds its operands left to right; ("not", exists, x) = exists \\ x."""
    leaves, index, prog = [], {}, []

    def walk(t):
        if isinstance(t, Leaf):
            if id(t) not in index:
                index[id(t)] = len(leaves)
                leaves.append(t)
            prog.append((PUSH << 24) | index[id(t)])
            return
        walk(t[1])
        for a in t[2:]:
            walk(a)
            prog.append(OPCODE[t[0]] << 24)

    walk(tree)
    return leaves, prog


def stack_depth(prog: List[int]) -> int:
    sp = deepest = 0
    for w in prog:
        sp += 1 if (w >> 24) == PUSH else -1
        deepest = max(deepest, sp)
    return deepest


def words_of_row(row: Dict[int, object]) -> np.ndarray:
    w = np.zeros((16, 1024), dtype=np.uint64)
    for k, c in row.items():
        w[k & 15] = c.words()
    return w


def words_of_bitmap(bm) -> np.ndarray:
    w = np.zeros((16, 1024), dtype=np.uint64)
    if bm is not None:
        for k, c in bm.items():
            w[k & 15] = c.words()
    return w


def apply(name: str, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    if name == "and":
        return a & b
    if name == "or":
        return a | b
    if name == "xor":
        return a ^ b
    return a & ~b


class World:
    def __init__(self, it: int):
        from oracle import pybsi

        self.it = it
        rng = self.rng = D.rng_for(9100, it)
        self.n_shards = 1 + it % 3
        self.depth = DEPTHS[it % len(DEPTHS)]
        self.rows = {"A": [], "B": []}  # batch -> rows in ordinal order, each {key: oracle container}
        forced = ["array_dense_runs", "run_full", "bitmap_dense", None, "run_many", "array_small", "bitmap_sparse", "array_big"]
        for s in range(self.n_shards):
            for r in range(RA):
                rid = s * RA + r
                row = D.random_row(rng, rid, p_missing=0.45)
                if s == 0 and r == 0:  # every encoding, a nil slot, a full container and an array of over 4096 values for certain
                    for slot, kind in enumerate(forced):
                        row.pop(rid * 16 + slot, None)
                        if kind:
                            row[rid * 16 + slot] = D.oracle_container(rng, kind)
                self.rows["A"].append(row)
            for r in range(RB):
                rid = s * RB + r
                if r == 0:  # the existence row: dense
                    row = {rid * 16 + slot: D.oracle_container(rng, ["bitmap_dense", "run_full", "run_split"][int(rng.integers(0, 3))]) for slot in range(16)}
                elif r == RB - 1:
                    row = {}  # a batch's empty row is a leaf like any other
                else:
                    row = D.random_row(rng, rid, p_missing=0.3)
                self.rows["B"].append(row)
        # one BSI fragment per shard
        self.frags, self.values = [], []
        lim = (1 << min(self.depth, 63)) - 1
        for s in range(self.n_shards):
            cols = rng.choice(1 << 20, size=200, replace=False)
            vals = {}
            for c in cols.tolist():
                mag = int.from_bytes(rng.bytes(8), "little") & lim
                vals[int(c)] = -mag if rng.random() < 0.4 else mag
            self.values.append(vals)
            self.frags.append(pybsi.bsi_fragment_from_values(vals, self.depth))
        self.base = [s * (self.depth + 2) for s in range(self.n_shards)]
        self.a = [Leaf(ROW, "A", [s * RA + r for s in range(self.n_shards)]) for r in range(RA)]
        self.b = [Leaf(ROW, "B", [s * RB + r for s in range(self.n_shards)]) for r in range(RB)]
        self.exists, self.empty = self.b[0], self.b[RB - 1]
        self.preds = [self._predicate_leaf(rng) for _ in range(6)]
        self._cache: Dict[int, np.ndarray] = {}

    # -- leaves -------------------------------------------------------------------------------------------------------
    def _predicate(self, rng) -> int:
        lim = (1 << min(self.depth, 63)) - 1
        some = list(self.values[0].values())
        pick = int(rng.integers(0, 8))
        if pick == 0:
            return 0
        if pick == 1:
            return int(rng.choice([-1, 1]))
        if pick == 2:
            return lim if rng.random() < 0.5 else -lim
        if pick == 3:  # beyond the field
            return min(lim + 1, (1 << 63) - 1) * int(rng.choice([-1, 1]))
        v = some[int(rng.integers(0, len(some)))]
        return max(-(1 << 63) + 1, min((1 << 63) - 1, v + int(rng.integers(-1, 2))))

    def _predicate_leaf(self, rng) -> Leaf:
        if rng.random() < 0.35:
            lo, hi = self._predicate(rng), self._predicate(rng)
            if rng.random() < 0.85 and lo > hi:
                lo, hi = hi, lo
            return Leaf(BETWEEN, "V", self.base, 0, self.depth, lo, hi)
        return Leaf(BSI, "V", self.base, BSI_OPS[int(rng.integers(0, 6))], self.depth, self._predicate(rng), 0)

    def random_leaf(self, rng) -> Leaf:
        pool = self.a + self.b + self.preds
        return pool[int(rng.integers(0, len(pool)))]

    # -- trees --------------------------------------------------------------------------------------------------------
    def _gen(self, rng, budget: int, level: int):
        if budget <= 1 or level >= 5 or rng.random() < 0.3:
            return self.random_leaf(rng)
        name = ["and", "or", "xor", "andnot", "not"][int(rng.integers(0, 5))]
        if name == "not":
            return ("not", self.exists, self._gen(rng, budget - 1, level + 1))
        k = int(rng.choice([1, 2, 2, 3, 4]))
        return (name, self._gen(rng, budget, level + 1), *[self._gen(rng, budget - 1, level + 1) for _ in range(k - 1)])

    def tree(self):
        """this iteration's tree: four designated shapes, the rest random"""
        rng, shape = self.rng, self.it % 8
        ops = ["and", "or", "xor", "andnot"]
        if shape == 0:  # exactly at the depth limit: l0 op (l1 op (l2 op ...)) pushes MAX_DEPTH leaves before the first operator
            t = self.random_leaf(rng)
            for _ in range(MAX_DEPTH - 1):
                t = (ops[int(rng.integers(0, 4))], self.random_leaf(rng), t)
            return t
        if shape == 1:  # fan-out 64 (leaves repeat: the world has fewer rows)
            pool = self.a + self.b
            return ("or", *[pool[int(rng.integers(0, len(pool)))] for _ in range(64)])
        if shape == 2:  # a single PUSH
            return self.random_leaf(rng)
        if shape == 3:  # subtrees on both sides of every operator, predicates among them: values are saved and combined
            p = self.preds
            return ("xor", ("and", ("or", p[0], p[1]), ("andnot", self.a[0], p[2])), ("or", ("and", p[3], self.a[1]), ("not", self.exists, ("xor", p[4], p[5]))))
        while True:
            t = self._gen(rng, int(rng.integers(2, MAX_DEPTH + 1)), 0)
            leaves, prog = postfix(t)
            if len(prog) <= MAX_PROG and len(leaves) <= MAX_LEAVES and stack_depth(prog) <= MAX_DEPTH:
                return t

    # -- the model ----------------------------------------------------------------------------------------------------
    def leaf_words(self, leaf: Leaf) -> np.ndarray:
        """[n_shards, 16, 1024] uint64"""
        if id(leaf) not in self._cache:
            from oracle import pybsi

            out = np.zeros((self.n_shards, 16, 1024), dtype=np.uint64)
            for s in range(self.n_shards):
                if leaf.kind == ROW:
                    out[s] = words_of_row(self.rows[leaf.batch][leaf.rows[s]])
                elif leaf.kind == BSI:
                    out[s] = words_of_bitmap(pybsi.bsi_range(self.frags[s], leaf.op, leaf.bit_depth, leaf.lo))
                else:
                    out[s] = words_of_bitmap(pybsi.bsi_range_between(self.frags[s], leaf.bit_depth, leaf.lo, leaf.hi))
            self._cache[id(leaf)] = out
        return self._cache[id(leaf)]

    def fragment_row_words(self, row: int) -> np.ndarray:
        """row `row` (0 exists, 1 sign, 2 + i plane i) of every shard's BSI fragment"""
        return np.stack([words_of_bitmap(self.frags[s].rows[row]) for s in range(self.n_shards)])

    def model(self, tree) -> np.ndarray:
        if isinstance(tree, Leaf):
            return self.leaf_words(tree)
        acc = self.model(tree[1])
        for t in tree[2:]:
            acc = apply("andnot" if tree[0] == "not" else tree[0], acc, self.model(t))
        return acc


def popcount(words: np.ndarray) -> np.ndarray:
    """[n_shards, 16, 1024] -> cardinality per shard"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], -1), axis=1).sum(axis=1).astype(np.uint64)


# ---- malformed programs (tag = the rule that must refuse them) --------------------------------------------------------------------
def malformed(w: World) -> List[Tuple[str, List[Leaf], List[int]]]:
    a, v = w.a, w.preds[0]
    two = [a[0], a[1]]
    push = lambda i: (PUSH << 24) | i  # noqa: E731
    bad_leaf = lambda **kw: Leaf(**{**dict(kind=BSI, batch="V", rows=w.base, op=3, bit_depth=w.depth, lo=1, hi=0), **kw})  # noqa: E731
    return [
        ("underflow", two, [push(0), AND << 24]),
        ("underflow", two, [OR << 24]),
        ("underflow", two, [push(0), push(1), AND << 24, XOR << 24]),
        ("leftover", two, [push(0), push(1)]),
        ("leftover", two, [push(0), push(1), push(0), OR << 24]),
        ("leaf_index", two, [push(2)]),
        ("leaf_index", two, [push(0), push(0xFFFFFF), OR << 24]),
        ("opcode", two, [push(0), push(1), 5 << 24]),
        ("opcode", two, [push(0), 255 << 24]),
        ("max_depth", two, [push(0)] * (MAX_DEPTH + 1) + [OR << 24] * MAX_DEPTH),
        ("n_prog", two, []),
        ("max_prog", two, [push(0)] + [push(1), OR << 24] * (MAX_PROG // 2)),
        ("max_leaves", [a[i % RA] for i in range(MAX_LEAVES + 1)], [push(0)]),
        ("leaf_kind", [a[0], bad_leaf(kind=3)], [push(0)]),
        ("bit_depth", [a[0], bad_leaf(bit_depth=65)], [push(0)]),
        ("bit_depth", [bad_leaf(kind=BETWEEN, bit_depth=1000)], [push(0)]),
        ("null_batch", [a[0], Leaf(ROW, "A", a[1].rows, has_batch=False)], [push(0)]),
        ("range_op", [bad_leaf(op=0)], [push(0)]),
        ("range_op", [v, bad_leaf(op=7)], [push(0)]),
    ]


def verdict(leaves: List[Leaf], prog: List[int]):
    """The rules of include/fbk.h restated: ("OK", depth) or ("ERR", tag), rules in the planner's order."""
    if len(prog) == 0:
        return "ERR", "n_prog"
    if len(prog) > MAX_PROG:
        return "ERR", "max_prog"
    if len(leaves) > MAX_LEAVES:
        return "ERR", "max_leaves"
    for lf in leaves:
        if not lf.has_batch:
            return "ERR", "null_batch"
        if lf.kind not in (ROW, BSI, BETWEEN):
            return "ERR", "leaf_kind"
        if lf.kind != ROW and lf.bit_depth > 64:
            return "ERR", "bit_depth"
        if lf.kind == BSI and lf.op not in BSI_OPS:
            return "ERR", "range_op"
    sp = deepest = 0
    for wd in prog:
        opc, leaf = wd >> 24, wd & 0xFFFFFF
        if opc > ANDNOT:
            return "ERR", "opcode"
        if opc == PUSH:
            if leaf >= len(leaves):
                return "ERR", "leaf_index"
            sp += 1
            deepest = max(deepest, sp)
            if sp > MAX_DEPTH:
                return "ERR", "max_depth"
        else:
            if sp < 2:
                return "ERR", "underflow"
            sp -= 1
    if sp != 1:
        return "ERR", "leftover"
    return "OK", deepest


# ---- the stand-alone planner check (tests/cpp/expr_plan_check.cpp) -------------------------------------------------------------
def build_checker(out: str) -> str:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "expr_plan_check.cpp"), "-o", out])
    return out


def run_checker(exe: str, cases: List[Tuple[List[Leaf], List[int]]], corpus_path: str) -> List[List[str]]:
    with open(corpus_path, "w") as f:
        for leaves, prog in cases:
            f.write(f"case {len(leaves)} {len(prog)}\n")
            for lf in leaves:
                f.write(f"leaf {lf.kind} {lf.op} {lf.bit_depth} {lf.lo} {lf.hi} {int(lf.has_batch)}\n")
            f.write("prog " + " ".join(str(x) for x in prog) + "\n")
    run = subprocess.run([exe, corpus_path], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, f"expr_plan_check exit {run.returncode}\n{run.stderr[-4000:]}"
    out = [line.split() for line in run.stdout.splitlines()]
    assert len(out) == len(cases), f"{len(out)} verdicts for {len(cases)} cases"
    return out


# the planner's instruction set (fbk_expr_plan.h, enum Ins), interpreted by numpy
I_LOAD, I_AND, I_ANDN, I_OR, I_XOR, I_ANDN_REV, I_MOR_XA, I_MOR_XAN, I_MZERO, I_X_FROM_M, I_ZERO_X, I_PUSH, I_POP = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16


def run_lowered(w: World, leaves: List[Leaf], ins: List[int]) -> Tuple[np.ndarray, int]:
    """(X after the last instruction, the most values saved at once)"""
    shape = (w.n_shards, 16, 1024)
    X, M, stack, deepest = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64), [], 0

    def f(op, x, t):
        return {I_LOAD: t, I_AND: x & t, I_ANDN: x & ~t, I_OR: x | t, I_XOR: x ^ t, I_ANDN_REV: t & ~x}[op]

    for word in ins:
        op, leaf, row = word >> 24, (word >> 12) & 0xFFF, word & 0xFFF
        if op <= I_MOR_XAN:
            lf = leaves[leaf]
            assert row == 0 or (lf.kind != ROW and row < lf.bit_depth + 2), (op, leaf, row)
            T = w.leaf_words(lf) if lf.kind == ROW else w.fragment_row_words(row)
            if op <= I_ANDN_REV:
                X = f(op, X, T)
            else:
                M = M | (X & (T if op == I_MOR_XA else ~T))
        elif op == I_MZERO:
            M = np.zeros(shape, np.uint64)
        elif op == I_X_FROM_M:
            X = M.copy()
        elif op == I_ZERO_X:
            X = np.zeros(shape, np.uint64)
        elif op == I_PUSH:
            stack.append(X.copy())
            deepest = max(deepest, len(stack))
        else:
            assert I_POP + I_AND <= op <= I_POP + I_ANDN_REV and stack, op
            X = f(op - I_POP, X, stack.pop())
    assert not stack
    return X, deepest
