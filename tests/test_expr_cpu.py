"""CPU checks of fbk_expr_* (no GPU): the numpy model of tests/expr_gen.py against the oracle's pairwise container operations
folded node by node, and the host planner (featurebase_amd/csrc/fbk_expr_plan.h, compiled WITHOUT HIP into
tests/cpp/expr_plan_check.cpp with -fsanitize=address,undefined) against a Python restatement of its rules and, for what it
lowers, against the model: the lowered program interpreted by numpy gives the tree's value.

The default iterations (expr_gen.ITERS = 24) reach every opcode, every leaf kind, the depth limit and every encoding as a leaf —
test_generated_trees_cover_the_ground asserts it rather than promising it."""
import os

import numpy as np
import pytest

import expr_gen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(oracle):
    from oracle import pybsi

    pybsi._lib()
    out = []
    for it in range(G.ITERS):
        w = G.World(it)
        t = w.tree()
        leaves, prog = G.postfix(t)
        out.append((w, t, leaves, prog))
    return out


@pytest.fixture(scope="module")
def checker():
    return G.build_checker(os.path.join(ROOT, "build", "expr_plan_check_san"))


def test_generated_trees_cover_the_ground(cases, oracle):
    O = oracle
    opcodes, kinds, depths, fanout, encodings, bit_depths = set(), set(), set(), set(), set(), set()
    repeated = big_array = nots = False

    def walk(w, t):
        nonlocal nots
        if isinstance(t, G.Leaf):
            return
        fanout.add(len(t) - 1)
        nots |= t[0] == "not"
        for c in t[1:]:
            walk(w, c)

    for w, t, leaves, prog in cases:
        walk(w, t)
        depths.add(G.stack_depth(prog))
        pushes = [x & 0xFFFFFF for x in prog if (x >> 24) == G.PUSH]
        repeated |= len(pushes) != len(set(pushes))
        opcodes |= {x >> 24 for x in prog}
        for lf in leaves:
            kinds.add(lf.kind)
            if lf.kind != G.ROW:
                bit_depths.add(lf.bit_depth)
                continue
            for s in range(w.n_shards):
                row = w.rows[lf.batch][lf.rows[s]]
                encodings |= {c.typ for c in row.values()}
                if len(row) < 16:
                    encodings.add(O.NIL)
                big_array |= any(c.typ == O.ARRAY and c.n > 4096 for c in row.values())
                if any(c.n == 65536 for c in row.values()):
                    encodings.add("full")
    assert opcodes == {G.PUSH, G.AND, G.OR, G.XOR, G.ANDNOT}
    assert kinds == {G.ROW, G.BSI, G.BETWEEN}
    assert {1, G.MAX_DEPTH} <= depths and len(depths) >= 4, depths
    assert {1, 2, 64} <= fanout, fanout
    assert encodings >= {O.NIL, O.ARRAY, O.BITMAP, O.RUN, "full"}, encodings
    assert {0, 1, 63, 64} <= bit_depths, bit_depths
    assert repeated and big_array and nots


def oracle_fold(O, w, tree, s):
    """the tree's value in shard s as 16 oracle containers (None = nil), every operator applied by the oracle's pairwise kernels"""
    from oracle import pybsi

    if isinstance(tree, G.Leaf):
        if tree.kind == G.ROW:
            row = w.rows[tree.batch][tree.rows[s]]
            return [row.get(tree.rows[s] * 16 + slot) for slot in range(16)]
        bm = pybsi.bsi_range(w.frags[s], tree.op, tree.bit_depth, tree.lo) if tree.kind == G.BSI else pybsi.bsi_range_between(w.frags[s], tree.bit_depth, tree.lo, tree.hi)
        by_slot = {k & 15: c for k, c in bm.items()}
        return [by_slot.get(slot) for slot in range(16)]
    name = {"and": "intersect", "or": "union", "xor": "xor", "andnot": "difference", "not": "difference"}[tree[0]]
    acc = oracle_fold(O, w, tree[1], s)
    for t in tree[2:]:
        nxt = oracle_fold(O, w, t, s)
        for slot in range(16):
            a, b = acc[slot], nxt[slot]
            if a is not None and b is not None:
                acc[slot] = O.OPS[name](a, b)
            elif name == "intersect" or (name == "difference" and a is None):
                acc[slot] = None
            elif a is None:  # union / xor with a nil left side
                acc[slot] = b
    return acc


def test_model_equals_the_oracle_folded_node_by_node(cases, oracle):
    for w, t, _, _ in cases:
        m = w.model(t)
        for s in range(w.n_shards):
            got = oracle_fold(oracle, w, t, s)
            for slot in range(16):
                exp = got[slot].words() if got[slot] is not None else np.zeros(1024, np.uint64)
                assert (m[s, slot] == exp).all(), (w.it, s, slot, t)


def test_planner_verdicts_depth_and_lowering(cases, checker, tmp_path):
    good = [(leaves, prog) for _, _, leaves, prog in cases]
    bad = [(tag, leaves, prog) for tag, leaves, prog in G.malformed(cases[0][0])]
    out = G.run_checker(checker, good + [(lv, pr) for _, lv, pr in bad], str(tmp_path / "corpus.txt"))
    for (w, t, leaves, prog), line in zip(cases, out):
        assert G.verdict(leaves, prog) == ("OK", G.stack_depth(prog))
        assert line[0] == "OK", (w.it, line)
        depth, slots, first_leaf, n_ins = (int(x) for x in line[1:5])
        ins = [int(x) for x in line[5:]]
        assert depth == G.stack_depth(prog) and n_ins == len(ins)
        assert first_leaf == prog[0] & 0xFFFFFF
        assert slots <= depth  # what bounds the kernel's LDS by FBK_EXPR_MAX_DEPTH
        x, saved = G.run_lowered(w, leaves, ins)
        assert saved == slots, (w.it, saved, slots)
        assert (x == w.model(t)).all(), (w.it, t)
        # every container is read at most once per time its leaf is pushed: the lowering adds no loads of set rows
        row_loads = sum(1 for i in ins if (i >> 24) <= 7 and leaves[(i >> 12) & 0xFFF].kind == G.ROW)
        assert row_loads == sum(1 for x in prog if (x >> 24) == G.PUSH and leaves[x & 0xFFFFFF].kind == G.ROW)
    for (tag, leaves, prog), line in zip(bad, out[len(good):]):
        assert G.verdict(leaves, prog) == ("ERR", tag), tag
        assert line == ["ERR", tag], (tag, line)


def test_operators_over_row_leaves_save_nothing(checker, tmp_path, oracle):
    """The lowering's point: 'top op= leaf' for a ROW operand on either side, the deeper operand first otherwise.  The WHERE clause
    Intersect(Union(a, b), Not(c), Row(x > 5)) needs one saved value (for the predicate's own scan at most), a 64-way union none."""
    w = G.World(0)
    a, b = w.a, w.b
    gt = G.Leaf(G.BSI, "V", w.base, 5, w.depth, 5, 0)
    where = ("and", ("or", a[1], a[2]), ("not", w.exists, a[3]), gt)
    union64 = ("or", *[a[i % G.RA] for i in range(64)])
    right_deep = ("andnot", a[0], ("xor", a[1], ("or", a[2], ("and", a[3], a[4]))))
    trees = [where, union64, right_deep]
    out = G.run_checker(checker, [G.postfix(t) for t in trees], str(tmp_path / "corpus.txt"))
    slots = [int(line[2]) for line in out]
    assert slots[1] == 0 and slots[2] == 0 and slots[0] <= 2, slots
    for t, line in zip(trees, out):
        x, _ = G.run_lowered(w, G.postfix(t)[0], [int(v) for v in line[5:]])
        assert (x == w.model(t)).all()
