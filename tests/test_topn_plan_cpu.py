"""CPU checks of the host rules of the TopK / TopN family (featurebase_amd/csrc/fbk_topn_plan.h, no GPU): the header is compiled
into a stand-alone program (tests/cpp/topn_plan_check.cpp, -fsanitize=address,undefined, as tests/expr_rows_gen.py builds its
checker) and
  (a) fbk_topn_plan::plan, the ONE sizing rule of a call's passes and scratch vectors, is compared on a grid with a Python
      restatement and with the three formulas it replaced — the one-shot calls', the prepared query's and the call-tree calls' —
      each for the sources it served;
  (b) fbk_topn_plan::order, the ONE host ordering, is compared with expr_rows_gen.top_of on vectors with ties and zeros, with and
      without candidate flags."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import expr_rows_gen as RG
import fuzz_topn_gen as FT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ROW, TREE = 0, 1, 2


@pytest.fixture(scope="module")
def checker():
    out = os.path.join(ROOT, "build", "topn_plan_check_san")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "topn_plan_check.cpp"), "-o", out])

    def run(lines):
        r = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"topn_plan_check exit {r.returncode}\n{r.stderr[-4000:]}"
        got = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got

    return run


def pass_shards(n_a, n_shards, kb):
    """fuzz_topn_gen.Case.pass_shards on a stand-in case: the shards one pass holds under option matrix_pass_kb"""
    return FT.Case.pass_shards(SimpleNamespace(n_shards=n_shards, options={"matrix_pass_kb": kb}), n_a)


def restated(n_a, ns, source, mt, tt, cand_n, kb, keep_ps, keep_src):
    """(pass_shards, tanimoto in force, thresholds, cands, shard, cards, src, cand words)"""
    tani = tt if source != NONE else 0  # a Tanimoto threshold without a source is ignored
    thresholds = mt > 0 or tani > 0
    ps = ns if keep_ps else pass_shards(n_a, ns, kb)
    rules = thresholds or cand_n > 0
    return [ps, tani, int(thresholds), int(cand_n > 0), ps * n_a, ps * n_a if rules and source != NONE else 0,
            ns if source != NONE and (rules or keep_src) else 0, n_a if cand_n else 0]


# The formulas the rule replaced, as the three allocation sites wrote them: (pass_shards, cards words, source counts?, flags words).
def former_one_shot(n_a, ns, filt, mt, tt, cand_n, kb):  # topn_totals_locked + topn_impl
    thresholds = mt > 0 or (tt > 0 and filt)
    ps = max(1, min(ns, (kb << 10) // (n_a * 8)))
    both = (thresholds or cand_n > 0) and filt
    return ps, ps * n_a if both else 0, bool(both), n_a if cand_n else 0


def former_prepared(n_a, ns, filt, mt, tt, cand_n, kb):  # fbk_query_topn: `thresholds` included cand_n
    thresholds = mt > 0 or (tt > 0 and filt) or cand_n > 0
    ps = max(1, min(ns, (kb << 10) // (n_a * 8)))
    both = thresholds and filt
    return ps, ps * n_a if both else 0, bool(both), n_a if cand_n else 0


def former_tree(n_a, ns, mt, tt, cand_n, kb, keep_ps, keep_src):  # expr_rows_totals_locked
    thresholds = mt > 0 or tt > 0
    ps = ns if keep_ps else max(1, min(ns, (kb << 10) // (n_a * 8)))
    return ps, ps * n_a if thresholds or cand_n else 0, bool(thresholds or cand_n or keep_src), n_a if cand_n else 0


def test_one_sizing_rule(checker):
    grid = [(n_a, ns, src, mt, tt, cand_n, kb, kps, ksrc)
            for n_a in (1, 64, 65, 4096, 4097, 1 << 22) for ns in (1, 3, 96, 1024) for src in (NONE, ROW, TREE)
            for mt, tt in ((0, 0), (2, 0), (0, 30), (2, 30)) for cand_n in (0, 3) for kb in (1, 4, 1 << 20)
            for kps in (0, 1) for ksrc in (0, 1)]
    got = checker(["S " + " ".join(str(x) for x in g) for g in grid])
    several = one = 0
    for g, out in zip(grid, got):
        n_a, ns, src, mt, tt, cand_n, kb, kps, ksrc = g
        assert out == restated(*g), g
        ps, tani, thresholds, cands, shard_w, cards_w, src_w, cand_w = out
        assert 1 <= ps <= ns and shard_w == ps * n_a and src_w in (0, ns) and (kps == 0 or ps == ns), g
        several += ps < ns
        one += ps == ns
        # the source counts are [n_shards] words indexed by the call's shard for every source (the former one-shot and prepared
        # forms kept [pass_shards], pass-local): their PRESENCE is what is compared with the former formulas
        mine = (ps, cards_w, src_w > 0, cand_w)
        if src == TREE:
            assert mine == former_tree(n_a, ns, mt, tt, cand_n, kb, bool(kps), bool(ksrc)), g
        elif not kps and not ksrc:  # (the calls over a filter row or none never kept either)
            assert mine == former_one_shot(n_a, ns, src == ROW, mt, tt, cand_n, kb), g
            assert mine == former_prepared(n_a, ns, src == ROW, mt, tt, cand_n, kb), g
    assert several > 100 and one > 100
    # the cases tests/test_gpu_topn_paths.py relies on: matrix_pass_kb = 1 holds one shard of 65 or 200 rows, all three of 5
    assert [pass_shards(n, 3, 1) for n in (5, 65, 200)] == [3, 1, 1]


def test_one_host_ordering(checker):
    rng = np.random.default_rng(8100)
    vectors = [np.asarray([3, 0, 9, 3, 9], dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.asarray([7], dtype=np.uint64), np.zeros(0, dtype=np.uint64),
               np.full(6, 5, dtype=np.uint64), np.asarray([1 << 63, 1, (1 << 63) + 1, 1 << 63], dtype=np.uint64)]
    vectors += [rng.integers(0, 4, size=n).astype(np.uint64) for n in (2, 17, 64, 65, 300)]  # few values: many ties and zeros
    lines, want = [], []
    for v in vectors:
        n = v.size
        flag_sets = [None, np.ones(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), rng.integers(0, 2, size=n).astype(np.uint64) * 5]
        for flags in flag_sets:
            for k in sorted({0, 1, n, n + 3}):
                body = [k, 0 if flags is None else 1, n] + v.tolist() + ([] if flags is None else flags.tolist())
                lines.append("O " + " ".join(str(x) for x in body))
                kept = v if flags is None else np.where(flags != 0, v, np.uint64(0))
                want.append(RG.top_of(kept, k)[0])
    got = checker(lines)
    for line, g, w in zip(lines, got, want):
        assert g[0] == len(g) - 1 and g[1:] == w, line
    # the two vectors of tests/test_expr_rows_cpu.py
    assert checker(["O 0 0 5 3 0 9 3 9", "O 3 0 5 3 0 9 3 9"]) == [[4, 2, 4, 0, 3], [3, 2, 4, 0]]
