"""The generator and the model of the structural fuzz of the prepared forms (tests/fuzz_prepared_gen.py) checked without a GPU: the
cases are deterministic in (seed, iteration); the model's count-matrix, fold, fold + count and TopN expectations equal the restated
reference (oracle/pybatch.py, oracle/pytopn.py) on the same rows; the schedules of the default iterations contain every step the GPU
test exists for (asserted on the model's own words, not on the generator's intentions); and the one-pass Sum(Range) is refused for at
most a quarter of the predicates drawn."""
import numpy as np
import pytest

import datagen as D
import fuzz_prepared_gen as G
from oracle import pybatch as PB
from oracle import pytopn as T


@pytest.fixture(scope="module")
def walked(oracle):
    """[(case, model after the whole schedule)] of the default iterations"""
    out = []
    for it in range(6):
        c = G.Case(it)
        m = G.Model(c)
        for si, st in enumerate(c.steps):
            try:
                m.apply(st)
            except Exception as e:
                raise AssertionError(c.describe(si)) from e
        out.append((c, m))
    return out


def _same(a, b) -> bool:
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_cases_are_deterministic(oracle, monkeypatch):
    a, b = G.Case(1), G.Case(1)
    assert _same(a.steps, b.steps) and _same(a.queries, b.queries) and _same(a.W0, b.W0)
    assert _same(G.PlanCase(2).steps, G.PlanCase(2).steps)
    monkeypatch.setattr(D, "SEED", D.SEED + 1)
    c = G.Case(1)
    assert not _same(a.W0["S0"][:4], c.W0["S0"][:4]) and not (_same(a.steps, c.steps) and _same(a.queries, c.queries))
    assert a.plan_names == c.plan_names, "the forced structure follows the iteration, not the seed"


def test_schedules_are_well_formed(walked):
    for c, m in walked:
        live, ran = set(), set()
        assert 12 <= len(c.steps) <= 50 and 4 <= len([q for q in c.queries if q["refusal"] is None]) <= 10, c
        for si, st in enumerate(c.steps):
            q = c.queries[st["q"]] if "q" in st else None
            if st["do"] == "prepare":
                assert all(not o.startswith("q") or (int(o[1:]) in live and int(o[1:]) in ran) for o in c.operands(q)), c.describe(si)
                for name, rows in (("a", q.get("ra", q.get("groups", q.get("base")))), ("b", q.get("rb")), ("f", q.get("rf"))):
                    if q[name] is not None and rows.size:
                        top = int(rows.max()) + (q["depth"] + 2 if name == "a" and "depth" in q else 1)
                        assert top <= c.size[q[name]], c.describe(si)
                if q["refusal"] is None:
                    live.add(st["q"])
            elif st["do"] in ("run", "read", "free"):
                assert st["q"] in live, c.describe(si)
                assert all(not o.startswith("q") or int(o[1:]) in live for o in c.operands(q)), c.describe(si)
                if st["do"] == "run" and G.run_refusal(q["kind"], st["dest"], st["acc"]) is None:
                    ran.add(st["q"])
                if st["do"] == "read":
                    assert st["q"] in ran, c.describe(si)
                if st["do"] == "free":
                    assert not any(f"q{st['q']}" in c.operands(c.queries[j]) for j in live), c.describe(si)
                    live.discard(st["q"])
            elif st["do"] == "oneshot":
                assert all(not o.startswith("q") or int(o[1:]) in live for o in c.operands(q)), c.describe(si)


def test_default_iterations_cover_the_structure(walked):
    cov = set().union(*(m.cov for _, m in walked))
    want = {"kind:" + k for k in G.KINDS} | {"chain2", "filter_mutable", "empty_slot_rerun", "compact_live", "kps_pass4", "topn_pass", "acc_cell", "stale_read"}
    assert cov >= want, want - cov
    steps = [st for c, _ in walked for st in c.steps]
    assert {st["do"] for st in steps} == {"prepare", "run", "read", "mutate", "compact", "set_option", "oneshot", "free"}
    assert any(c.dense for c, _ in walked) and not all(c.dense for c, _ in walked)
    qs = [q for c, _ in walked for q in c.queries]
    assert any(q["kind"] in G.ROW_KINDS and q["a"].startswith("q") for q in qs), "no row-valued query reads another one's rows"
    assert any(q.get("f") and q["f"].startswith("q") and q["kind"] in ("count_matrix", "topn", "fold_icount") for q in qs), "no query output is a filter"
    assert any(q["kind"] == "count_matrix" and q["rb"].shape[1] == 1 and q["f"] is None for q in qs), "no TopK-shaped count matrix"
    assert any(q["refusal"] is not None for q in qs) and any(st["do"] == "run" and G.run_refusal(c.queries[st["q"]]["kind"], st["dest"], st["acc"])
                                                              for c, _ in walked for st in c.steps), "no refusal is exercised"
    assert any("depth" in q and q["depth"] > 40 for q in qs) and any("depth" in q and q["depth"] < 8 for q in qs)
    assert any("base" in q and np.unique(q["base"]).size < q["base"].size for q in qs), "no BSI fragment repeats across shards"
    assert any(q["kind"] == "bsi_sum" and q["f"] is not None for q in qs)
    assert any(st["do"] == "run" and st["dest"] == "cell" and c.queries[st["q"]]["kind"] in ("bsi_sum", "bsi_range_sum") and not st["acc"]
               for c, _ in walked for st in c.steps), "no BSI records into a caller buffer"


def test_refused_share_of_range_sum_predicates(oracle):
    qs = [q for it in range(max(G.ITERS, 24)) for q in G.Case(it).queries if q["kind"] == "bsi_range_sum"]
    refused = [q for q in qs if q["refusal"] is not None]
    assert len(qs) >= 6 and 4 * len(refused) <= len(qs), (len(refused), len(qs))
    bsi = [q for it in range(6) for q in G.Case(it).queries if q["kind"].startswith("bsi")]
    assert 4 * sum(q["refusal"] is not None for q in bsi) <= len(bsi)
    for q in qs:  # the prediction is the plan function's and nothing else
        assert (q["refusal"] is None) == (G.range_sum_plan(q["op"], q["depth"], q["pred"]) is not None)


@pytest.mark.parametrize("it", range(6))
def test_model_equals_the_restated_reference(walked, it):
    """count matrix, fold, fold + count (Union: the oracle's n-way form; the other operations: chained orc_batch_setop) and the
    per-shard TopN counts on the words every query of the case had at the end of its schedule"""
    c, m = walked[it]
    rs = {}
    seen = set()
    for qi, q in enumerate(c.queries):
        if q["refusal"] is not None or not all(o in m.W for o in c.operands(q)) or q["kind"].startswith("bsi"):
            continue
        for o in c.operands(q):
            if o not in rs:
                rs[o] = PB.RowSet.from_dense(m.W[o])
        res = m._evaluate(q, 0)
        A, F = rs[q["a"]], rs.get(q["f"])
        seen.add(q["kind"])
        if q["kind"] == "count_matrix":
            assert np.array_equal(res["ps"], PB.count_matrix(A, q["ra"], rs[q["b"]], q["rb"], F, q.get("rf"))), (c, qi)
        elif q["kind"] in ("fold", "fold_icount"):
            g = q["groups"]
            if q["op"] == G.OP_OR:
                R, cnt = PB.union_n(A, g)
            else:
                R, cnt = PB.setop(G.OP_OR, A, g[:, 0], A, g[:, 0])  # the first row of every group, then one pairwise call a column
                for j in range(1, g.shape[1]):
                    R, cnt = PB.setop(q["op"], R, np.arange(len(g)), A, g[:, j])
            if q["kind"] == "fold":
                assert np.array_equal(res["out"], R.words()) and np.array_equal(res["value"], cnt), (c, qi)
            elif F is not None:
                if q["op"] == G.OP_OR:
                    assert np.array_equal(res["value"], PB.union_n_intersection_count(A, g, F, q["rf"])[0]), (c, qi)
                assert np.array_equal(res["value"], PB.intersection_count(R, np.arange(len(g)), F, q["rf"])), (c, qi)
            else:
                assert np.array_equal(res["value"], cnt), (c, qi)
        elif q["kind"] == "topn":
            per = PB.topk_counts(A, q["ra"], F, q.get("rf"))
            exact = G.topn_model(popc(m, q), per, G.popc_rows(m.W[q["f"]])[q["rf"]] if F is not None else np.zeros(q["n"], np.uint64), F is not None, 0, 0, 0, 0)
            tot = per.sum(axis=0)
            order = sorted((i for i in range(len(tot)) if tot[i]), key=lambda i: (-int(tot[i]), i))
            assert exact == (order, [int(tot[i]) for i in order]), (c, qi)
    assert seen, c


def popc(m, q):
    return G.popc_rows(m.W[q["a"]])[q["ra"]]


def test_every_kind_is_tied_somewhere(walked):
    kinds = {q["kind"] for c, m in walked for q in c.queries if q["refusal"] is None and all(o in m.W for o in c.operands(q))}
    assert kinds >= set(G.KINDS) - {"bsi_sum", "bsi_range_sum", "bsi_range"}


@pytest.mark.parametrize("seed", range(40))
def test_topn_model_equals_pytopn_on_small_sets(seed):
    """topn_model works on (cardinality, count with the source, source size) per row and shard; pytopn works on column sets.  Rows
    as intervals of a small universe give any triple: both semantics, thresholds around the counts, every n up to past the field."""
    rng = np.random.default_rng([0x70b1, seed])
    ns, na, U = int(rng.integers(1, 5)), int(rng.integers(1, 12)), 60
    has_src = bool(rng.random() < 0.7)
    shards, srcs = [], []
    cnt, count, src_n = np.zeros((ns, na), np.uint64), np.zeros((ns, na), np.uint64), np.zeros(ns, np.uint64)
    for s in range(ns):
        src = set(range(int(rng.integers(0, U // 2)), int(rng.integers(U // 2, U)))) if rng.random() < 0.9 else set()
        rows = {}
        for r in range(na):
            lo = int(rng.integers(0, U))
            rows[r] = set(range(lo, min(U, lo + int(rng.choice([0, 1, 2, 5, 20, 40])))))
            if rng.random() < 0.3:
                rows[r] = set(int(x) for x in rng.integers(0, U, int(rng.integers(0, 30))))
            cnt[s, r], count[s, r] = len(rows[r]), len(rows[r] & src) if has_src else len(rows[r])
        shards.append(rows)
        srcs.append(src)
        src_n[s] = len(src)
    for n in (0, 1, 2, max(1, na - 1), na, na + 3):
        for mt, tt in ((0, 0), (1, 0), (3, 0), (12, 0), (0, 10), (0, 35), (0, 80), (4, 50)):
            if tt and not has_src:
                continue
            ss = srcs if has_src else None
            ref = T.execute_topn(shards, n, ss, None, mt, tt)
            got = G.topn_model(cnt, count, src_n, has_src, n, mt, tt, 1)
            assert list(zip(*got)) == ref, ("reference", seed, n, mt, tt)
            got = G.topn_model(cnt, count, src_n, has_src, n, mt, tt, 0)
            assert list(zip(*got)) == T.top_exact(shards, list(range(na)), n, ss, mt, tt), ("exact", seed, n, mt, tt)
            for s in range(ns):
                if shards[s] and 0 < n:
                    ft = sorted(T.fragment_top(shards[s], n, srcs[s] if has_src else None, None, mt or 1, tt))
                    assert sorted(G.fragment_top_counts(cnt[s], count[s], int(src_n[s]), has_src, n, mt or 1, tt)) == ft, ("fragment.top", seed, s, n, mt, tt)


def test_plan_cases(oracle):
    for it in range(6):
        c = G.PlanCase(it)
        m = G.PlanModel(c)
        names = [st[0] for st in c.steps]
        assert "detach" in names and names.index("detach") < len(names) - 1 - names[::-1].index("setop"), "no set-op after the detach"
        for st in c.steps:
            if st[0] in ("total", "total_cell", "read"):
                assert m.counts is not None, c
            if st[0] == "detach":
                assert m.out is not None, c
            m.apply(st)
        assert len(m.detached) >= 1
        A, B = PB.RowSet.from_dense(c.W["X"]), PB.RowSet.from_dense(c.W["Y"])
        assert np.array_equal(m.icounts, PB.intersection_count(A, c.ia, B, c.ib))
        R, cnt = PB.setop(G.OP_XOR, A, c.ia, B, c.ib)
        assert np.array_equal(m.out, R.words()) and np.array_equal(m.counts, cnt)
    all_names = {st[0] for it in range(6) for st in G.PlanCase(it).steps}
    assert all_names >= {"setop", "total", "total_cell", "intersection_count", "intersection_count_total", "intersection_count_accumulate", "read", "detach"}
