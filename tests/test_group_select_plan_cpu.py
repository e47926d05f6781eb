"""CPU check of the host rules of the GroupBy selection stage (featurebase_amd/csrc/fbk_group_select_plan.h, no GPU): the header is
compiled into a stand-alone program (tests/cpp/group_select_check.cpp, -fsanitize=address,undefined, run as a program the way
tests/test_topn_plan_cpu.py runs its checker), fed generated cases and compared with the model of the reference
(groupby_select_ref.py).  The same header is the library's small-input path and the C++ mirror's blocked path."""
import os
import subprocess

import numpy as np
import pytest

import datagen
import groupby_select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX, U64_MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
SUBJECT = {"count": 1, "sum": 2}


@pytest.fixture(scope="module")
def checker():
    out = os.path.join(ROOT, "build", "group_select_check_san")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "group_select_check.cpp"), "-o", out])

    def run(lines):
        r = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"group_select_check exit {r.returncode}\n{r.stderr[-4000:]}"
        got = r.stdout.splitlines()
        assert len(got) == len(lines)
        return got

    return run


def line(counts, aggs, sort=(), having=None, offset=0, limit=None, flags=0, n_sort=None, raw_having=None):
    terms = [(SUBJECT[s], int(d)) for s, d in sort] + [(0, 0), (0, 0)]
    wrap = lambda v: v - (1 << 64) if v > I64_MAX else v
    hv = raw_having if raw_having is not None else ((0, 0, 0, 0) if having is None else (SUBJECT[having[0]], R.OP_CODE[having[1]], wrap(having[2]), wrap(having[3])))
    head = [flags, len(sort) if n_sort is None else n_sort, *terms[0], *terms[1], *hv, offset, U64_MAX if limit is None else limit, int(aggs is not None), len(counts)]
    return " ".join(str(int(x)) for x in head + list(counts) + (list(aggs) if aggs is not None else []))


def cases():
    rng = datagen.rng_for(9320)
    sorts = [()] + [((s, d),) for s in ("count", "sum") for d in (False, True)] + [
        ((s0, d0), (s1, d1)) for s0, s1 in (("count", "sum"), ("sum", "count")) for d0 in (False, True) for d1 in (False, True)]
    out = []
    for n in (0, 1, 2, 7, 64, 65, 300):
        for kind in range(4):
            if kind == 0:
                counts, aggs = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint64), n), rng.integers(-2, 3, n).astype(np.int64)
            elif kind == 1:
                counts, aggs = rng.integers(1, 4, n).astype(np.uint64), rng.choice(np.array([I64_MIN, -1, 0, 1, I64_MAX], dtype=np.int64), n)
            elif kind == 2:
                counts = rng.choice(np.array([0, 1, I64_MAX, 1 << 63, (1 << 63) + 1, U64_MAX], dtype=np.uint64), n)
                aggs = rng.integers(-2, 3, n).astype(np.int64)
            else:
                counts, aggs = np.full(n, 7, dtype=np.uint64), np.full(n, -5, dtype=np.int64)
            for _ in range(24):
                sort = sorts[int(rng.integers(len(sorts)))]
                having = None
                if rng.integers(3) and n:
                    subject = ("count", "sum")[int(rng.integers(2))]
                    src = counts if subject == "count" else aggs
                    lo, hi = sorted(int(v) for v in rng.choice(src, 2))
                    if rng.integers(8) == 0:
                        lo, hi = hi, lo  # lo > hi selects nothing (the BETWEEN forms)
                    having = (subject, R.OPS[int(rng.integers(len(R.OPS)))], lo, hi)
                offset = [0, 0, 1, 3, n, n + 2, U64_MAX][int(rng.integers(7))]
                limit = [None, 0, 1, 5, n, U64_MAX][int(rng.integers(6))]
                with_aggs = bool(rng.integers(4)) or any(s == "sum" for s, _ in sort) or (having is not None and having[0] == "sum")
                out.append((counts, aggs if with_aggs else None, sort, having, offset, limit))
    return out


def test_the_host_selection_matches_the_model(checker):
    cs = cases()
    got = checker([line(*c) for c in cs])
    sorted_n = limited = 0
    for c, g in zip(cs, got):
        counts, aggs, sort, having, offset, limit = c
        exp, matched = R.select(counts, aggs, sort, having, offset, limit)
        assert [int(x) for x in g.split()] == [matched, len(exp)] + exp, (sort, having, offset, limit, counts.tolist())
        sorted_n += bool(sort) and len(exp) > 1
        limited += bool(sort) and 0 < len(exp) < matched
    assert sorted_n > 50 and limited > 20  # the generator reaches the partial sort


def test_the_argument_rules(checker):
    c, a = [1, 2, 3], [4, 5, 6]
    bad = [
        (line(c, a, flags=4), "unknown flag"),
        (line(c, a, flags=3), "both path flags"),
        (line(c, a, sort=[("count", 1)], n_sort=3), "more than two sort terms"),
        (line(c, a, sort=[("count", 1), ("count", 0)]), "the same sort subject twice"),
        (line(c, None, sort=[("sum", 1)]), "sort on the aggregate of a call without one"),
        (line(c, None, having=("sum", "gt", 1, 0)), "having on the aggregate of a call without one"),
        (line(c, a, raw_having=(1, 0, 0, 0)), "unknown having op"),
        (line(c, a, raw_having=(1, 11, 0, 0)), "unknown having op"),
        (line(c, a, raw_having=(3, 1, 0, 0)), "unknown having subject"),
        (line(c, a, sort=[("count", 2)]), "unknown sort direction"),
    ]
    got = checker([l for l, _ in bad])
    for (l, what), g in zip(bad, got):
        assert g == "E " + what, l
    assert checker([line(c, a, flags=1), line(c, a, flags=2, sort=[("sum", True)])]) == ["3 3 0 1 2", "3 3 2 1 0"]
