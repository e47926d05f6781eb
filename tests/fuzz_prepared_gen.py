"""Case generator and model of the structural fuzz of the prepared forms (fbk_query_*, fbk_plan_*): the part of the ABI that keeps
state between launches.  tests/test_gpu_fuzz_prepared.py executes the cases on the GPU, tests/test_fuzz_prepared_cpu.py checks the
generator and the model without one.  No GPU in here.

A case (Case(it), from datagen.rng_for(7400, it)) is a WORLD, QUERIES and a SCHEDULE.

World: two or three static batches S0, S1, S2 — rows of every container archetype as in tests/test_gpu_fuzz_struct.py's make_batch
(missing-slot probability from {0, 0.15, 0.6, 0.95}, 5 % empty rows), 4 .. 40 rows each; every third iteration S1 has 66 .. 70 rows so that
a BSI fragment of depth 64 fits.  Every fourth iteration (it % 4 == 3) uploads them dense.  Two batches change under live queries:
  O  the output of a plan over pairs (S0[ia], S1[ib]): `mutate` re-runs the plan with another operation (and flags), which rewrites
     O in place.  Row 0 of S0 holds containers in slots 0 .. 7 only and row 0 of S1 in slots 8 .. 15 only, and pair 0 is (0, 0): OR
     and XOR fill all 16 slots of O's row 0, AND empties them all, whatever the seed;
  C  a one-shot fbk_setop result without FBK_SETOP_OPTIMIZE (8 KiB cells) that the caller owns: `compact` moves it into a
     right-sized arena with a new slot table (fbk_batch_compact), content unchanged, version bumped.  Nine of its 12 .. 20 rows are
     pairs of empty rows (row 1 of S0 and of S1), so that the first compact of an encoded world always moves it.

Queries: the seven single-context kinds (KINDS).  An operand is a static batch, O, C, or the output of an earlier row-valued query
of the case ("q<i>": a chain).  Row lists are rng.integers with repeats; a BSI kind reads any depth + 2 consecutive rows of its batch
as a fragment (arbitrary planes, bits outside the exists row), depth 1 .. 64 cut to what the batch holds.

Schedule: steps {"do": prepare | run | read | mutate | compact | set_option | oneshot | free}.  The structure a default run must
cover does not depend on the seed: PLAN[it % 6] names the scenarios an iteration plays first (a chain of depth 2, the mutable batch as
a filter, a row-valued query re-run after its input lost a slot, compact under a live query, keep_per_shard at matrix_pass_kb = 4, a
TopN whose pass is shorter than its shards, accumulate into a caller cell, a stale read), two kinds are dealt by the iteration number,
then a refused run and a refused prepare, 4 .. 7 random steps, a one-shot call, a free and a prepare under the live queries, and runs of
what is still live: about 40 steps (at most 50), 4 .. 10 queries a case.

Model: mirrors every step on numpy words and gives the expectation of the step.  Counts are set algebra with np.bitwise_count; BSI
results come from oracle/pybatch.py on the model's current words; TopN is fragment.top's walk on counts (topn_model), tied to
oracle/pytopn.py by the CPU test.  A query's results are those of its last run: a read after a mutation without a re-run gives the
old answer.  A refusal is an expectation too: the generator predicts every FBK_E_INVALID from host-only checks (a query's `refusal`, run_refusal, the option a plan's FBK_SETOP_OPTIMIZE needs), any
other error fails the test."""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np

import datagen as D

ITERS = int(os.environ.get("FBK_FUZZ_ITERS", "6"))
KINDS = ("count_matrix", "fold_icount", "bsi_sum", "bsi_range_sum", "bsi_range", "fold", "topn")
ROW_KINDS = ("bsi_range", "fold")
COUNT_KINDS = ("count_matrix", "fold_icount")  # the kinds FBK_QUERY_ACCUMULATE applies to
OP_AND, OP_OR, OP_XOR, OP_ANDNOT = 0, 1, 2, 3
OPTIMIZE = 1
CELL_FILL = 5  # what every caller cell holds before its first run
NP_OPS = {OP_AND: np.bitwise_and, OP_OR: np.bitwise_or, OP_XOR: np.bitwise_xor, OP_ANDNOT: lambda a, b: a & ~b}
DEFAULTS = {"matrix_fused": -1, "matrix_spb": 0, "matrix_pass_kb": 1 << 20, "matrix_shadow": 1, "matrix_shadow_array": 2048, "matrix_shadow_run": 0,
            "topk_device_sort": -1, "setop_direct_encode": 2, "topn_semantics": 1}
SHADOW_MODES = [(1, 2048, 0), (1, 64, 0), (0, 2048, 0), (1, 2048, 20)]  # the shadow_mode fixture of tests/test_gpu_queries.py
OPTION_DRAWS = {"matrix_fused": [-1, 0, 1], "matrix_spb": [0, 1, 2, 4, 8, 16], "matrix_pass_kb": [4, 64, 1 << 20], "topk_device_sort": [-1, 0, 1],
                "setop_direct_encode": [0, 1, 2], "topn_semantics": [0, 1]}

# the scenarios iteration it plays first (it % 6): six iterations cover every one of them for every seed
PLAN = [
    ("chain2",),
    ("filter_mutable", "empty_slot_rerun"),
    ("compact_live", "kps_pass4"),
    ("topn_pass", "acc_stale"),
    ("empty_slot_rerun", "acc_stale"),
    ("compact_live", "filter_mutable"),
]

popc_rows = lambda w: np.bitwise_count(w).reshape(w.shape[0], -1).sum(axis=1).astype(np.uint64)  # noqa: E731


# ---- references on words ---------------------------------------------------------------------------------------------------------
def fold_np(op: int, W: np.ndarray, groups: np.ndarray) -> np.ndarray:
    """[n_groups, 16, 1024]: row g = W[groups[g, 0]] <op> W[groups[g, 1]] ... folded left to right"""
    out = np.empty((groups.shape[0], 16, 1024), dtype=np.uint64)
    for g, ids in enumerate(groups):
        acc = W[ids[0]].copy()
        for i in ids[1:]:
            acc = NP_OPS[op](acc, W[i])
        out[g] = acc
    return out


def count_matrix_np(WA, ra, WB, rb, WF=None, rf=None) -> np.ndarray:
    """per-shard matrices [n_shards, n_a, n_b]: |A_i ∩ F ∩ B_j|"""
    ns, na = ra.shape
    nb = rb.shape[1]
    out = np.zeros((ns, na, nb), dtype=np.uint64)
    for s in range(ns):
        a = WA[ra[s]].reshape(na, -1)
        if WF is not None:
            a = a & WF[rf[s]].reshape(1, -1)
        b = WB[rb[s]].reshape(nb, -1)
        for j in range(nb):
            out[s, :, j] = np.bitwise_count(a & b[j]).sum(axis=1)
    return out


def fragment_top_counts(cnt, count, src_n: int, has_src: bool, n: int, min_threshold: int, tanimoto_threshold: int, ids=None):
    """fragment.top (fragment.go:1317-1437) of ONE shard as oracle/pytopn.fragment_top walks it, on numbers instead of column sets:
    cnt[r] = the row's cardinality, count[r] = |row ∩ src| (= cnt[r] without a source row).  The rule of one row is
    pytopn.row_passes, the heap pytopn's; tests/test_fuzz_prepared_cpu.py compares the walk with fragment_top on real sets."""
    from oracle import pytopn as T

    rows = range(len(cnt)) if ids is None else ids
    pairs = sorted(((r, int(cnt[r])) for r in rows if cnt[r] > 0), key=lambda p: (-p[1], p[0]))
    if ids is not None:
        n = 0
    tanimoto = tanimoto_threshold if (tanimoto_threshold > 0 and has_src) else 0
    results: list = []
    for r, c in pairs:
        if tanimoto:  # the cardinality part of the rule comes before the heap (:1343-1362)
            if c * 100 <= src_n * tanimoto or c * tanimoto >= src_n * 100:
                continue
        elif c < min_threshold:
            continue
        if n == 0 or len(results) < n:
            if not T.row_passes(c, int(count[r]), src_n, has_src, min_threshold, tanimoto_threshold):  # (the part that needs the count)
                continue
            T.heap_push(results, (r, int(count[r])))
            if n > 0 and len(results) == n and not has_src:
                break
            continue
        threshold = results[0][1]
        if threshold < min_threshold or c < threshold:
            break
        if int(count[r]) < threshold:
            continue
        T.heap_push(results, (r, int(count[r])))
    return results


def topn_model(cnt, count, src_n, has_src: bool, n: int, min_threshold: int, tanimoto_threshold: int, semantics: int):
    """cnt, count [n_shards, n_a], src_n [n_shards] -> (indexes, counts): count descending, index ascending, zeros dropped, the first n.
    semantics 0: pytopn.top_exact's rule on every row of every shard; 1: pytopn.execute_topn's two passes (candidates per shard)."""
    from oracle import pytopn as T

    ns, na = cnt.shape
    mt = min_threshold
    ids = None
    if semantics == 1:
        mt = mt or T.DEFAULT_MIN_THRESHOLD
        if 0 < n < na:
            cand = set()
            for s in range(ns):
                cand |= {r for r, _ in fragment_top_counts(cnt[s], count[s], int(src_n[s]), has_src, n, mt, tanimoto_threshold)}
            ids = sorted(cand)
    tot = np.zeros(na, dtype=np.uint64)
    for s in range(ns):
        for r in (range(na) if ids is None else ids):
            if T.row_passes(int(cnt[s, r]), int(count[s, r]), int(src_n[s]), has_src, mt, tanimoto_threshold):
                tot[r] += count[s, r]
    order = sorted((i for i in range(na) if tot[i]), key=lambda i: (-int(tot[i]), i))
    if n:
        order = order[:n]
    return order, [int(tot[i]) for i in order]


def range_sum_plan(op: int, depth: int, pred: int):
    """fbk_bsi_range_sum_plan (host arithmetic of libfbk.so, no GPU): None when the one-pass Sum(Range) does not serve the predicate,
    else scan_positive (the sign of the raw records fbk_query_run leaves in a caller buffer)"""
    import ctypes as C

    from featurebase_amd import lib as L

    act, vhi, sp, to = (C.c_uint8 * 64)(), (C.c_uint64 * 64)(), C.c_uint32(), C.c_uint32()
    rc = L.load().fbk_bsi_range_sum_plan(op, depth, C.c_int64(pred), act, vhi, C.byref(sp), C.byref(to))
    assert rc in (0, 1), rc
    return None if rc else bool(sp.value)


def run_refusal(kind: str, dest: str, acc: bool) -> Optional[str]:
    """why fbk_query_run refuses (FBK_E_INVALID), or None"""
    if acc and kind not in COUNT_KINDS:
        return "accumulate on a kind that refuses it"
    if kind == "topn" and dest == "cell":
        return "a TopN writes its own buffers"
    return None


def cell_words(q: dict) -> int:
    """uint64 words of the caller buffer a run of q may be given"""
    k = q["kind"]
    if k == "count_matrix":
        return q["ra"].shape[1] * q["rb"].shape[1]
    return q["n"] * {"bsi_sum": 3, "bsi_range_sum": 4}.get(k, 1) if k != "topn" else q["ra"].shape[1]


# ---- the world -------------------------------------------------------------------------------------------------------------------
def _rows_words(rows) -> np.ndarray:
    W = np.zeros((len(rows), 16, 1024), dtype=np.uint64)
    for r, row in enumerate(rows):
        for k, c in row.items():
            W[r, k & 15] = c.words()
    return W


def _static_batch(rng, n_rows: int, dense: bool, slots_of_row0):
    """-> (rows or None, words): rows = {slot: oracle container} per row for the encoded upload; row 0 holds something in every slot of
    slots_of_row0 and nothing elsewhere, row 1 is empty"""
    if dense:
        W = rng.integers(0, 1 << 63, (n_rows, 16, 1024), dtype=np.uint64) & rng.integers(0, 1 << 63, (1, 16, 1024), dtype=np.uint64)
        W[rng.random(n_rows) < 0.05] = 0
        W[0] = rng.integers(0, 1 << 63, (16, 1024), dtype=np.uint64) | np.uint64(1)
        W[0, [s for s in range(16) if s not in slots_of_row0]] = 0
        W[1] = 0
        return None, W
    p_missing = float(rng.choice([0.0, 0.15, 0.6, 0.95]))
    rows = [D.random_row(rng, 0, p_missing) if rng.random() > 0.05 else {} for _ in range(n_rows)]
    kinds = [k for k in D.KINDS if k != "empty_array"]
    rows[0] = {s: D.oracle_container(rng, kinds[int(rng.integers(0, len(kinds)))]) for s in slots_of_row0}
    rows[1] = {}
    return rows, _rows_words(rows)


class Case:
    def __init__(self, it: int):
        self.it = it
        self.rng = rng = D.rng_for(7400, it)
        self.dense = it % 4 == 3
        self.plan_names = PLAN[it % 6]
        # -- world
        self.size: Dict[str, int] = {}
        self.rows: Dict[str, Optional[list]] = {}
        self.W0: Dict[str, np.ndarray] = {}  # the words every batch starts with
        n_static = 2 + int(rng.random() < 0.5)
        for i in range(n_static):
            n = int(rng.integers(4, 41))
            if i == 1 and it % 3 == 1:
                n = int(rng.integers(66, 71))
            self.rows[f"S{i}"], self.W0[f"S{i}"] = _static_batch(rng, n, self.dense, range(0, 8) if i == 0 else range(8, 16) if i == 1 else range(16))
            self.size[f"S{i}"] = n
        self.statics = [f"S{i}" for i in range(n_static)]
        n_o, n_c = int(rng.integers(4, 25)), int(rng.integers(12, 21))
        self.ia, self.ib = rng.integers(0, self.size["S0"], n_o), rng.integers(0, self.size["S1"], n_o)
        self.ia[0] = self.ib[0] = 0
        self.op0 = int(rng.integers(0, 4))
        self.ja, self.jb = rng.integers(0, self.size["S0"], n_c), rng.integers(0, self.size["S1"], n_c)
        self.ja[1:10] = self.jb[1:10] = 1  # nine rows of nothing: 144 nil cells, more than the 1 MiB below which compact leaves a batch alone
        self.opc = int(rng.choice([OP_OR, OP_XOR, OP_ANDNOT, OP_AND]))
        self.size["O"], self.size["C"] = n_o, n_c
        self.W0["O"] = NP_OPS[self.op0](self.W0["S0"][self.ia], self.W0["S1"][self.ib])
        self.W0["C"] = NP_OPS[self.opc](self.W0["S0"][self.ja], self.W0["S1"][self.jb])
        # -- queries and schedule
        self.queries: List[dict] = []
        self.steps: List[dict] = []
        _Builder(self).build()

    def __repr__(self):
        return f"Case(seed {D.SEED:#x}, it {self.it}, {'dense' if self.dense else 'encoded'}, {len(self.queries)} queries, {len(self.steps)} steps)"

    def operands(self, q: dict) -> List[str]:
        return [q[x] for x in ("a", "b", "f") if q.get(x) is not None]

    def depth_of(self, name: str) -> int:
        """0 for a batch of the world, 1 + the deepest operand for the output of a query"""
        if not name.startswith("q"):
            return 0
        return 1 + max(self.depth_of(o) for o in self.operands(self.queries[int(name[1:])]))

    def describe(self, si: int) -> str:
        st = self.steps[si]
        kind = self.queries[st["q"]]["kind"] if "q" in st else "-"
        return f"seed {D.SEED:#x} it {self.it} step {si} kind {kind}: {({k: v for k, v in st.items()})}"


class _Builder:
    """Draws the queries and the schedule of a case, tracking what the library's state will be (live queries, which have run, whose
    own buffer holds a value, the options in force) as far as the next draw depends on it."""

    def __init__(self, case: Case):
        self.c, self.rng = case, case.rng
        self.live: set = set()
        self.ran: set = set()
        self.own: set = set()  # queries whose own result buffer holds the result of a run
        self.opts = dict(DEFAULTS)
        self.refused_range_sums = 0

    # -- draws
    def small(self, lo=1, hi=41, big=(33, 71)) -> int:
        return int(self.rng.integers(lo, hi)) if self.rng.random() < 0.8 else int(self.rng.integers(*big))

    def pick(self, min_rows: int = 1, exclude=()) -> str:
        """a batch for an operand: a static one, O, C or the output of a live row-valued query that has run"""
        rng, c = self.rng, self.c
        outs = [f"q{i}" for i in sorted(self.live & self.ran) if c.queries[i]["kind"] in ROW_KINDS]
        for _ in range(50):
            r = rng.random()
            name = "O" if r < 0.25 else "C" if r < 0.4 else outs[int(rng.integers(0, len(outs)))] if (r < 0.6 and outs) else c.statics[int(rng.integers(0, len(c.statics)))]
            if c.size[name] >= min_rows and name not in exclude:
                return name
        return "S1" if c.size["S1"] >= min_rows else "S0"

    def predicate(self, depth: int) -> int:
        rng = self.rng
        lim = (1 << min(depth, 63)) - 1
        some = [0, 1, -1, lim, -lim, lim + 1 if lim < (1 << 62) else lim,
                int(rng.integers(-lim, lim + 1)) if lim < (1 << 62) else int(rng.integers(-(1 << 62), 1 << 62))]
        return some[int(rng.integers(0, len(some)))]

    def new_query(self, kind: str, a: Optional[str] = None, f: Optional[str] = None, **over) -> dict:
        rng, c = self.rng, self.c
        q: dict = {"kind": kind, "a": None, "b": None, "f": None, "refusal": None}
        want_f = f is not None
        if kind == "count_matrix":
            ns, na, nb = int(rng.integers(1, 7)), self.small(), int(rng.integers(1, 41))
            topk_shape = over.get("topk", (not want_f) and rng.random() < 0.25 and "nb" not in over)
            if topk_shape:
                nb = 1
            na, nb, ns = over.get("na", na), over.get("nb", nb), over.get("ns", ns)
            while ns * na * nb > 6000:  # (the numpy reference walks every pair)
                ns, nb = (ns - 1, nb) if ns > 3 else (ns, max(2, nb // 2))
            q["a"] = a or self.pick()
            q["b"] = q["a"] if rng.random() < 0.5 else self.pick()
            q["ra"], q["rb"] = rng.integers(0, c.size[q["a"]], (ns, na)), rng.integers(0, c.size[q["b"]], (ns, nb))
            if want_f or (not topk_shape and rng.random() < 0.7):
                q["f"] = f or self.pick()
            q["n"], q["keep"] = ns, bool(over.get("keep", rng.random() < 0.4))
        elif kind in ("fold_icount", "fold"):
            g = over.get("g", int(rng.integers(1, 7)))
            k = over.get("k", int(rng.integers(1, 9)) if rng.random() < 0.8 else int(rng.integers(65, 81)))
            q["a"] = a or self.pick()
            q["op"] = over.get("op", int(rng.integers(0, 4)))
            q["groups"] = rng.integers(0, c.size[q["a"]], (g, k))
            q["n"] = g
            if kind == "fold":
                q["flags"] = over.get("flags", OPTIMIZE if rng.random() < 0.5 else 0)
            elif want_f or rng.random() < 0.6:
                q["f"] = f or self.pick()
        elif kind in ("bsi_sum", "bsi_range_sum", "bsi_range"):
            q["a"] = a or self.pick(min_rows=3)
            size = c.size[q["a"]]
            depth = min(over.get("depth", int(rng.integers(1, 65))), size - 2)
            ns = over.get("ns", int(rng.integers(1, 7)))
            q["depth"], q["n"] = depth, ns
            q["base"] = rng.integers(0, size - depth - 1, ns)
            if kind != "bsi_range" and (want_f or rng.random() < 0.6):
                q["f"] = f or self.pick()
            if kind != "bsi_sum":
                q["op"], q["pred"] = int(rng.integers(1, 7)), self.predicate(depth)
            if kind == "bsi_range_sum":
                for _ in range(60):  # at most one refused Sum(Range) a case: the predicate is drawn again after that
                    if range_sum_plan(q["op"], depth, q["pred"]) is not None or (self.refused_range_sums == 0 and not over.get("served")):
                        break
                    q["op"], q["pred"] = int(rng.integers(1, 7)), self.predicate(depth)
                sp = range_sum_plan(q["op"], depth, q["pred"])
                if sp is None:
                    self.refused_range_sums += 1
                    q["refusal"] = "the one-pass Sum(Range) does not serve the predicate"
                q["scan_positive"] = sp
        elif kind == "topn":
            ns, na = over.get("ns", int(rng.integers(1, 7))), over.get("na", self.small())
            q["a"] = a or self.pick()
            q["ra"] = rng.integers(0, c.size[q["a"]], (ns, na))
            if want_f or rng.random() < 0.7:
                q["f"] = f or self.pick()
            q["n"] = ns
            q["top"] = int(rng.choice([0, 1, int(rng.integers(1, na + 3))]))
            q["mt"] = int(rng.choice([0, 0, int(rng.integers(1, 200)), int(rng.integers(200, 30000))]))
            q["tt"] = int(rng.choice([0, 0, int(rng.integers(1, 101))])) if q["f"] else 0
        else:
            raise ValueError(kind)
        if q["f"] is not None:
            q["rf"] = rng.integers(0, c.size[q["f"]], q["n"])
            if q["f"] == "O" and "rf0" in over:
                q["rf"][0] = 0
        return q

    # -- steps
    def emit(self, **st) -> None:
        self.c.steps.append(st)

    def prepare(self, q: dict) -> int:
        qi = len(self.c.queries)
        self.c.queries.append(q)
        if q["kind"] in ROW_KINDS:
            self.c.size[f"q{qi}"] = q["n"]
        self.emit(do="prepare", q=qi)
        if q["refusal"] is None:
            self.live.add(qi)
        return qi

    def run(self, qi: int, dest: Optional[str] = None, acc: Optional[bool] = None) -> None:
        rng, kind = self.rng, self.c.queries[qi]["kind"]
        if dest is None:
            dest = "cell" if rng.random() < 0.35 else "own"
            if kind == "topn" and rng.random() < 0.85:
                dest = "own"
        if acc is None:
            acc = rng.random() < (0.35 if kind in COUNT_KINDS else 0.08)
            if acc and dest == "own" and qi not in self.own:
                acc = False  # (nothing to add to yet: the query's own buffer is not zeroed at prepare)
        self.emit(do="run", q=qi, dest=dest, acc=bool(acc))
        if run_refusal(kind, dest, acc) is None:
            self.ran.add(qi)
            if dest == "own":
                self.own.add(qi)

    def read(self, qi: int) -> None:
        self.emit(do="read", q=qi)

    def mutate(self, op: Optional[int] = None, flags: Optional[int] = None) -> None:
        rng = self.rng
        op = int(rng.integers(0, 4)) if op is None else op
        if flags is None:
            flags = OPTIMIZE if rng.random() < 0.5 else 0
        self.emit(do="mutate", op=op, flags=flags)

    def set_option(self, **opts) -> None:
        self.opts.update(opts)
        self.emit(do="set_option", opts=dict(opts))

    def deps_live(self, qi: int) -> bool:
        return all((not o.startswith("q")) or int(o[1:]) in self.live for o in self.c.operands(self.c.queries[qi]))

    def dependants(self, qi: int) -> List[int]:
        return [j for j in self.live if f"q{qi}" in self.c.operands(self.c.queries[j])]

    # -- scenarios
    def chain2(self) -> None:
        """fold -> BSI Range over the fold's rows -> a count over the Range's rows as a filter; the upstream re-run under them"""
        rng = self.rng
        q0 = self.prepare(self.new_query("fold", a="O" if rng.random() < 0.5 else None, g=int(rng.integers(5, 7)), op=int(rng.choice([OP_OR, OP_XOR, OP_ANDNOT]))))
        self.run(q0, "own", False)
        q1 = self.prepare(self.new_query("bsi_range", a=f"q{q0}", ns=int(rng.integers(1, 4))))
        self.run(q1, "own", False)
        q2 = self.prepare(self.new_query(str(rng.choice(["count_matrix", "topn", "fold_icount"])), f=f"q{q1}"))
        self.run(q2, "own", False)
        q3 = self.prepare(self.new_query("fold", a=f"q{q1}"))  # Range output -> a of a fold
        self.run(q3, "own", False)
        self.mutate()
        self.run(q0, "own", False)  # the upstream alone: the downstream queries stay prepared, their results those of their last runs
        self.read(q2)
        self.run(q1, "own", False)
        self.run(q2)
        self.read(q2)
        self.run(q3, "own", False)
        self.read(q3)

    def filter_mutable(self) -> None:
        """the mutable batch as the filter of a count matrix on the kernel with the kept program"""
        self.set_option(matrix_fused=1)
        q = self.prepare(self.new_query("count_matrix", f="O", rf0=True, nb=int(self.rng.integers(2, 41)), keep=bool(self.rng.random() < 0.5),
                                        a=self.c.statics[int(self.rng.integers(0, len(self.c.statics)))]))
        self.run(q, "own", False)
        self.read(q)
        self.mutate(OP_AND if self.rng.random() < 0.5 else OP_ANDNOT, 0)
        self.run(q, "own", False)
        self.read(q)
        self.mutate(OP_OR, None)
        self.run(q)
        self.read(q)

    def empty_slot_rerun(self) -> None:
        """a materialised fold over the mutable batch whose group 0 is O's row 0: 16 containers after OR, none after AND"""
        q = self.new_query("fold", a="O", op=OP_OR, k=int(self.rng.integers(1, 5)))
        q["groups"][0, :] = 0
        qi = self.prepare(q)
        self.mutate(OP_OR if self.rng.random() < 0.5 else OP_XOR, None)
        self.run(qi, "own", False)
        self.read(qi)
        self.mutate(OP_AND, None if self.opts["setop_direct_encode"] == 2 else 0)
        self.run(qi, "own", False)
        self.read(qi)

    def compact_live(self) -> None:
        kind = str(self.rng.choice(["count_matrix", "fold_icount", "topn", "fold", "bsi_sum"]))
        q = self.prepare(self.new_query(kind, a="C", f="C" if kind in ("count_matrix", "fold_icount", "topn") and self.rng.random() < 0.5 else None))
        self.run(q, "own", False)
        self.read(q)
        self.emit(do="compact")
        self.run(q)
        self.read(q)

    def kps_pass4(self) -> None:
        """per-shard matrices of more than one 4 KiB pass; and a query whose pass buffer grows when the option is raised"""
        self.set_option(matrix_pass_kb=4)
        q = self.prepare(self.new_query("count_matrix", keep=True, ns=int(self.rng.integers(3, 7)), na=int(self.rng.integers(12, 30)), nb=int(self.rng.integers(12, 30))))
        p = self.prepare(self.new_query("count_matrix", keep=False, ns=int(self.rng.integers(3, 7)), na=int(self.rng.integers(12, 30)), nb=int(self.rng.integers(12, 30))))
        self.run(q, "own", False)
        self.run(p, "own", False)
        self.read(q)
        self.read(p)
        self.set_option(matrix_pass_kb=1 << 20)
        self.run(p)
        self.run(q)
        self.read(p)
        self.read(q)

    def topn_pass(self) -> None:
        """a TopN prepared while a pass holds fewer shards than the query has; options it captured changed before its later runs"""
        self.set_option(matrix_pass_kb=4)
        q = self.prepare(self.new_query("topn", ns=6, na=int(self.rng.integers(100, 131))))
        self.run(q, "own", False)
        self.read(q)
        self.set_option(matrix_pass_kb=1 << 20, topn_semantics=1 - self.opts["topn_semantics"])
        self.run(q, "own", False)
        self.read(q)

    def acc_stale(self) -> None:
        """a count over the mutable batch: accumulated twice into a caller cell, read stale after a mutation, run again"""
        kind = str(self.rng.choice(COUNT_KINDS))
        q = self.prepare(self.new_query(kind, a="O"))
        self.run(q, "cell", True)
        self.run(q, "cell", True)
        self.read(q)
        self.mutate()
        self.read(q)  # stale: the result of the run before the mutation
        self.run(q, "own", False)
        self.read(q)

    def random_step(self) -> None:
        rng, c = self.rng, self.c
        r = rng.random()
        runnable = sorted(i for i in self.live if self.deps_live(i))
        if r < 0.3 and runnable:
            qi = int(rng.choice(runnable))
            self.run(qi)
            if qi in self.ran and rng.random() < 0.7:
                self.read(qi)
        elif r < 0.45 and (self.live & self.ran):
            self.read(int(rng.choice(sorted(self.live & self.ran))))
        elif r < 0.55:
            self.mutate()
        elif r < 0.6:
            self.emit(do="compact")
        elif r < 0.7:
            if rng.random() < 0.3:
                m = SHADOW_MODES[int(rng.integers(0, len(SHADOW_MODES)))]
                self.set_option(matrix_shadow=m[0], matrix_shadow_array=m[1], matrix_shadow_run=m[2])
            else:
                name = sorted(OPTION_DRAWS)[int(rng.integers(0, len(OPTION_DRAWS)))]
                self.set_option(**{name: int(rng.choice(OPTION_DRAWS[name]))})
        elif r < 0.8:
            ok = [i for i, q in enumerate(c.queries) if q["refusal"] is None and self.deps_live(i)]
            if ok:
                self.emit(do="oneshot", q=int(rng.choice(ok)))
        elif r < 0.87:
            free = [i for i in sorted(self.live) if not self.dependants(i)]
            if free:
                qi = int(rng.choice(free))
                self.emit(do="free", q=qi)
                self.live.discard(qi)
        elif r < 0.92:
            self.refused_prepare()
        elif len(self.live) < 8:
            qi = self.prepare(self.new_query(KINDS[int(rng.integers(0, len(KINDS)))]))
            if qi in self.live:
                self.run(qi)

    def refused_prepare(self) -> None:
        if self.rng.random() < 0.5:
            q = self.new_query("fold", op=OP_AND, k=0)
            q["refusal"] = "Intersect of no rows"
        else:
            q = self.new_query("fold", flags=2)
            q["refusal"] = "unknown flag"
        self.prepare(q)

    def build(self) -> None:
        c, rng = self.c, self.rng
        for name in c.plan_names:
            getattr(self, name)()
        for j in range(2):  # two kinds by the iteration number: 0 .. 11 mod 7 over six iterations
            kind = KINDS[(2 * c.it + j) % len(KINDS)]
            deep = kind.startswith("bsi") and c.size["S1"] >= 66  # the deep planes: a fragment of more than 40 bits in the large batch
            qi = self.prepare(self.new_query(kind, served=True, topk=True, **({"a": "S1", "depth": int(rng.integers(41, 65))} if deep else {})))
            if kind in ("bsi_sum", "bsi_range_sum"):
                self.run(qi, "cell", False)  # the raw per-shard records into a caller buffer, read back through it
            else:
                self.run(qi)
            if qi in self.ran:
                self.read(qi)
        # refusals: a run the kind refuses, after which the query still reads its last result; every other case a prepare
        no_acc = [i for i in sorted(self.live & self.ran) if c.queries[i]["kind"] not in COUNT_KINDS and self.deps_live(i)]
        if no_acc:
            qi = int(rng.choice(no_acc))
            self.run(qi, "cell" if c.queries[qi]["kind"] == "topn" and rng.random() < 0.5 else "own", c.queries[qi]["kind"] != "topn" or bool(rng.random() < 0.5))
            if run_refusal(c.queries[qi]["kind"], c.steps[-1]["dest"], c.steps[-1]["acc"]) is None:  # (a TopN into its own buffer)
                self.run(qi, "cell", True)
            self.read(qi)
        if c.it % 2 == 0:
            self.refused_prepare()
        for _ in range(int(rng.integers(4, 8))):  # arbitrary order: runs, reads, mutations, options, one-shot calls, frees, prepares
            self.random_step()
        while len(c.steps) < 12:
            self.random_step()
        # whatever was drawn: a one-shot call between the runs of live queries, and a free + prepare under them (pool blocks recycled)
        ok = [i for i, q in enumerate(c.queries) if q["refusal"] is None and self.deps_live(i)]
        self.emit(do="oneshot", q=int(rng.choice(ok)))
        free = [i for i in sorted(self.live) if not self.dependants(i)]
        qi = int(rng.choice(free))
        self.emit(do="free", q=qi)
        self.live.discard(qi)
        qi = self.prepare(self.new_query(KINDS[int(rng.integers(0, len(KINDS)))], served=True))
        self.run(qi, "own", False)
        self.read(qi)
        again = [i for i in sorted(self.live & self.ran) if self.deps_live(i)]
        for i in sorted(rng.permutation(again)[:3].tolist()):
            self.run(i)
            if run_refusal(c.queries[i]["kind"], c.steps[-1]["dest"], c.steps[-1]["acc"]) is None:
                self.read(i)
        n_q = len([q for q in c.queries if q["refusal"] is None])
        while n_q < 4:  # 4 .. 8 queries a case
            qi = self.prepare(self.new_query(KINDS[int(rng.integers(0, len(KINDS)))]))
            if qi in self.live:
                n_q += 1
                self.run(qi, "own", False)
                self.read(qi)


# ---- the model -------------------------------------------------------------------------------------------------------------------
class Model:
    """The state the library must be in after every step of a case, on numpy words.  apply(step) -> the step's expectation."""

    def __init__(self, case: Case):
        self.c = case
        self.W = {k: v.copy() for k, v in case.W0.items()}
        self.ver = {k: 0 for k in self.W}
        self.opts = dict(DEFAULTS)
        self.qs: Dict[int, dict] = {}
        self.cov: set = set()
        self._eval: dict = {}
        self._rs: dict = {}

    # -- evaluation of a query on the current words
    def rowset(self, name: str):
        from oracle import pybatch as PB

        key = (name, self.ver[name])
        if key not in self._rs:
            self._rs = {k: v for k, v in self._rs.items() if k[0] != name}
            self._rs[key] = PB.RowSet.from_dense(self.W[name])
        return self._rs[key]

    def versions(self, q: dict):
        return tuple(self.ver[o] for o in self.c.operands(q))

    def evaluate(self, qi: int, semantics: int) -> dict:
        q = self.c.queries[qi]
        key = (qi, self.versions(q), semantics if q["kind"] == "topn" else 0)
        if key not in self._eval:
            self._eval[key] = self._evaluate(q, semantics)
        return self._eval[key]

    def _evaluate(self, q: dict, semantics: int) -> dict:
        from oracle import pybatch as PB

        kind, W = q["kind"], self.W
        WF = W[q["f"]] if q["f"] is not None else None
        if kind == "count_matrix":
            ps = count_matrix_np(W[q["a"]], q["ra"], W[q["b"]], q["rb"], WF, q.get("rf"))
            return {"value": ps.sum(axis=0), "ps": ps}
        if kind in ("fold", "fold_icount"):
            out = fold_np(q["op"], W[q["a"]], q["groups"])
            if kind == "fold":
                return {"value": popc_rows(out), "out": out}
            return {"value": popc_rows(out & WF[q["rf"]] if WF is not None else out)}
        if kind == "topn":
            ns, na = q["ra"].shape
            card = popc_rows(W[q["a"]])
            cnt = card[q["ra"]]
            if WF is not None:
                count = np.stack([popc_rows(W[q["a"]][q["ra"][s]] & WF[q["rf"][s]]) for s in range(ns)])
                src_n = popc_rows(WF)[q["rf"]]
            else:
                count, src_n = cnt, np.zeros(ns, dtype=np.uint64)
            return {"topn": topn_model(cnt, count, src_n, WF is not None, q["top"], q["mt"], q["tt"], semantics)}
        A, idx = self.rowset(q["a"]), np.arange(q["n"])
        F = self.rowset(q["f"]) if q["f"] is not None else None
        if kind == "bsi_sum":
            s, c = PB.bsi_sum(A, q["base"], q["depth"], F, q.get("rf"))
            return {"sums": s, "counts": c}
        R, cnt = PB.bsi_range(A, q["base"], q["depth"], q["op"], q["pred"])
        if kind == "bsi_range":
            return {"value": cnt, "out": R.words()}
        if F is not None:
            R, _ = PB.setop(PB.OP_AND, R, idx, F, q["rf"])
        s, c = PB.bsi_sum(A, q["base"], q["depth"], R, idx)
        return {"sums": s, "counts": c}

    # -- steps
    def apply(self, st: dict) -> dict:
        return getattr(self, "_" + st["do"])(st)

    def _prepare(self, st):
        qi = st["q"]
        q = self.c.queries[qi]
        if q["refusal"] is not None:
            return {"refused": q["refusal"]}
        self.qs[qi] = {"own": None, "cell": np.full(cell_words(q), CELL_FILL, dtype=np.uint64), "last": None, "res": None, "vers": None,
                       "semantics": self.opts["topn_semantics"], "runs": 0}
        if q["kind"] in ROW_KINDS:
            self.W[f"q{qi}"], self.ver[f"q{qi}"] = np.zeros((q["n"], 16, 1024), dtype=np.uint64), 0
        if q["kind"] == "topn":
            ns, na = q["ra"].shape
            if max(1, min(ns, (self.opts["matrix_pass_kb"] << 10) // (na * 8))) < ns:
                self.cov.add("topn_pass")
        return {"refused": None}

    def _run(self, st):
        qi, dest, acc = st["q"], st["dest"], st["acc"]
        q, s = self.c.queries[qi], self.qs[qi]
        why = run_refusal(q["kind"], dest, acc)
        if why:
            return {"refused": why}
        res = self.evaluate(qi, s["semantics"])
        kind = q["kind"]
        if kind in COUNT_KINDS or kind in ROW_KINDS:
            v = res["value"].reshape(-1).astype(np.uint64)
            s[dest] = (s[dest] + v) if acc else v.copy()
        else:
            s[dest] = res  # (BSI records and TopN results are whole answers)
        if kind in ROW_KINDS:
            name = f"q{qi}"
            if s["runs"]:
                was, now = self.W[name].reshape(q["n"], 16, -1).any(axis=2), res["out"].reshape(q["n"], 16, -1).any(axis=2)
                if (was & ~now).any():
                    self.cov.add("empty_slot_rerun")
            self.W[name], self.ver[name] = res["out"].copy(), self.ver[name] + 1
        s["last"], s["res"], s["vers"], s["runs"] = dest, res, self.versions(q), s["runs"] + 1
        self.cov.add("kind:" + kind)
        if max(self.c.depth_of(o) for o in self.c.operands(q)) >= 2:
            self.cov.add("chain2")
        if q["f"] == "O":
            self.cov.add("filter_mutable")
        if kind == "count_matrix" and q["keep"] and self.opts["matrix_pass_kb"] == 4:
            self.cov.add("kps_pass4")
        if acc and dest == "cell":
            self.cov.add("acc_cell")
        return {"refused": None, "cell": s["cell"] if dest == "cell" else None, "res": res}

    def _read(self, st):
        qi = st["q"]
        q, s = self.c.queries[qi], self.qs[qi]
        stale = s["vers"] != self.versions(q)
        if stale:
            self.cov.add("stale_read")
        return {"last": s[s["last"]], "res": s["res"], "stale": stale}

    def _mutate(self, st):
        if st["flags"] and self.opts["setop_direct_encode"] != 2:
            return {"refused": "FBK_SETOP_OPTIMIZE on a plan needs setop_direct_encode = 2"}
        self.W["O"] = NP_OPS[st["op"]](self.W["S0"][self.c.ia], self.W["S1"][self.c.ib])
        self.ver["O"] += 1
        return {"refused": None, "words": self.W["O"]}

    def _compact(self, st):
        self.ver["C"] += 1
        if any("C" in self.c.operands(self.c.queries[i]) and s["runs"] for i, s in self.qs.items()):
            self.cov.add("compact_live")
        return {}

    def _set_option(self, st):
        self.opts.update(st["opts"])
        return {}

    def _oneshot(self, st):
        return {"res": self.evaluate(st["q"], self.opts["topn_semantics"])}

    def _free(self, st):
        del self.qs[st["q"]]
        return {}


# ---- plans -----------------------------------------------------------------------------------------------------------------------
class PlanCase:
    """fbk_plan_*: a plan over random pairs with repeats and a random sequence of its launch-only forms.  steps: (name, *args)."""

    def __init__(self, it: int):
        self.it = it
        self.rng = rng = D.rng_for(7500, it)
        self.dense = it % 4 == 3
        self.rows, self.W = {}, {}
        for name in ("X", "Y"):
            self.rows[name], self.W[name] = _static_batch(rng, int(rng.integers(4, 41)), self.dense, range(0, 8) if name == "X" else range(8, 16))
        self.same = bool(rng.random() < 0.3)  # both operands from one batch
        if self.same:
            self.rows["Y"], self.W["Y"] = self.rows["X"], self.W["X"]
        n = int(rng.integers(1, 61))
        self.ia, self.ib = rng.integers(0, len(self.W["X"]), n), rng.integers(0, len(self.W["Y"]), n)
        self.ia[0] = self.ib[0] = 0
        self.n = n
        steps = [("setop", int(rng.integers(0, 4)), OPTIMIZE if rng.random() < 0.5 else 0)] if rng.random() < 0.5 else [("intersection_count",)]
        has_out, detached = steps[0][0] == "setop", False
        names = ["setop", "setop", "setop", "total", "total_cell", "intersection_count", "intersection_count_total", "intersection_count_accumulate", "read", "read", "detach"]
        for _ in range(int(rng.integers(10, 17))):
            name = names[int(rng.integers(0, len(names)))]
            if name == "setop":
                steps.append(("setop", int(rng.integers(0, 4)), OPTIMIZE if rng.random() < 0.5 else 0))
                has_out = True
            elif name == "detach":
                if has_out:
                    steps.append(("detach", bool(rng.random() < 0.5)))  # (and compact what was detached)
                    has_out, detached = False, True
            else:
                steps.append((name,))
        if not detached:  # every case detaches once, with a set-op on each side
            steps += [("setop", OP_OR, 0), ("detach", True)]
        steps += [("setop", OP_AND, OPTIMIZE), ("read",), ("setop", OP_XOR, 0), ("total",), ("read",)]
        self.steps = steps

    def __repr__(self):
        return f"PlanCase(seed {D.SEED:#x}, it {self.it}, {self.n} pairs, {len(self.steps)} steps)"


class PlanModel:
    """counts [n] (what the plan's count vector holds), total (its total cell, None until written), cell (the caller's uint64, starting
    at CELL_FILL), out (the words of the set-op output, None after a detach), detached (the words of every detached batch)"""

    def __init__(self, case: PlanCase):
        self.c = case
        self.A, self.B = case.W["X"][case.ia], case.W["Y"][case.ib]
        self.icounts = popc_rows(self.A & self.B)
        self.counts = self.total = self.out = None
        self.cell = CELL_FILL
        self.detached: list = []

    def apply(self, st) -> None:
        name = st[0]
        if name == "setop":
            self.out = NP_OPS[st[1]](self.A, self.B)
            self.counts = popc_rows(self.out)
        elif name == "total":
            self.total = int(self.counts.sum())
        elif name == "total_cell":
            self.cell = int(self.counts.sum())
        elif name == "intersection_count":
            self.counts = self.icounts
        elif name == "intersection_count_total":
            self.counts, self.total = self.icounts, int(self.icounts.sum())
        elif name == "intersection_count_accumulate":
            self.counts, self.cell = self.icounts, self.cell + int(self.icounts.sum())
        elif name == "detach":
            self.detached.append(self.out)
            self.out = None
