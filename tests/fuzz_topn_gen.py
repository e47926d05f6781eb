"""Case generator and expectations of the structural fuzz of TopN / TopK / TopK-BSI on fields of thousands of rows: the sizes at which
k_topn_candidates' two-level selection, the host / device ordering switch, the chunked k_rows_vs_filter launch and k_counts_to_bsi's slot
term do something.  tests/test_gpu_fuzz_topn.py executes the cases on the GPU, tests/test_fuzz_topn_cpu.py checks the generator
without one.  No GPU in here.

A case (Case(it), from datagen.rng_for(7600, it)) is a POOL of about 200 distinct device rows, indexed many times: rows_a is an index
list with repeats, so a 5003-row field costs one small upload and one small reference — cnt = pool_card[ra], count = pool_count[s][ra]
with pool_count[s][p] = popcount(pool_words[p] & F_s).

Pool: a random set G of B columns (a fifth to a quarter of the shard) and rows drawn as `k_in` columns of G plus `k_out` columns
outside it, so a row's cardinality and its count with a filter close to G are chosen separately:
  groups    8 cardinalities around B (0.62 B .. 1.5 B), 8 rows each with 98 % .. 15 % of their columns inside G: ties in cnt that carry
            different counts; group CUT (cardinality ~ B) is the one the fields place the cut of the candidate pass in
  one apart cardinalities CUT - 1, CUT + 1, CUT + 2 (one 2048-bin of the kernel's cardinality key), two rows each
  scattered 80 cardinalities log-uniform in 100 .. 890 000 (more than 2048 apart: level 0 of the key), any share inside G
  encodings 40 rows of datagen.random_row (every container encoding, missing slots), 6 empty rows, the full row of 2^20 columns
One filter row per shard: G with 4 % .. 30 % of its columns dropped and a few outside columns added, so |F_s| ~ B and the Tanimoto band
src T / 100 < cnt < src 100 / T holds the groups — more than a third of the pool — for every T used here (1, 20, 60).  rows_f is a
permutation of the filter batch's rows.

A case holds two FIELDS over its pool, a small and a large one (SIZES[it % 4]: 255 | 2049, 256 | 4096, 257 | 4097, 2047 | 5003: the
block stride of the candidate kernel, the first bin of its index key, the host / device ordering switch, a size that is no multiple
of 64), 2 + it % 3 shards, and on odd iterations option matrix_pass_kb = 4 (one or two shards a pass: the candidate flags accumulate
over the passes).  A field's rows_a repeats whole columns (field rows that are the same pool row in every shard: equal totals), puts
72 rows of group CUT into every field (36 on either side of row 2048; 71 and the one row past it in the 2049-row field) and a heavy row last.  Its parameter sets (n, min_threshold, tanimoto_threshold, with
the filter or not) are computed from the field, not hoped for: n = 1, 2, n_a - 1, the number of qualifying rows of the poorest shard
and one more, an n whose cut falls inside group CUT at an index >= 2048 and one at an index < 2048, Tanimoto 60 / 20 / 1, and a
(min_threshold, Tanimoto) pair whose min_threshold is one above the smallest count of the first n rows of shard 0.

Expectations: (indexes, counts) of every set under both topn_semantics from fuzz_prepared_gen.topn_model (tied to oracle/pytopn.py by
tests/test_fuzz_prepared_cpu.py); per shard the qualifying totals and the candidate flags from fuzz_prepared_gen.fragment_top_counts,
which members_expect adds up for any dealing of the shards.  walk_tags(case) names, from fragment_top_counts alone (Field.top and
what from_shards puts together from it), the regimes a case reaches.  The module itself needs no GPU and no ctypes; the two upload
helpers (Pool.upload_rows, filter_upload_rows) are the exception: they build featurebase_amd.roaring.Container rows for the GPU test.

BsiCase(n_a) (n_a in BSI_SIZES: 65 536, 65 537, 131 077, 2^20): the same kind of pool, 2 or 3 shards, the totals
pool_count[s][ra[s]].sum(0), their bit planes as words, and a split of the shards into two sets whose largest totals need different
bit depths (shard 0's filter is a sixteenth of the others')."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np

import datagen as D
from fuzz_prepared_gen import fragment_top_counts, topn_model

ITERS = int(os.environ.get("FBK_FUZZ_ITERS", "6"))
U = 1 << 20
SIZES = [(255, 2049), (256, 4096), (257, 4097), (2047, 5003)]
BSI_SIZES = (65536, 65537, 131077, 1 << 20)
SHARES = (0.98, 0.93, 0.86, 0.75, 0.6, 0.45, 0.3, 0.15)  # the part of a group row's columns that lies inside G
GROUP_CARDS = (0.62, 0.74, 0.87, 1.0, 1.12, 1.25, 1.38, 1.5)  # x B; index 3 is group CUT
CUT_GROUP = 3
CUT_ROWS = 72  # the rows of group CUT a field holds at least
DEFAULT_MIN_THRESHOLD = 1  # executor.go:40-42 (what topn_model puts for 0 under topn_semantics = 1)

def popc_rows(w: np.ndarray) -> np.ndarray:
    return np.bitwise_count(w).reshape(w.shape[0], -1).sum(axis=1).astype(np.uint64)


class Pool:
    """words [P, 16, 1024]; rows[p] = {slot: oracle container} for the rows of datagen.random_row, else None (uploaded by words_row: bitmaps,
    and what optimize() picks below 4096 columns a slot); card [P]; group[g] = the pool rows of cardinality group g"""

    def __init__(self, rng, n_scattered: int = 80, n_random: int = 40, per_group: int = 8, universe: int = U):
        """universe < 2^20 (and n_random = 0): the same pool on the first `universe` columns, for references that work on column sets"""
        self.universe = universe
        perm = rng.permutation(universe)
        self.B = B = int(rng.integers(universe // 5, universe // 4))
        self.pg, self.pc = perm[:B], perm[B:]
        words, rows = [], []

        def add(k_in: int, k_out: int) -> int:
            words.append(self.columns_words(rng, k_in, k_out))
            rows.append(None)
            return len(words) - 1

        def add_card(card: int, share: float) -> int:
            k_in = min(B, int(round(card * share)))
            k_in = max(k_in, card - (universe - B))
            return add(k_in, card - k_in)

        self.group_card = [int(B * f) + int(rng.integers(0, 50)) for f in GROUP_CARDS]
        self.group = [[add_card(c, SHARES[j % len(SHARES)]) for j in range(per_group)] for c in self.group_card]
        cut = self.group_card[CUT_GROUP]
        self.one_apart = [add_card(cut + d, sh) for d in (-1, 1, 2) for sh in (0.9, 0.5)]
        for _ in range(n_scattered):
            add_card(int(np.exp(rng.uniform(np.log(100), np.log(0.85 * universe)))), float(rng.uniform(0.05, 1.0)))
        for _ in range(n_random):
            row = D.random_row(rng, 0, float(rng.choice([0.0, 0.15, 0.6])))
            w = np.zeros((16, 1024), dtype=np.uint64)
            for k, c in row.items():
                w[k & 15] = c.words()
            words.append(w)
            rows.append(row)
        self.empty = []
        for _ in range(6):
            self.empty.append(add(0, 0))
        self.full = add(B, universe - B)
        order = rng.permutation(len(words))  # no structure in the pool's own row order
        back = np.argsort(order)
        self.words = np.stack([words[i] for i in order])
        self.rows = [rows[i] for i in order]
        self.group = [[int(back[p]) for p in g] for g in self.group]
        self.one_apart = [int(back[p]) for p in self.one_apart]
        self.empty = [int(back[p]) for p in self.empty]
        self.full = int(back[self.full])
        self.card = popc_rows(self.words)
        assert int(self.card[self.full]) == universe and not self.card[self.empty].any()
        assert all(int(self.card[p]) == c for g, c in zip(self.group, self.group_card) for p in g)

    def columns_words(self, rng, k_in: int, k_out: int) -> np.ndarray:
        """[16, 1024] words of k_in columns of G and k_out columns outside it: windows of the two fixed permutations"""
        bits = np.zeros(U, dtype=np.uint8)
        for src, k in ((self.pg, k_in), (self.pc, k_out)):
            if k:
                o = int(rng.integers(0, src.size))
                bits[np.take(src, np.arange(o, o + k), mode="wrap")] = 1
        return np.packbits(bits, bitorder="little").view(np.uint64).reshape(16, 1024).copy()

    def filter_words(self, rng, keep: float = 1.0) -> np.ndarray:
        """G * keep with 4 % .. 30 % of it dropped and up to 3 % of B added from outside"""
        B = self.B
        k_in = int(B * keep * (1.0 - float(rng.uniform(0.04, 0.3))))
        return self.columns_words(rng, k_in, int(B * keep * float(rng.uniform(0.0, 0.03))))

    def upload_rows(self) -> list:
        """the pool as {slot: featurebase_amd.roaring.Container} rows for Context.upload"""
        return [D.to_fbk_row(row) if row is not None else words_row(self.words[p]) for p, row in enumerate(self.rows)]


def words_row(w: np.ndarray) -> dict:
    """[16, 1024] words -> {slot: Container}: a bitmap from 4096 columns on, below that what optimize() picks (numpy only)"""
    from featurebase_amd.roaring import Container

    row = {}
    n = np.bitwise_count(w).sum(axis=1)
    for s in np.nonzero(n)[0]:
        if n[s] >= 4096:
            row[int(s)] = Container.bitmap(w[s], int(n[s]))
        else:
            row[int(s)] = D.fbk_container_of_vals(np.nonzero(np.unpackbits(w[s].view(np.uint8), bitorder="little"))[0].astype(np.int64))
    return row


def filter_upload_rows(words: np.ndarray) -> list:
    return [words_row(w) for w in words]


class Field:
    """ra [n_shards, n_a] over the pool; cnt, count_f [n_shards, n_a] (cardinality, count with the shard's filter); sets = the parameter
    sets (n, min_threshold, tanimoto_threshold, with the filter); expect[(set, semantics)] = (indexes, counts)"""

    def __init__(self, case: "Case", n_a: int):
        rng, pool, ns = case.rng, case.pool, case.n_shards
        self.n_a, self.case = n_a, case
        m = max(40, n_a // 3)
        pattern = rng.integers(0, len(pool.card), (ns, m))
        ra = pattern[:, rng.integers(0, m, n_a)]  # whole columns repeat: field rows with the same pool row in every shard
        hi = 2048 + rng.choice(n_a - 2048, min(36, n_a - 2048), replace=False) if n_a > 2048 else np.zeros(0, dtype=np.int64)
        lo = rng.choice(min(n_a, 2048), CUT_ROWS - hi.size, replace=False)  # (2049 rows: one row past 2048, 71 before it)
        self.cut_rows = np.sort(np.concatenate([lo, hi])).astype(np.int64)
        ra[:, self.cut_rows] = rng.choice(pool.group[CUT_GROUP], (ns, self.cut_rows.size))
        if n_a - 1 not in self.cut_rows:
            ra[:, n_a - 1] = pool.group[-1][0]  # the last row: the heaviest group's row closest to G (or a row of group CUT)
        ra[:, int(rng.integers(0, n_a - 1))] = pool.full
        self.ra = np.ascontiguousarray(ra, dtype=np.uint32)
        self.cnt = pool.card[self.ra]
        self.count_f = np.stack([case.pool_count[s][self.ra[s]] for s in range(ns)])
        self._ftc: Dict[tuple, list] = {}
        self.sets: List[Tuple[int, int, int, bool]] = []
        self.why: List[str] = []
        self._build_sets()
        self.expect: Dict[Tuple[int, int], Tuple[list, list]] = {}
        self.shard_tot: List[np.ndarray] = []
        self.shard_cand: List[Optional[np.ndarray]] = []
        zeros = np.zeros(ns, dtype=np.uint64)
        for si, (n, mt, tt, hf) in enumerate(self.sets):
            count, src = (self.count_f, case.src_n) if hf else (self.cnt, zeros)
            for sem in (0, 1):
                self.expect[(si, sem)] = topn_model(self.cnt, count, src, hf, n, mt, tt, sem)
            tot = np.zeros((ns, n_a), dtype=np.uint64)
            for s in range(ns):
                for r, c in self.top(s, 0, mt, tt, hf):
                    tot[s, r] = c
            self.shard_tot.append(tot)
            cand = None
            if 0 < n < n_a:
                cand = np.zeros((ns, n_a), dtype=bool)
                for s in range(ns):
                    cand[s, [r for r, _ in self.top(s, n, mt, tt, hf)]] = True
            self.shard_cand.append(cand)

    def top(self, s: int, n: int, mt: int, tt: int, hf: bool) -> list:
        """fragment.top of shard s: [(row, count)] (n = 0: every qualifying row)"""
        key = (s, n, mt, tt, hf)
        if key not in self._ftc:
            count, src = (self.count_f[s], int(self.case.src_n[s])) if hf else (self.cnt[s], 0)
            self._ftc[key] = fragment_top_counts(self.cnt[s], count, src, hf, n, mt or DEFAULT_MIN_THRESHOLD, tt)
        return self._ftc[key]

    def rank_order(self, s: int, mt: int, tt: int, hf: bool) -> List[int]:
        """the qualifying rows of shard s in the order fragment.top meets them: cardinality descending, row ascending"""
        return sorted((r for r, _ in self.top(s, 0, mt, tt, hf)), key=lambda r: (-int(self.cnt[s, r]), r))

    def _cut_in_group(self, s: int, mt: int, tt: int, hf: bool, high: bool) -> int:
        """an n whose n-th qualifying row of shard s is a row of group CUT with an index >= 2048 (high) or < 2048, other rows of the
        group on both sides of it"""
        order = self.rank_order(s, mt, tt, hf)
        card = self.case.pool.group_card[CUT_GROUP]
        tied = [j for j, r in enumerate(order) if int(self.cnt[s, r]) == card]
        pick = [j for j in tied[1:-1] if (order[j] >= 2048) == high] or [j for j in tied if (order[j] >= 2048) == high] or tied
        return pick[len(pick) // 2] + 1

    def _build_sets(self) -> None:
        case, pool, n_a, ns = self.case, self.case.pool, self.n_a, self.case.n_shards
        it, large = case.it, self.n_a > 2048
        uc = np.unique(pool.card)
        j = int(np.searchsorted(uc, int(pool.B * 0.55)))
        while uc[j + 1] - uc[j] < 2:
            j += 1
        mt_mid = int(uc[j]) + 1  # between two pool cardinalities
        q = [len(self.top(s, 0, mt_mid, 0, True)) for s in range(ns)]

        def add(why, n, mt, tt, hf):
            self.sets.append((int(n), int(mt), int(tt), bool(hf)))
            self.why.append(why)

        add("n = 1", 1, 0, 0, False)
        add("n = 2", 2, 1, 0, True)
        add("n = n_a - 1: no heap fills, fewer results than n", n_a - 1, mt_mid, 0, True)
        add("heap fills exactly in the poorest shard", min(q), mt_mid, 0, True)
        add("one more: that shard's heap never fills", min(q) + 1, mt_mid, 0, True)
        add("cut inside group CUT, id >= 2048" if large else "cut inside group CUT", self._cut_in_group(0, 0, 0, True, large), 0, 0, True)
        tt = (20, 1, 60)[it % 3]
        n = (8, 5, 3)[it % 3]
        t_heap = min(int(self.count_f[0, r]) for r in self.rank_order(0, 0, tt, True)[:n])
        add("min_threshold above the heap minimum under Tanimoto", n, t_heap + 1, tt, True)
        if large:
            add("cut inside group CUT, id < 2048, no filter", self._cut_in_group(ns - 1, 0, 0, False, False), 0, 0, False)
            add("Tanimoto 60", 2, 0, 60, True)
            add("Tanimoto 20, the poorest shard's heap fills exactly", min(len(self.top(s, 0, 0, 20, True)) for s in range(ns)), 0, 20, True)
            add("Tanimoto 1", 5, 0, 1, True)
            add("Tanimoto 20, cut inside group CUT", self._cut_in_group(ns - 1, 0, 20, True, it % 2 == 0), 0, 20, True)

    def from_shards(self, si: int, sem: int) -> Tuple[list, list]:
        """(indexes, counts) of set si put together from fragment.top's per-shard answers alone: the totals of the rows some shard
        returns for N = n (semantics 1), of every qualifying row (semantics 0)"""
        tot, flags = self.members_expect(si, sem, range(self.case.n_shards))
        tot = np.where(flags, tot, np.uint64(0))
        order = np.lexsort((np.arange(self.n_a), -tot.astype(np.int64)))
        order = order[tot[order] > 0][: self.sets[si][0] or None]
        return order.tolist(), [int(c) for c in tot[order]]

    def members_expect(self, si: int, sem: int, shards) -> Tuple[np.ndarray, np.ndarray]:
        """(totals, candidate flags) fbk_topn_partials reports for a member that owns `shards`"""
        tot = np.zeros(self.n_a, dtype=np.uint64)
        flags = np.zeros(self.n_a, dtype=bool)
        cand = self.shard_cand[si] if sem == 1 else None
        for s in shards:
            tot += self.shard_tot[si][s]
            if cand is not None:
                flags |= cand[s]
        return tot, (flags if cand is not None else tot != 0)


class Case:
    def __init__(self, it: int, sizes=None, **pool_args):
        """sizes / pool_args: a down-sized case (tests/test_fuzz_topn_cpu.py ties one to oracle/pytopn.py on column sets)"""
        self.it = it
        self.rng = rng = D.rng_for(7600, it)
        self.n_shards = ns = 2 + it % 3
        self.options = {"matrix_pass_kb": 4} if it % 2 else {}
        self.pool = pool = Pool(rng, **pool_args)
        f_words = np.stack([pool.filter_words(rng) for _ in range(ns)])
        self.rf = rng.permutation(ns).astype(np.uint32)
        self.filter_words = np.empty_like(f_words)  # the filter batch: shard s reads its row rf[s]
        self.filter_words[self.rf] = f_words
        self.src_n = popc_rows(f_words)
        self.pool_count = [popc_rows(pool.words & f_words[s]) for s in range(ns)]
        self.fields = [Field(self, n_a) for n_a in (sizes or SIZES[it % 4])]
        # two uneven dealings of the shards to two members (one member gets a single shard), and the groups' dealings
        self.dealings = [[[0], list(range(1, ns))], [list(range(ns - 1)), [ns - 1]]]
        self.group_dealings = [[list(range(1, ns)), [0]], [[ns - 1], [], list(range(ns - 1))]]

    def __repr__(self):
        return f"Case(seed {D.SEED:#x}, it {self.it}, {self.n_shards} shards, fields {[f.n_a for f in self.fields]}, options {self.options})"

    def pass_shards(self, n_a: int) -> int:
        """the shards one pass of topn_totals_locked holds under the case's options"""
        return max(1, min(self.n_shards, (self.options.get("matrix_pass_kb", 1 << 20) << 10) // (n_a * 8)))


def walk_tags(case: Case) -> Dict[str, list]:
    """tag -> [(field's n_a, set index)]: the regimes of the candidate pass and of the ordering that the case reaches, read off
    fragment_top_counts' own answers (Field.top, Field.from_shards)"""
    tags: Dict[str, list] = {}
    tani_ok, tani_seen = True, False

    def tag(name, f, si):
        tags.setdefault(name, []).append((f.n_a, si))

    for f in case.fields:
        ns, n_a = case.n_shards, f.n_a
        for si, (n, mt, tt, hf) in enumerate(f.sets):
            if n_a > 256:
                tag("stride2", f, si)
            if n_a > 4096:
                tag("device_sort_default", f, si)
            if case.pass_shards(n_a) < ns:
                tag("multi_pass", f, si)
            if f.from_shards(si, 0) != f.from_shards(si, 1):
                tag("ref_ne_exact", f, si)
            if not 0 < n < n_a:
                continue
            orders = [f.rank_order(s, mt, tt, hf) for s in range(ns)]
            short = [len(o) < n for o in orders]
            if tt:
                tani_seen = True
                tani_ok = tani_ok and not all(short)
            if any(short):
                tag("heap_short", f, si)
                if not all(short):
                    tag("heap_short_one_shard_only", f, si)
            cands = [set(r for r, _ in f.top(s, n, mt, tt, hf)) for s in range(ns)]
            for s, o in enumerate(orders):
                if len(o) == n:
                    tag("heap_exact", f, si)
                if len(o) < n:
                    continue
                id_cut, v = o[n - 1], int(f.cnt[s, o[n - 1]])
                if sum(int(f.cnt[s, r]) == v for r in o) >= 2:
                    if id_cut >= 2048:
                        tag("id_bin_hi", f, si)
                    elif n_a > 2048:
                        tag("id_bin_lo", f, si)
                if len(cands[s]) > n:
                    tag("later_rows", f, si)
                count = f.count_f[s] if hf else f.cnt[s]
                t_heap = min(int(count[r]) for r in o[:n])
                if tt and t_heap < mt and len(f.top(s, n, 0, tt, hf)) > n:  # (rows that a MinThreshold of 0 would have let in later)
                    tag("later_off_tanimoto", f, si)
            once = [r for r in f.from_shards(si, 1)[0] if sum(r in c for c in cands) == 1]
            if once:
                tag("cand_from_one_shard", f, si)
    if tani_seen and tani_ok:
        tags["tanimoto_nondegenerate"] = [(-1, -1)]
    return tags


def planes_of(tot: np.ndarray) -> np.ndarray:
    """[depth, 16, 1024] words: plane p holds row id i iff bit p of tot[i] is set (bsiBuilder.Insert, bsi.go:251-284)"""
    depth = int(tot.max()).bit_length()
    out = np.zeros((depth, 16, 1024), dtype=np.uint64)
    bits = np.zeros(U, dtype=np.uint8)
    for p in range(depth):
        bits[: tot.size] = (tot >> np.uint64(p)) & np.uint64(1)
        out[p] = np.packbits(bits, bitorder="little").view(np.uint64).reshape(16, 1024)
    return out


def decode_planes(planes: np.ndarray) -> np.ndarray:
    """[2^20] values from [depth, 16, 1024] words"""
    got = np.zeros(U, dtype=np.uint64)
    for p in range(planes.shape[0]):
        got |= np.unpackbits(planes[p].reshape(-1).view(np.uint8), bitorder="little").astype(np.uint64) << np.uint64(p)
    return got


def top_of(tot: np.ndarray, k: int) -> Tuple[list, list]:
    """(indexes, counts) of the k largest totals: count descending, index ascending, zeros dropped"""
    order = np.lexsort((np.arange(tot.size), -tot.astype(np.int64)))
    order = order[tot[order] > 0][:k]
    return order.tolist(), [int(c) for c in tot[order]]


class BsiCase:
    def __init__(self, n_a: int):
        self.n_a = n_a
        self.rng = rng = D.rng_for(7700, n_a)
        self.n_shards = ns = 2 + (BSI_SIZES.index(n_a) % 2 if n_a in BSI_SIZES else 0)
        self.pool = pool = Pool(rng, n_scattered=30, n_random=16, per_group=3)
        f_words = np.stack([pool.filter_words(rng, keep=1.0 / 16 if s == 0 else 1.0) for s in range(ns)])
        self.rf = rng.permutation(ns).astype(np.uint32)
        self.filter_words = np.empty_like(f_words)
        self.filter_words[self.rf] = f_words
        self.src_n = popc_rows(f_words)
        self.pool_count = [popc_rows(pool.words & f_words[s]) for s in range(ns)]
        m = max(40, n_a // 3)
        pattern = rng.integers(0, len(pool.card), (ns, m))
        ra = pattern[:, rng.integers(0, m, n_a)]
        ra[:, n_a - 1] = pool.group[-1][0]  # a bit in the last (partial) word of every plane
        ra[:, int(rng.integers(0, n_a - 1))] = pool.full
        self.ra = np.ascontiguousarray(ra, dtype=np.uint32)
        self.shard_tot = np.stack([self.pool_count[s][self.ra[s]] for s in range(ns)])
        self.tot = self.shard_tot.sum(axis=0)
        self.split = ([0], list(range(1, ns)))  # shard 0 reads the small filter: its totals need fewer planes
        self.planes = planes_of(self.tot)
        order = np.lexsort((np.arange(n_a), -self.tot.astype(np.int64)))
        self.order = order[self.tot[order] > 0]

    def topn_expect(self, n: int, semantics: int):
        """(indexes, counts) of fbk_topn(n) with the filter, no thresholds"""
        return topn_model(self.pool.card[self.ra], self.shard_tot, self.src_n, True, n, 0, 0, semantics)

    def __repr__(self):
        return f"BsiCase(seed {D.SEED:#x}, {self.n_a} rows, {self.n_shards} shards)"
