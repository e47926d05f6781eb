"""Worlds and the numpy model for fbk_expr_row_counts / fbk_expr_topk / fbk_expr_topn (shared by tests/test_expr_rows_cpu.py and
tests/test_gpu_expr_rows.py): expr_gen.World plus a set field "F" the counting operators group by.

The field is a POOL of 40 datagen.random_row rows, uploaded once and indexed many times (as fuzz_topn_gen.Pool does): a field of n_a
rows in a world of n_shards shards is an [n_shards, n_a] array of pool indexes, rows repeating freely.  Pool row 0 certainly holds an
array of more than 4096 values (the over-8-KiB path of the streaming phase), a full container, a nil slot and a run container; row 1
is empty.  The model: counts[s][i] = popcount(model(tree)[s] & words(F_i[s])), totals and per-shard filter counts from it.

rows_per_block is the Python restatement of fbk_expr::rows_per_block (fbk_expr_plan.h), operand_reads of fbk_expr::operand_reads
over the numpy-interpretable instruction list the stand-alone planner check prints."""
import os
import subprocess
from typing import List, Tuple

import numpy as np

import datagen as D
import expr_gen as G

ROOT = G.ROOT
POOL = 40
N_AS = (1, 63, 64, 65, 200)
FORCED = ["array_dense_runs", "run_full", None, "run_many", "bitmap_dense", "array_small"]  # slots 0.. of pool row 0


def popc(words: np.ndarray) -> np.ndarray:
    """[..., 16, 1024] uint64 -> popcount over the last two axes"""
    w = np.ascontiguousarray(words)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[:-2] + (-1,)), axis=-1).sum(axis=-1).astype(np.uint64)


class World(G.World):
    def __init__(self, it: int):
        super().__init__(it)
        rng = D.rng_for(9300, it)
        self.pool = []
        for r in range(POOL):
            row = {} if r == 1 else D.random_row(rng, r, p_missing=0.3)
            if r == 0:
                for slot, kind in enumerate(FORCED):
                    row.pop(slot, None)
                    if kind:
                        row[slot] = D.oracle_container(rng, kind)
            self.pool.append(row)
        self.pool_words = np.stack([G.words_of_row(r) for r in self.pool])  # [POOL, 16, 1024]
        self.field_rng = D.rng_for(9301, it)
        self._pool_counts = {}

    def field(self, n_a: int) -> np.ndarray:
        """[n_shards, n_a] pool indexes; row 0 of shard 0 is pool row 0, the last row of the last shard the empty pool row"""
        rows = self.field_rng.integers(0, POOL, size=(self.n_shards, n_a)).astype(np.uint32)
        rows[0, 0] = 0
        if n_a > 1:
            rows[-1, -1] = 1
        return rows

    def pool_counts(self, tree) -> np.ndarray:
        """[n_shards, POOL]: |pool row p ∩ model(tree)[s]|"""
        hit = self._pool_counts.get(id(tree))
        if hit is None or hit[0] is not tree:
            f = self.model(tree)
            hit = self._pool_counts[id(tree)] = (tree, np.stack([popc(self.pool_words & f[s][None]) for s in range(self.n_shards)]))
        return hit[1]

    def model_counts(self, tree, rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(totals [n_a], per shard [n_shards, n_a], filter counts [n_shards])"""
        pc = self.pool_counts(tree)
        per = np.stack([pc[s][rows[s]] for s in range(self.n_shards)]).astype(np.uint64)
        return per.sum(axis=0).astype(np.uint64), per, G.popcount(self.model(tree))


def top_of(totals: np.ndarray, k: int) -> Tuple[List[int], List[int]]:
    """fbk_topk's ordering: count descending, index ascending, zeros dropped, k = 0 for all"""
    order = [i for i in sorted(range(len(totals)), key=lambda i: (-int(totals[i]), i)) if totals[i]]
    if k:
        order = order[:k]
    return order, [int(totals[i]) for i in order]


# ---- rows per block ---------------------------------------------------------------------------------------------------------------
def rounded(r: int) -> int:
    return max(64, (r + 63) & ~63)


def rows_per_block(n_a: int, n_shards: int, L: int) -> int:
    """the rule of k_rows_vs_filter's launches (halve while the grid is short of 2048 blocks and more than 64 rows are left, then a
    multiple of 64, at least 64), a split taken only while (chunks - 1) * L <= n_a for the chunks it leads to"""
    rpb = n_a
    while rpb > 64 and n_shards * 16 * ((n_a + rpb - 1) // rpb) < 2048:
        half = (rpb + 1) // 2
        chunks = (n_a + rounded(half) - 1) // rounded(half)
        if (chunks - 1) * L > n_a:
            break
        rpb = half
    return rounded(rpb)


def chunks_of(n_a: int, n_shards: int, L: int) -> Tuple[int, int]:
    """(blocks per (shard, slot), rows of the last one)"""
    rpb = rows_per_block(n_a, n_shards, L)
    c = (n_a + rpb - 1) // rpb
    return c, n_a - (c - 1) * rpb


def operand_reads(ins: List[int]) -> int:
    return sum(1 for w in ins if (w >> 24) <= G.I_MOR_XAN)


# ---- the stand-alone check of fbk_expr::rows_per_block (tests/cpp/expr_rows_check.cpp) ---------------------------------------------
def build_rows_checker(out: str) -> str:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "expr_rows_check.cpp"), "-o", out])
    return out


def run_rows_checker(exe: str, grid: List[Tuple[int, int, int]]) -> List[int]:
    run = subprocess.run([exe], input="".join(f"{a} {s} {l}\n" for a, s, l in grid), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, f"expr_rows_check exit {run.returncode}\n{run.stderr[-4000:]}"
    out = [int(x) for x in run.stdout.split()]
    assert len(out) == len(grid)
    return out
