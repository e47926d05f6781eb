"""CPU checks of fbk_bsi_moments (no GPU): the ABI's shape, the host rules of featurebase_amd/csrc/fbk_moments_plan.h compiled
into a stand-alone program (tests/cpp/moments_plan_check.cpp, -fsanitize=address,undefined, as the other test_*_plan_cpu.py build
theirs), the reference model of tests/moments_ref.py against the Python-int definition, a numpy model of the kernel's arithmetic
(chunk bytes, Gram matrix, fold) against it, and moments_var / moments_corr against the decimals of the reference's SQL tests
(tests/golden/sql_var_corr.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import datagen as D
import moments_ref as M
from featurebase_amd import lib as L
from featurebase_amd import roaring as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker():
    out = os.path.join(ROOT, "build", "moments_plan_check_san")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "moments_plan_check.cpp"), "-o", out])

    def run(lines):
        r = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"moments_plan_check exit {r.returncode}\n{r.stderr[-4000:]}"
        got = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got

    return run


def test_symbol_signature_and_struct():
    lib = L.load()
    assert hasattr(lib, "fbk_bsi_moments")
    assert len(L.SIGNATURES["fbk_bsi_moments"][1]) == 11
    assert C.sizeof(L.Moments) == 96 and C.sizeof(L.I128) == 16
    assert int(L.I128(lo=(1 << 64) - 1, hi=-1)) == -1 and int(L.I128(lo=5, hi=2)) == (2 << 64) + 5


def test_null_arguments_are_invalid():
    lib = L.load()
    out = L.Moments()
    rows = np.zeros(1, dtype=np.uint32)
    fake = C.c_void_p(16)  # never dereferenced: a NULL argument is found first
    calls = [
        (None, fake, rows.ctypes.data, 1, None, None, 0, None, None, 0, C.byref(out)),  # ctx
        (None, None, rows.ctypes.data, 1, None, None, 0, None, None, 0, C.byref(out)),
        (None, fake, None, 1, None, None, 0, None, None, 0, C.byref(out)),
        (None, fake, rows.ctypes.data, 1, None, None, 0, None, None, 0, None),
    ]
    for args in calls:
        assert lib.fbk_bsi_moments(*args) == L.FBK_E_INVALID


def from_checker(vals):
    n, rest = vals[0], vals[1:]
    return M.Moments(n, *(rest[2 * k + 1] * (1 << 64) + rest[2 * k] for k in range(5)))


def test_chunk_row_map_and_flush_bound(checker):
    depths = [0, 1, 6, 7, 8, 14, 15, 20, 63, 64]
    grid = [(dx, dy) for dx in depths for dy in depths]
    got = checker([f"R {dx} {dy}" for dx, dy in grid])
    for (dx, dy), g in zip(grid, got):
        cx, cy = -(-dx // 7), -(-dy // 7)
        assert g[:4] == [cx, cy, cx + cy, cx + cy + 1] == list(M.rows_of(dx, dy)), (dx, dy)
        # spare rows: 4 (2) column blocks share the 32-row tile when the call has at most 8 (16) rows
        assert g[3] <= 32 // g[4] and g[4] == (4 if g[3] <= 8 else 2 if g[3] <= 16 else 1), (dx, dy)
    assert checker(["R 64 64", "R 20 20", "R 32 32", "R 20 0", "R 49 0", "R 50 0"]) == [[10, 10, 20, 21, 1], [3, 3, 6, 7, 4], [5, 5, 10, 11, 2],
                                                                                         [3, 0, 3, 4, 4], [7, 0, 7, 8, 4], [8, 0, 8, 9, 2]]
    (cols, shards), = checker(["K"])
    # an i32 cell is exact for `cols` columns of products of magnitude 127^2 and for no more; 2^17 is the safe power of two
    assert cols * 127 * 127 < 1 << 31 <= (cols + 1) * 127 * 127
    assert 1 << 17 <= cols < 1 << 18
    assert shards * (1 << 20) * 127 * 127 < 1 << 63  # the cross-shard sums stay in i64


def test_densify_chunk(checker):
    cases = [(xe, dx, hy, ye, dy, hf, fe) for xe in (0, 1) for dx in (0, 20, 64) for hy in (0, 1) for ye in (0, 1) for dy in (0, 13, 64)
             for hf in (0, 1) for fe in (0, 1) if hy or dy == 0]
    rows = checker(["D " + " ".join(map(str, c)) for c in cases])
    for (xe, dx, hy, ye, dy, hf, fe), (r,) in zip(cases, rows):
        assert r == (dx + 2 if xe else 0) + (dy + 2 if hy and ye else 0) + (1 if hf and fe else 0)
    grid = [(ns, r) for ns in (0, 1, 2, 61, 62, 64, 100, 1000, 1 << 20) for r in (0, 1, 2, 22, 66, 67, 133)]
    got = checker([f"C {ns} {r}" for ns, r in grid])
    for (ns, r), (c,) in zip(grid, got):
        if r == 0 or ns == 0:
            assert c == ns
            continue
        most = max(1, min(ns, (1 << 30) // ((1 << 17) * r)))
        passes = -(-ns // most)
        assert c == -(-ns // passes), (ns, r)
        assert c <= most and c * passes >= ns
    # the call of tests/test_gpu_bsi_moments.py: 64 shards of encoded x, y and filter at depth 64 x 64: 61 fit, two chunks of 32
    assert checker(["C 64 133"]) == [[32]]
    assert M.densify_chunk(64, False, 64, False, 64, False) == 32
    assert M.densify_chunk(64, True, 64, True, 64, True) == 64 and M.densify_chunk(1000, False, 64, None, 0, None) == 112


def _fold_line(dx, dy, S):
    cells = [(i, j, int(S[i, j])) for i in range(32) for j in range(32) if S[i, j]]
    return f"F {dx} {dy} {len(cells)} " + " ".join(f"{i} {j} {v}" for i, j, v in cells)


def test_fold_of_random_and_extreme_matrices(checker):
    rng = D.rng_for(9100)
    lines, want = [], []
    for dx, dy in [(0, 0), (1, 0), (7, 8), (8, 7), (20, 13), (63, 64), (64, 64), (64, 0)]:
        _, _, _, n_rows = M.rows_of(dx, dy)
        mats = [rng.integers(-(1 << 62), 1 << 62, (32, 32), dtype=np.int64) for _ in range(3)]
        # every cell at +- 2^20 n 127^2 (n = 2^28 shards: the largest a call takes), uniform and with random signs
        big = (1 << 20) * (1 << 28) * 127 * 127
        mats += [np.full((32, 32), big, dtype=np.int64), np.full((32, 32), -big, dtype=np.int64),
                 np.where(rng.random((32, 32)) < 0.5, -big, big).astype(np.int64),
                 np.full((32, 32), np.iinfo(np.int64).max, dtype=np.int64), np.full((32, 32), np.iinfo(np.int64).min, dtype=np.int64)]
        for S in mats:
            S = S.copy()
            S[n_rows:, :] = 0  # rows the call does not have are zero (and never read)
            S[:, n_rows:] = 0
            lines.append(_fold_line(dx, dy, S))
            want.append(M.fold(S, dx, dy))
    got = checker(lines)
    for line, g, w in zip(lines, got, want):
        assert g[0] == w.n % (1 << 64), line[:40]
        assert from_checker(g)[1:] == w[1:], line[:40]
    # depth 64 x 64 with every cell at the extreme: the exact sum does not fit 128 bits, the fold wraps
    S = np.full((32, 32), (1 << 20) * (1 << 28) * 127 * 127, dtype=np.int64)
    S[21:, :] = 0
    S[:, 21:] = 0
    exact = sum(int(S[m, 10 + k]) << (7 * (m + k)) for m in range(10) for k in range(10))
    assert exact >= 1 << 127 and M.fold(S, 64, 64).sum_xy == M.wrap128(exact) != exact
    assert from_checker(checker([_fold_line(64, 64, S)])[0]).sum_xy == M.wrap128(exact)


def _fragment(rng, depth, n_cols, density=0.7, junk=True):
    """[depth + 2, 16, 1024] words with values in the first n_cols columns only; sign and plane bits outside exists when junk"""
    S = np.zeros((depth + 2, 1 << 20), dtype=bool)
    S[0, :n_cols] = rng.random(n_cols) < density
    S[1:, :n_cols] = rng.random((depth + 1, n_cols)) < 0.5
    if not junk:
        S[1:] &= S[0]
    packed = np.packbits(S, axis=1, bitorder="little").view(np.uint64)
    return packed.reshape(depth + 2, 16, 1024)


@pytest.mark.parametrize("dx,dy", [(0, 0), (1, 1), (7, 8), (8, 7), (63, 64), (64, 64), (64, None), (7, None)])
def test_models_agree_with_the_definition(dx, dy):
    """expected() (16-bit limbs) and the kernel's arithmetic (7-bit signed chunks, Gram, fold) equal the Python-int loop; both signs"""
    rng = D.rng_for(9200, dx, 99 if dy is None else dy)
    n_sh, n_cols = 2, 3000
    Sx = np.stack([_fragment(rng, dx, n_cols) for _ in range(n_sh)])
    Sy = np.stack([_fragment(rng, dy, n_cols) for _ in range(n_sh)]) if dy is not None else None
    if dx >= 63:  # the extremes: the largest magnitude with both signs, and a set sign over magnitude 0
        Sx[0, :, 0, 0] &= ~np.uint64(0xF)  # columns 0..3: -(2^dx - 1), 2^dx - 1, "-0", 0
        Sx[0, 0, 0, 0] |= np.uint64(0xF)
        Sx[0, 1, 0, 0] |= np.uint64(0x5)
        Sx[0, 2:, 0, 0] |= np.uint64(0x3)
        assert M.values_at(Sx[0], dx, range(4)) == [-((1 << dx) - 1), (1 << dx) - 1, 0, 0]
        if Sy is not None:
            Sy[0, 0, 0, 0] |= np.uint64(0xF)
    F = _fragment(rng, 0, n_cols, 0.8)[0][None].repeat(n_sh, axis=0)
    for filt in (None, F):
        want = M.brute_shards(Sx, dx, Sy, dy or 0, filt)
        assert want.n > 500
        assert M.expected(Sx, dx, Sy, dy or 0, filt) == want
        G = np.zeros((32, 32), dtype=object)
        for s in range(n_sh):
            ex, mx, nx = M.decode(Sx[s], dx)
            sel = ex.copy()
            my = ny = None
            if Sy is not None:
                ey, my, ny = M.decode(Sy[s], dy)
                sel &= ey
            if filt is not None:
                sel &= M.R.bits(filt[s])
            G += M.gram(mx[sel], nx[sel], dx, my[sel] if Sy is not None else None, ny[sel] if Sy is not None else None, dy or 0).astype(object)
        got = M.fold(G, dx, dy or 0)
        if Sy is None:
            assert got[2] == got[4] == got[5] == 0
        assert got == want
    if dx >= 1:
        assert any(v is not None and v < 0 for v in M.values_at(Sx[0], dx, range(64))) and any(v is not None and v > 0 for v in M.values_at(Sx[0], dx, range(64)))


def test_sql_var_and_corr_goldens():
    with open(os.path.join(ROOT, "tests", "golden", "sql_var_corr.json")) as f:
        gold = json.load(f)
    assert len(gold["cases"]) == 5
    for case in gold["cases"]:
        t = gold["tables"][case["table"]]
        assert all(len(v) == 6 for v in t.values())
        xs, ys = t[case["x"]], t[case["y"]] if case["y"] else None
        m = RO.Moments(*M.brute(xs, ys))
        got = RO.moments_var(m) if case["agg"] == "var" else RO.moments_corr(m)
        assert got == case["expect"], case["sql"]
        # Base changes neither: the moments of the shifted values, from the raw ones
        shifted = RO.moments_shift(RO.Moments(*M.brute([x - 7 for x in xs], [y + 1000 for y in ys] if ys else None)), 7, -1000 if ys else 0)
        assert shifted == m
    # no value where the reference's is undefined
    assert RO.moments_var(RO.Moments(0, 0, 0, 0, 0, 0)) is None and RO.moments_corr(RO.Moments(0, 0, 0, 0, 0, 0)) is None
    assert RO.moments_corr(RO.Moments(*M.brute([3, 3, 3], [1, 2, 3]))) is None  # a constant column: zero under the root
    assert RO.moments_var(RO.Moments(*M.brute([-5, 5], None))) == 25_000_000
    assert RO.moments_corr(RO.Moments(*M.brute([1, 2, 3], [-2, -4, -6]))) == -1_000_000
