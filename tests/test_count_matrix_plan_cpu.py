"""CPU check of the host rules of the GroupBy count-matrix family (featurebase_amd/csrc/fbk_count_matrix_plan.h, no GPU): the header is
compiled into a stand-alone program (tests/cpp/count_matrix_plan_check.cpp, -fsanitize=address,undefined, run as a program the way
tests/test_group_select_plan_cpu.py runs its checker) and compared with a Python restatement of what the five launch sites, the path
chain and the pass rule were before they shared it: each site's loop is written out below with its own constants, as it stood."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS_VS_FILTER, DENSE, FUSED, GENERIC = 0, 1, 2, 3
SHARDS = (1, 2, 3, 64, 255, 256, 257, 1024, 8192)
SIDES = (1, 2, 4, 15, 16, 31, 32, 33, 64, 65, 4096)
SHAPES = [(a, b) for a in SIDES for b in SIDES] + [(1 << 22, 1)]
PINS = (0, 1, 2, 4, 8, 16)
N_CU = (1, 256, 304)
PASS_KB = (1, 4, 64, 1 << 20)


@pytest.fixture(scope="module")
def checker():
    out = os.path.join(ROOT, "build", "count_matrix_plan_check_san")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "count_matrix_plan_check.cpp"), "-o", out])

    def run(lines):
        r = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"count_matrix_plan_check exit {r.returncode}\n{r.stderr[-4000:]}"
        got = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got

    return run


def ask(checker, kind, grid):
    return checker([kind + " " + " ".join(str(x) for x in g) for g in grid])


# ---- the former code, site by site ----
def former_dense(n_a, n_b, n_shards, pin):
    tm, tn = (2 if n_a > 32 else 1), (2 if n_b > 32 else 1)
    tiles = ((n_a + 32 * tm - 1) // (32 * tm)) * ((n_b + 32 * tn - 1) // (32 * tn))
    spb = 16
    while spb > 2 and n_shards * (16 // spb) * tiles < 4096:
        spb >>= 1
    if pin:
        spb = pin
    return [tm, tn, tiles, spb, n_shards * (16 // spb) * tiles]


def former_fused(n_a, n_b, pn, n_cu, pin):
    tiles = ((n_a + 31) // 32) * ((n_b + 31) // 32)
    spb = 16
    while spb > 2 and pn * (16 // spb) * tiles < max(n_cu, 1):
        spb >>= 1
    if pin:
        spb = pin
    return [tiles, spb, pn * (16 // spb) * tiles]


def former_generic(n_a, pn, pin):  # (the option was never read here)
    ta = 4
    agroups = (n_a + 8 * ta - 1) // (8 * ta)
    spb = 16
    while spb > 1 and pn * (16 // spb) * agroups < 1024:
        spb >>= 1
    return [agroups, spb, pn * (16 // spb) * agroups]


def former_sum(n_a, n_b, ns, pin):  # (nor here)
    tiles = ((n_a + 31) // 32) * ((n_b + 31) // 32)
    spb = 16
    while spb > 1 and ns * (16 // spb) * tiles < 2048:
        spb >>= 1
    return [tiles, spb, ns * (16 // spb) * tiles]


def former_cube(n_p, n_a, n_b, ns, pin):
    pt = 4 if n_p <= 4 else 8
    tiles = ((n_p + pt - 1) // pt) * ((n_a + 31) // 32) * ((n_b + 31) // 32)
    spb = 16
    while spb > 1 and ns * (16 // spb) * tiles < 2048:
        spb >>= 1
    if pin:
        spb = pin
    return [pt, tiles, spb, ns * (16 // spb) * tiles]


def former_path(n_a, n_b, has_filter, all_dense, fused_mode):
    if n_b == 1 and not has_filter:
        return ROWS_VS_FILTER
    if all_dense and n_b > 1:
        return DENSE
    if n_b > 1 and fused_mode != 0 and (fused_mode == 1 or n_a * n_b >= 16):
        return FUSED
    return GENERIC


def former_pass_shards(n_shards, n_a, n_b, kb, keep):
    return n_shards if keep else max(1, min(n_shards, (kb << 10) // (n_a * n_b * 8)))


def test_slots_per_block_and_tiles_of_the_five_sites(checker):
    dense = [(a, b, ns, pin) for a, b in SHAPES for ns in SHARDS for pin in PINS]
    for g, got in zip(dense, ask(checker, "D", dense)):
        assert got == former_dense(*g), g
    fused = [(a, b, ns, cu, pin) for a, b in SHAPES for ns in SHARDS for cu in N_CU for pin in PINS]
    for g, got in zip(fused, ask(checker, "F", fused)):
        assert got == former_fused(*g), g
    generic = [(a, ns, pin) for a in SIDES + (1 << 22,) for ns in SHARDS for pin in PINS]
    for g, got in zip(generic, ask(checker, "G", generic)):
        assert got == former_generic(*g), g
    msum = [(a, b, ns, pin) for a, b in SHAPES for ns in SHARDS for pin in PINS]
    for g, got in zip(msum, ask(checker, "M", msum)):
        assert got == former_sum(*g), g
    cube = [(p, a, b, ns, pin) for p in (1, 4, 5, 8, 9, 65, 4096) for a, b in SHAPES for ns in SHARDS for pin in PINS]
    for g, got in zip(cube, ask(checker, "C", cube)):
        assert got == former_cube(*g), g
    # the rule itself: the floor stops the halving, a pin replaces the result below the floor too, n_cu <= 0 counts as 1
    assert ask(checker, "R", [(1, 1, 2, 4096, 0), (1, 1, 1, 4096, 0), (1, 1, 2, 4096, 1), (1, 1, 16, 4096, 0), (1, 4096, 1, 4096, 0)]) == [[2], [1], [1], [16], [16]]
    assert ask(checker, "F", [(32, 32, 1, 0, 0), (32, 32, 1, -5, 0)]) == [[1, 16, 1], [1, 16, 1]]


def test_the_pinned_cases(checker):
    spb = lambda kind, g, at: ask(checker, kind, [g])[0][at]
    assert ask(checker, "D", [(32, 32, 1024, 0)]) == [[1, 1, 1, 4, 4096]]
    assert spb("D", (32, 32, 1, 0), 3) == 2  # the floor
    assert spb("D", (32, 32, 1024, 1), 3) == 1 and spb("D", (32, 32, 1, 1), 3) == 1  # a pin goes below it
    assert spb("F", (32, 32, 256, 256, 0), 1) == 16
    assert spb("F", (32, 32, 64, 256, 0), 1) == 4
    assert ask(checker, "G", [(2, 64, 0)]) == [[1, 1, 1024]]
    assert ask(checker, "M", [(128, 128, 8, 0)]) == [[16, 1, 2048]]
    assert [spb("M", (128, 128, 8, pin), 1) for pin in PINS] == [1] * len(PINS)  # the pin is ignored
    assert [spb("G", (2, 64, pin), 1) for pin in PINS] == [1] * len(PINS)
    assert ask(checker, "C", [(8, 32, 32, 256, 0)]) == [[8, 1, 2, 2048]]


def test_the_path_and_the_pass(checker):
    paths = [(a, b, f, d, m) for a, b in SHAPES for f in (0, 1) for d in (0, 1) for m in (-1, 0, 1)]
    seen = set()
    for g, got in zip(paths, ask(checker, "P", paths)):
        assert got == [former_path(*g)], g
        seen.add(got[0])
    assert seen == {ROWS_VS_FILTER, DENSE, FUSED, GENERIC}
    path = lambda *g: ask(checker, "P", [g])[0][0]
    assert path(4, 4, 1, 0, -1) == FUSED and path(4, 4, 0, 0, -1) == FUSED  # 16 pairs on encoded rows
    assert path(3, 5, 1, 0, -1) == GENERIC and path(3, 5, 1, 0, 1) == FUSED and path(4, 4, 1, 0, 0) == GENERIC  # 15 pairs; the pins
    assert [path(200, 1, 0, d, m) for d in (0, 1) for m in (-1, 0, 1)] == [ROWS_VS_FILTER] * 6  # whatever matrix_fused says
    assert [path(200, 1, 1, d, m) for d in (0, 1) for m in (-1, 0, 1)] == [GENERIC] * 6
    assert path(9, 8, 1, 1, 1) == DENSE  # dense batches never decode

    passes = [(ns, a, b, kb, keep) for ns in SHARDS for a, b in SHAPES for kb in PASS_KB for keep in (0, 1)]
    several = 0
    for g, got in zip(passes, ask(checker, "S", passes)):
        assert got == [former_pass_shards(*g)] and 1 <= got[0] <= g[0], g
        several += got[0] < g[0]
    assert several > 100
    assert ask(checker, "S", [(1024, 4096, 4096, 1 << 20, 0), (1024, 4096, 4096, 1 << 20, 1), (1024, 4096, 4096, 1, 1)]) == [[8], [1024], [1024]]
    # the passes tests/test_gpu_prepared.py relies on: 72 cells are 576 B, so matrix_pass_kb = 1 holds one of 3 shards; 200 cells too
    assert ask(checker, "S", [(3, 9, 8, 1, 0), (3, 200, 1, 1, 0), (3, 9, 8, 1 << 20, 0)]) == [[1], [1], [3]]
