"""Executor::GroupBy with having / sort / offset / limit (include/fbk_executor.hpp: GroupByOptions, the fbk_*_select calls when the
GroupBy fits one library call, the blocked path plus the host selection otherwise) against the reference's pipeline run on the
output of the existing GroupBy, in tests/cpp/test_groupby_select.cpp, built the way tests/test_cpp_groupby_cube.py builds its program;
the compile check and the sort-string parser's cases run everywhere, the rest needs the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_groupby_select.cpp")
BIN = os.path.join(ROOT, "build", "test_groupby_select")


def compile_it():
    import __graft_entry__ as g

    g.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "featurebase_amd", "csrc")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib, "-lfbk", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", BIN]
    )


def test_groupby_select_compiles_and_parses_sort_strings():
    compile_it()
    out = subprocess.run([BIN, "--parser-only"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "groupby select parser ok" in out.stdout


@pytest.mark.gpu
def test_groupby_select_on_gpu():
    compile_it()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "groupby select ok" in out.stdout
