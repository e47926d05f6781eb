"""Executor::GroupByQuantiles (include/fbk_executor.hpp) against a brute force in tests/cpp/test_groupby_quantiles.cpp,
built the way tests/test_cpp_host_mirror.py builds its programs; the compile check runs everywhere, the run needs the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_groupby_quantiles.cpp")
BIN = os.path.join(ROOT, "build", "test_groupby_quantiles")


def compile_it():
    import __graft_entry__ as g

    g.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "featurebase_amd", "csrc")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib, "-lfbk", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", BIN]
    )


def test_groupby_quantiles_compiles():
    compile_it()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_groupby_quantiles_on_gpu():
    compile_it()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "groupby quantiles ok" in out.stdout
