"""Executor::Sort / ExtractSorted (include/fbk_executor.hpp) against the reference's TestExecutor_Sort (tests/golden/sort_vectors.json,
the int query) and a std::stable_sort brute force in tests/cpp/test_sort.cpp, built the way tests/test_cpp_extract.py builds its
program; the compile check runs everywhere, the run needs the GPU."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_sort.cpp")
BIN = os.path.join(ROOT, "build", "test_sort")
TABLE = os.path.join(ROOT, "build", "sort_vectors.txt")


def compile_it():
    import __graft_entry__ as g

    g.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "featurebase_amd", "csrc")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib, "-lfbk", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", BIN]
    )


def write_table():
    """the golden data as the lines test_sort.cpp reads: value COL V | query PREDICATE LIMIT OFFSET DESC | want COL V"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "sort_vectors.json")))
    q = [q for q in g["queries"] if q["supported"]]
    assert len(q) == 1 and q[0]["field"] == "bsint" and q[0]["rows_field"] == "bsint"
    pred = int(re.fullmatch(r"Row\(bsint > (-?\d+)\)", q[0]["filter"]).group(1))
    lines = [f"value {c} {v}" for c, v in g["values"]["bsint"]]
    lines.append(f"query {pred} {q[0]['limit']} {q[0]['offset']} {int(q[0]['desc'])}")
    lines += [f"want {c['column']} {c['rows'][0]}" for c in q[0]["columns"]]
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_sort_compiles():
    compile_it()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_sort_on_gpu():
    compile_it()
    write_table()
    out = subprocess.run([BIN, TABLE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sort ok" in out.stdout
