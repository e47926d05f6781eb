"""Executor::eval with fuse_calls (include/fbk_executor.hpp: a call tree as ONE fbk_expr_eval / fbk_expr_count) against the
node-by-node path, over the set-operation and Count cases of tests/golden/executor_vectors.json and a seeded index in
tests/cpp/test_expr.cpp, built the way tests/test_cpp_sort.py builds its program; the compile check runs everywhere, the run
needs the GPU."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_expr.cpp")
BIN = os.path.join(ROOT, "build", "test_expr")
TABLE = os.path.join(ROOT, "build", "expr_vectors.txt")


def compile_it():
    import __graft_entry__ as g

    g.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "featurebase_amd", "csrc")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib, "-lfbk", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", BIN]
    )


def write_table():
    """the golden cases as the lines test_expr.cpp reads: case NAME | bit FIELD ROW COL | query OP FIELD ROW [ROW] | columns C... | count N"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "executor_vectors.json")))
    lines = []
    for c in g["cases"]:
        lines.append(f"case {c['test']}")
        lines += [f"bit {f} {r} {col}" for f, r, col in c["bits"]]
        m = re.fullmatch(r"(\w+)\((.*)\)", c["query"])
        rows = re.findall(r"Row\((\w+)=(\d+)\)", m.group(2))
        assert rows and len({f for f, _ in rows}) == 1 and m.group(1) in ("Difference", "Intersect", "Union", "Xor", "Count"), c["query"]
        lines.append(f"query {m.group(1)} {rows[0][0]} " + " ".join(r for _, r in rows))
        lines.append("columns " + " ".join(str(x) for x in c["columns"]) if "columns" in c else f"count {c['count']}")
    assert len(g["cases"]) == 5
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_expr_compiles():
    compile_it()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_expr_on_gpu():
    compile_it()
    write_table()
    out = subprocess.run([BIN, TABLE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "expr ok" in out.stdout
