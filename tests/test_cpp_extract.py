"""Executor::Extract (include/fbk_executor.hpp) against the reference's TestExecutor_Execute_Extract table
(tests/golden/extract_vectors.json) and a brute force in tests/cpp/test_extract.cpp, built the way tests/test_cpp_groupby_distinct.py
builds its program; the compile check runs everywhere, the run needs the GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_extract.cpp")
BIN = os.path.join(ROOT, "build", "test_extract")
TABLE = os.path.join(ROOT, "build", "extract_vectors.txt")


def compile_it():
    import __graft_entry__ as g

    g.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "featurebase_amd", "csrc")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib, "-lfbk", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", BIN]
    )


def write_table():
    """the golden data as the lines test_extract.cpp reads.  The reference clears one bit and the column stays in existence; the
    mirror's Index has no Clear, so cleared bits are left out and every existing column gets a bit in a helper field that is not
    extracted."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "extract_vectors.json")))
    cleared = {(c["field"], c["row"], c["column"]) for c in g["cleared"]}
    lines = ["setfield helper"] + [f"setfield {f}" for f in g["imported"]] + [f"intfield {f} {lo} {hi}" for f, (lo, hi) in g["int_range"].items()]
    lines += [f"bit helper 0 {c}" for c in g["existence"]]
    lines += [f"bit {f} {r} {c}" for f, bits in g["imported"].items() for r, c in bits if (f, r, c) not in cleared]
    lines += [f"value {f} {c} {v}" for f, vals in g["values"].items() for c, v in vals]
    lines.append("fields " + " ".join(g["fields"]))
    for col in g["columns"]:
        lines.append(f"col {col['column']} " + " ".join("null" if r is None else " ".join(map(str, [len(r)] + r)) for r in col["rows"]))
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_extract_compiles():
    compile_it()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_extract_on_gpu():
    compile_it()
    write_table()
    out = subprocess.run([BIN, TABLE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "extract ok" in out.stdout
