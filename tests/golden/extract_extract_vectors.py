#!/usr/bin/env python3
"""Extract the data of executor_test.go TestExecutor_Execute_Extract mechanically, for the fields this project's host mirror can
hold: `set`, `mutex` (as a set field), `bsint` and `bool` (as a set field with rows 0 = false / 1 = true).  Written to
extract_vectors.json: the bits imported and cleared, the values set, the columns that exist, the field order of the query and
the expected table — per column and field null (Go: nil / a nil slice) or a list ([]uint64{..}, uint64(x) -> [x],
int64(x) -> [x], true -> [1], false -> [0]).  `ShardWidth` expressions are evaluated with ShardWidth = 2^20.

    python tests/golden/extract_extract_vectors.py <reference tree> [--check]

--check compares with the committed file instead of writing it (tests/test_extract_cpu.py does that when the tree is there)."""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "extract_vectors.json")
SHARD_WIDTH = 1 << 20
FIELDS = ("set", "mutex", "bsint", "bool")


def value(expr: str) -> int:
    e = expr.strip()
    assert re.fullmatch(r"[0-9ShardWidth+*() -]+", e), e
    return int(eval(e.replace("ShardWidth", str(SHARD_WIDTH)), {"__builtins__": {}}))


def func_body(src: str, name: str):
    m = re.search(r"^func %s\(t \*testing\.T\) \{" % name, src, re.M)
    end = src.index("\n}\n", m.end())
    return src[m.end():end], src.count("\n", 0, m.start()) + 1, src.count("\n", 0, end) + 2


def braces(text: str, at: int) -> str:
    """the text between the brace at text[at] and its partner"""
    assert text[at] == "{"
    depth, j = 1, at + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return text[at + 1:j - 1]


def split_items(text: str):
    items, cur, depth = [], "", 0
    for ch in text:
        if ch in "{(":
            depth += 1
        elif ch in "})":
            depth -= 1
        if ch == "," and depth == 0:
            items.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        items.append(cur.strip())
    return items


def entry(item: str):
    item = " ".join(item.split())
    if item == "nil" or re.fullmatch(r"\[\]\w+\(nil\)", item):
        return None
    if item in ("true", "false"):
        return [int(item == "true")]
    m = re.fullmatch(r"u?int64\((-?\d+)\)", item)
    if m:
        return [int(m.group(1))]
    m = re.fullmatch(r"\[\]uint64\{(.*)\}", item)
    assert m, item
    return [int(x) for x in split_items(m.group(1))]


def extract(ref: str):
    src = open(os.path.join(ref, "executor_test.go")).read()
    body, first, last = func_body(src, "TestExecutor_Execute_Extract")
    out = {"source": "executor_test.go:%d-%d TestExecutor_Execute_Extract" % (first, last), "shard_width": SHARD_WIDTH, "imported": {}, "cleared": [],
           "values": {}, "int_range": {}}
    for m in re.finditer(r'c\.ImportBits\(t, c\.Idx\(\), "(\w+)", \[\]\[2\]uint64\{(.*?)\n\t\}\)', body, re.S):
        if m.group(1) in FIELDS:
            out["imported"][m.group(1)] = [[value(a), value(b)] for a, b in re.findall(r"\{([^,{}]+), ([^{}]+)\}", m.group(2))]
    for m in re.finditer(r'fmt\.Sprintf\("Clear\(%d, (\w+)=(\d+)\)", ([^)]+)\)', body):
        out["cleared"].append({"field": m.group(1), "row": int(m.group(2)), "column": value(m.group(3))})
    for m in re.finditer(r"Set\((\d+), (\w+)=([^,)\n]+)\)", body):
        col, field, v = int(m.group(1)), m.group(2), m.group(3).strip()
        if field == "bool":
            out["imported"].setdefault("bool", []).append([int(v == "true"), col])
        elif field == "bsint":
            out["values"].setdefault("bsint", []).append([col, int(v)])
    m = re.search(r'"bsint", pilosa\.OptFieldTypeInt\((-?\d+), (-?\d+)\)', body)
    out["int_range"]["bsint"] = [int(m.group(1)), int(m.group(2))]
    order = re.findall(r"Rows\((\w+)\)", re.search(r"`Extract\(All\(\), (.*?)`", body).group(1))
    out["query_fields"] = order
    out["fields"] = [f for f in order if f in FIELDS]
    table = braces(body, body.index("Columns: []pilosa.ExtractedTableColumn{") + len("Columns: []pilosa.ExtractedTableColumn"))
    out["columns"] = []
    for m in re.finditer(r"Column: pilosa\.KeyOrID\{ID: ([^}]+)\},\s*Rows: \[\]interface\{\}", table):
        items = split_items(braces(table, m.end()))
        assert len(items) == len(order)
        out["columns"].append({"column": value(m.group(1)), "rows": [entry(items[order.index(f)]) for f in out["fields"]]})
    out["existence"] = [c["column"] for c in out["columns"]]
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--check"]
    if not args:
        sys.exit(__doc__)
    got = extract(args[0])
    if "--check" in sys.argv:
        sys.exit(0 if got == json.load(open(OUT)) else "extract_vectors.json differs from the reference source")
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print("wrote", OUT, len(got["columns"]), "columns")


if __name__ == "__main__":
    main()
