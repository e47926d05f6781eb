#!/usr/bin/env python3
"""Extract the data of executor_test.go TestExecutor_Sort mechanically: the values set on `bsint`, and per query its text, whether
this project supports it (Sort by an int field; the bool and keyed-mutex queries are recorded but marked unsupported) and the
expected table.  Written to sort_vectors.json.

    python tests/golden/extract_sort_vectors.py <reference tree> [--check]

--check compares with the committed file instead of writing it (tests/test_sort_cpu.py does that when the tree is there)."""
import json
import os
import re
import sys

from extract_extract_vectors import braces, func_body, split_items

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sort_vectors.json")


def cell(item: str):
    item = " ".join(item.split())
    if item in ("true", "false"):
        return item == "true"
    m = re.fullmatch(r"int64\((-?\d+)\)", item)
    if m:
        return int(m.group(1))
    m = re.fullmatch(r'"(.*)"', item)
    assert m, item
    return m.group(1)


def extract(ref: str):
    src = open(os.path.join(ref, "executor_test.go")).read()
    body, first, last = func_body(src, "TestExecutor_Sort")
    out = {"source": "executor_test.go:%d-%d TestExecutor_Sort" % (first, last), "shard_width": 1 << 20}
    out["values"] = {"bsint": [[int(c), int(v)] for c, v in re.findall(r"Set\((\d+), bsint = (-?\d+)\)", body)]}
    queries = re.findall(r'^\t\t\t"(Extract\(Sort\(.*)",$', body, re.M)
    tables = []
    for m in re.finditer(r"Columns: \[\]pilosa\.ExtractedTableColumn", body):
        cols = []
        text = braces(body, m.end())
        for c in re.finditer(r"Column: pilosa\.KeyOrID\{ID: (\d+)\},\s*Rows: \[\]interface\{\}", text):
            cols.append({"column": int(c.group(1)), "rows": [cell(x) for x in split_items(braces(text, c.end()))]})
        tables.append(cols)
    assert len(queries) == len(tables) == 3
    out["queries"] = []
    for q, t in zip(queries, tables):
        m = re.fullmatch(r"Extract\(Sort\((.*?), field = (\w+)((?:, [\w-]+ = \w+)*)\), Rows\((\w+)\)\)", q)
        args = dict(a.split(" = ") for a in m.group(3).split(", ") if a)
        out["queries"].append({"pql": q, "filter": m.group(1), "field": m.group(2), "limit": int(args["limit"]) if "limit" in args else None,
                               "offset": int(args.get("offset", 0)), "desc": args.get("sort-desc") == "true", "rows_field": m.group(4),
                               "supported": m.group(2) == "bsint", "columns": t})
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--check"]
    if not args:
        sys.exit(__doc__)
    got = extract(args[0])
    if "--check" in sys.argv:
        sys.exit(0 if got == json.load(open(OUT)) else "sort_vectors.json differs from the reference source")
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print("wrote", OUT, len(got["queries"]), "queries")


if __name__ == "__main__":
    main()
