"""The host parsers of the serialised uploads (featurebase_amd/csrc/fbk_wire_parse.h) over the seeded fuzz corpus of
tests/wire_fuzz_gen.py, in a stand-alone host program (tests/cpp/fuzz_wire_parse.cpp) built with the address and undefined-behaviour
sanitizers: no read past an image, and every accepted image keeps the contract the device side relies on (the program exits non-zero
otherwise).  Verdicts are compared with the oracle's readers; three coverage conditions keep the fuzz from passing by never getting
anywhere.  No GPU."""
import collections
import os
import re

import numpy as np
import pytest

import datagen as D
import wire_fuzz_gen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "featurebase_amd", "csrc", "fbk_wire_parse.h")

# The parser may refuse what the oracle's readers take ONLY with these messages (regular expressions, matched at the start of the
# message); each with the comment of the code it comes from.  The other direction (the parser takes what the oracle refuses) is never
# allowed.  For RBF files the list names nearly every message of rbf_walk and fbk_rbf_find_root: oracle/pyrbf.py is a reader of
# well-formed files that slices and unpacks whatever is there, so "the parser refuses, the oracle reads" says nothing about an RBF
# mutant.  What the RBF mutants do check is the other direction, the contract of every accepted file, and the sanitizers.
PARSER_STRICTER = {
    "roaring: container keys not ascending":
        "wire_upload lays containers out over 'the distinct key >> 4 of the containers' in one ascending walk; the oracle's bitmap sorts / replaces on put",
    "roaring: run container with more than 32768 intervals":
        "disjoint non-empty intervals of 16-bit values number at most 32768; the oracle's reader copies whatever count the header states",
    "rbf: b-tree deeper than 16 levels": "rbf_walk bounds its recursion; oracle/pyrbf.py recurses as deep as the file says",
    r"rbf: page \d+ is reachable twice":
        "'a tree visits every page once: a branch cell that points back at an ancestor (or a page shared by two parents) is corruption'",
    r"rbf: page \d+ is neither a leaf nor a branch": "page flags are leaf or branch (rbf.go:189-206); the oracle's reader only asserts",
    "rbf: bitmap page ": "a bitmap page referenced twice (or one that is a page of the tree) is corruption; the oracle's reader reads it again",
    "rbf: page read out of bounds": "'page read out of bounds' (rbf/tx.go readPage); the oracle's reader slices an empty page and may find zero cells in it",
    "rbf: cannot read page": "toPgno(cell.Data) outside the file; numpy reads a short slice as an error, an in-bounds page 0 as a bitmap",
    "rbf: BitN out of range": "a container holds at most 65536 values; the oracle's reader passes BitN through",
    "rbf: leaf cell keys not ascending": "the b-tree is ordered by key; the oracle's reader returns cells in page order",
    "rbf: branch page ": "an empty branch page has no subtree; the oracle's reader walks zero children",
    "rbf: cell index overruns the page": "10 + 2 * cellN bytes of index must fit the 8 KiB page; the oracle's reader reads on into the next page",
    "rbf: branch cell out of bounds": "a cell lies inside its page; the oracle's reader slices the page and unpacks what is there",
    "rbf: leaf cell out of bounds": "a cell lies inside its page; the oracle's reader slices the page and unpacks what is there",
    "rbf: leaf cell data overruns the page": "cell data lies inside its page; numpy takes a short read only when the count does not fit the slice",
    "rbf: bitmap pointer out of bounds": "the 4-byte page number of a bitmap-pointer cell lies inside the page",
    "rbf: inline bitmap cell in a stored page": "'inline bitmap: only exists transiently inside the reference (rbf.go:52)'",
    "rbf: invalid container type": "ContainerType, rbf.go:63-69",
    "rbf: short root record buffer": "a root record's name lies inside its page; the oracle's find_root slices",
    "rbf: root record page out of bounds": "root record pages lie inside the file and their chain ends; the oracle's find_root follows any pointer",
    "rbf: bitmap not found": "ErrBitmapNotFound; (the oracle raises KeyError: listed for completeness)",
    "rbf: missing meta page magic": "a file of less than two pages has no root records; the oracle's find_root asserts the magic only",
}
# fail() messages of the moved parsers (as fail_messages() gives them) that no mutant of test size can produce, with the reason.  (The three the issue names — the
# 4 GiB offset wrap, "too many rows", allocation failure — have no message of their own in fbk_wire_parse.h: the wrap is arithmetic
# inside wire_parse that ends in "payload out of bounds", the other two are raised by wire_upload, outside the moved code.)
UNREACHABLE = {}

# What wire_parse / wire_push can say about a nested image of the ops log.  The reference drops the error of a malformed nested
# image, upload_roaring_with_ops reports it: only these may stand against an oracle that read the log and dropped the image.
NESTED_IMAGE_MESSAGES = (
    "invalid data: not long enough to be a roaring header", "wrong roaring version", "insufficient data for header + offsets",
    "roaring: run count out of bounds", "roaring: run container with more than 32768 intervals", "roaring: unknown container type",
    "roaring: container payload out of bounds", "roaring: container keys not ascending", "malformed bitmap, is-run bitmap overruns buffer",
    "did not find expected serialCookie in header", "it is logically impossible to have more than (1<<16) containers",
    "malformed bitmap, key-cardinality slice overruns buffer", "insufficient data for offsets", "unknown roaring magic number")


def fail_messages(src: str):
    """every distinct fail() call of the header as the tuple of the string literals of its message, in order: what lies between
    two literals is a number or a name put in at run time"""
    out = set()
    for m in re.finditer(r"\bfail\(FBK_E_\w+,", src):
        i, depth, quoted = m.end(), 1, False
        while depth:
            ch = src[i]
            if quoted:
                i += ch == "\\"
                quoted = ch != '"'
            elif ch == '"':
                quoted = True
            else:
                depth += (ch == "(") - (ch == ")")
            i += 1
        lits = tuple(re.findall(r'"((?:[^"\\]|\\.)*)"', src[m.end(): i - 1]))
        assert lits and not any("\\" in lit for lit in lits), src[m.start(): i]
        out.add(lits)
    return sorted(out)


@pytest.fixture(scope="module")
def corpus(oracle, tmp_path_factory):
    exe = G.build_checker(os.path.join(ROOT, "build", "fuzz_wire_parse_san"), sanitize=True)
    tmp = tmp_path_factory.mktemp("wire_fuzz")
    out = []
    for it in range(G.ITERS):
        case = G.case(it)
        verdicts = G.run_checker(exe, case.items, str(tmp / f"corpus_{it}.bin"), repr(case))
        os.remove(tmp / f"corpus_{it}.bin")
        for item, v in zip(case.items, verdicts):
            o = G.oracle_verdict(oracle, item)
            if item.tag == "valid":
                assert o.get("ok") and np.array_equal(o["bits"], G.positions_np(item.bits)), \
                    f"{case.where(item)}: the generator's expectation is not what the oracle reads ({o.get('why')})"
            o.pop("bits", None)  # (not kept: some hundred MB over the corpus)
            o.pop("leaves", None)
            out.append((case.where(item), G.Item(item.kind, b"", item.tag, item.fmt, ops=item.ops, name=item.name), v, o))
    return out


def _descs(v):
    return v["base"] + [d for op in v["ops"] for d in op[2]]


def test_valid_images_are_accepted_and_read_as_the_oracle_reads_them(corpus):
    n = 0
    for where, item, v, o in corpus:
        if item.tag != "valid":
            continue
        n += 1
        assert v["ok"], f"{where}: rejected: {v.get('msg')}"
        assert o["ok"], f"{where}: the oracle rejects a valid image: {o.get('why')}"
        assert o["refused"] is None, where
        assert [(d[0], d[1], d[2]) for d in v["base"]] == o["conts"], where
        if item.kind == 1:
            assert v["root"] == o["root"], where
        if item.ops is not None:
            assert [op[0] for op in v["ops"]] == [t for t, _ in item.ops], where
    assert n >= 13 * G.ITERS


def test_mutants_verdict_against_the_oracle(corpus):
    bad = []
    for where, item, v, o in corpus:
        if item.tag == "valid" or v["ok"] == o["ok"]:
            continue
        if v["ok"]:
            bad.append(f"{where}: the parser accepts what the oracle rejects ({o['why']})")
        elif o["nested_dropped"] and v["msg"].startswith(NESTED_IMAGE_MESSAGES):
            continue  # 'the reference drops the error of a malformed nested image — here it is reported' (upload_roaring_with_ops)
        elif not any(re.match(p, v["msg"]) for p in PARSER_STRICTER):
            bad.append(f"{where}: the parser rejects ({v['msg']}) what the oracle accepts")
    assert not bad, f"{len(bad)} disagreements:\n" + "\n".join(bad[:40])


def test_coverage_every_message_every_branch_both_outcomes(corpus):
    # (a) every distinct fail() message of the moved parsers comes out of some mutant: all of its literals, in their order
    literals = fail_messages(open(HEADER).read())
    assert len(literals) >= 36 and ("rbf: page ", " is reachable twice (cycle or shared page in the b-tree)") in literals, literals
    seen = sorted({v["msg"] for _, item, v, _ in corpus if item.tag != "valid" and not v["ok"]})
    missing = [m for m in literals if m not in UNREACHABLE and not any(re.match(".*".join(map(re.escape, m)), s, re.S) for s in seen)]
    assert not missing, f"no mutant produces: {missing} (seed {D.SEED:#x}, {G.ITERS} iterations)"
    # (b) every branch of k_wire_copy is taken by a descriptor of a valid image
    branches = collections.Counter(d[7] for _, item, v, _ in corpus if item.tag == "valid" and v["ok"] for d in _descs(v))
    assert set(branches) == set(range(6)), f"k_wire_copy branches taken by the valid images: {dict(branches)}"
    # (c) both outcomes of every class.  At least a third of the mutants of a class are rejected by the host parser.  Only for the
    # classes of G.PAYLOAD_CLASSES, edits inside a payload that leave the structure intact and that the host parser therefore cannot
    # see, "rejected" also counts the container invariants the device check enforces (arrays strictly ascending, runs ordered and
    # disjoint), judged by the oracle; and at least one mutant of each of these classes is accepted by the host parser.
    tot, host_rejects, device_refuses = collections.Counter(), collections.Counter(), collections.Counter()
    for _, item, v, o in corpus:
        if item.tag == "valid":
            continue
        tot[item.tag] += 1
        host_rejects[item.tag] += not v["ok"]
        device_refuses[item.tag] += bool(v["ok"] and o["ok"] and o["refused"] is not None)
    assert set(tot) == set(G.MUTATION_CLASSES), set(G.MUTATION_CLASSES) ^ set(tot)
    table = {c: (tot[c], host_rejects[c], device_refuses[c]) for c in G.MUTATION_CLASSES}
    print("(mutants, rejected by the host parser, accepted by it and against the container invariants):", table)
    for c in G.MUTATION_CLASSES:
        rejected = host_rejects[c] + (device_refuses[c] if c in G.PAYLOAD_CLASSES else 0)
        assert 3 * rejected >= tot[c], f"class {c}: (mutants, rejected by the host, refused by the device check) = {table[c]}; all: {table}"
    for c in G.PAYLOAD_CLASSES:
        assert host_rejects[c] < tot[c], f"payload-edit class {c}: the host parser accepts none of {table[c]}"
