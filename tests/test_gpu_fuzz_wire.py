"""Seeded structural fuzz of the serialised uploads on the GPU: fbk_batch_upload_roaring (Pilosa and official images, the ops-log
replay), fbk_rbf_find_root + fbk_batch_upload_rbf, over the cases of tests/wire_fuzz_gen.py (FBK_TEST_SEED, FBK_FUZZ_ITERS).

Valid images must come back bit for bit, with the oracle's container types and counts, re-serialise by the rules tests/test_gpu_wire.py
and tests/test_gpu_rbf.py fix, and work as operands.  Mutants: the stand-alone host program (tests/cpp/fuzz_wire_parse.cpp, built
without sanitizers) first runs the host parsers over the iteration's own corpus and checks what the device side relies on — a
violation fails the test before anything is uploaded.  Then every mutant is uploaded: one the host refuses must fail with the very
message the program printed and leave no batch; one the host accepts must hold the oracle's bits, or be refused by the device check
exactly when the oracle's containers break the invariants it enforces.  After every refusal a known-good image is uploaded and
checked.  A HIP error from any call ends the whole session (pytest.exit): nothing more runs on a device that has faulted."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import datagen as D
import wire_fuzz_gen as G
from featurebase_amd import lib as L
from featurebase_amd.roaring import Batch
from test_gpu_wire import batch_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_REFUSALS = ("array container not strictly ascending", "run container intervals overlap or are unordered")


@contextlib.contextmanager
def hip_guard(case, item):
    """FBK_E_HIP from any call is a finding, and the end of the session"""
    try:
        yield
    except L.FbkError as e:
        if e.code == L.FBK_E_HIP:
            pytest.exit(f"FBK_E_HIP at {case.where(item)} (mutation class {item.tag}): {e}; no further GPU work", returncode=3)
        raise


def upload(ctx, case, item):
    """-> (status, message, batch or None, row ids) straight from the C entry points, so that a failing call's handle can be looked at"""
    h, n, raw = C.c_void_p(), C.c_uint32(), item.raw
    if item.kind == 1:
        pg = C.c_uint32()
        rc = ctx.lib.fbk_rbf_find_root(raw, len(raw), item.name.encode(), C.byref(pg))
        if rc == L.FBK_OK:
            cap = max(len(raw) // 20, 1)
            ids = np.zeros(cap, dtype=np.uint64)
            rc = ctx.lib.fbk_batch_upload_rbf(ctx.h, raw, len(raw), pg.value, C.byref(h), ids.ctypes.data, cap, C.byref(n))
    else:
        cap = max(len(raw) // 2, 1)
        ids = np.zeros(cap, dtype=np.uint64)
        rc = ctx.lib.fbk_batch_upload_roaring(ctx.h, raw, len(raw), C.byref(h), ids.ctypes.data, cap, C.byref(n))
    if rc != L.FBK_OK:
        msg = (ctx.lib.fbk_last_error(None) or b"?").decode(errors="replace")
        if rc == L.FBK_E_HIP:
            pytest.exit(f"FBK_E_HIP at {case.where(item)} (mutation class {item.tag}): {msg}; no further GPU work", returncode=3)
        return rc, msg, (Batch(ctx, h.value) if h.value else None), None
    return rc, "", Batch(ctx, h.value), ids[: n.value].copy()


def bits_np(batch) -> np.ndarray:
    return G._bits_np([(k, c.words()) for row in batch.download() for k, c in sorted(row.items())])


@pytest.fixture(scope="module")
def checker():
    return G.build_checker(os.path.join(ROOT, "build", "fuzz_wire_parse"), sanitize=False)


@pytest.mark.parametrize("it", range(G.ITERS))
def test_fuzz_wire_valid_images(gpu_ctx, oracle, it):
    O = oracle
    case = G.case(it)
    for item in case.valid:
        where = case.where(item)
        o = G.oracle_verdict(O, item)
        assert o["ok"] and o["refused"] is None, where
        with hip_guard(case, item):
            rc, msg, batch, ids = upload(gpu_ctx, case, item)
            assert rc == L.FBK_OK, f"{where}: {msg}"
            bits = item.bits
            assert ids.tolist() == (sorted({b >> 20 for b in bits} | {k >> 4 for k, _, _ in o["conts"]}) if item.ops is None else
                                    sorted({b >> 20 for b in O.OBitmap.unmarshal(item.raw).slice()} | {v >> 20 for t, p in item.ops for v in
                                           ([p] if t < 2 else p if t < 4 else O.OBitmap.unmarshal(p).slice())})), where
            assert batch_bits(batch, ids) == bits, where
            cnt = batch.count(np.arange(len(ids)))
            assert int(cnt.sum()) == len(bits), where
            got = [(k, c.typ, c.n) for row in batch.download() for k, c in sorted(row.items())]
            if item.ops is not None:  # every container comes out Optimize()d: WriteTo of the replayed bitmap
                model = O.bitmap_from_values(bits)
                assert got == [(k, c.typ, c.n) for k, c in model.items()], where
                assert batch.to_roaring() == model.marshal(True), where
            elif item.kind == 1:
                assert got == o["conts"], where
                from oracle import pyrbf
                assert batch.to_roaring() == O.OBitmap.from_containers([(l[0], pyrbf.leaf_to_container(l)) for l in o["leaves"]]).marshal(False), where
            else:
                assert got == o["conts"], where
                assert batch.to_roaring() == (item.raw if item.fmt.startswith("pilosa") else O.OBitmap.unmarshal(item.raw).marshal(False)), where
            if len(ids):  # the uploaded slots work as operands: |row ∩ row| = |row|
                rows = np.arange(len(ids))
                assert gpu_ctx.intersection_count(batch, rows, batch, rows).tolist() == cnt.tolist(), where
            batch.free()


@pytest.mark.parametrize("it", range(G.ITERS))
def test_fuzz_wire_mutants(gpu_ctx, oracle, checker, tmp_path, it):
    O = oracle
    case = G.case(it)
    # the host parsers over this corpus, on the host: a contract violation (non-zero exit) fails here, before any upload
    verdicts = G.run_checker(checker, case.mutants, str(tmp_path / "corpus.bin"), repr(case))
    os.remove(tmp_path / "corpus.bin")
    good_raw, good_bits = G.known_good(O)
    good = G.Item(0, good_raw, "valid", "pilosa", good_bits, note="the known-good image")
    good_np = G.positions_np(good_bits)
    n_refused = n_device = n_equal = 0
    for item, v in zip(case.mutants, verdicts):
        where = case.where(item)
        with hip_guard(case, item):
            rc, msg, batch, ids = upload(gpu_ctx, case, item)
            if not v["ok"]:
                assert rc == L.FBK_E_INVALID and msg == v["msg"], f"{where}: status {rc} '{msg}', the host program said '{v['msg']}'"
                assert batch is None, f"{where}: a refused upload left a batch"
            else:
                o = G.oracle_verdict(O, item)
                assert o["ok"], f"{where}: the host accepts what the oracle rejects ({o.get('why')})"
                if o["refused"] is not None:
                    assert rc == L.FBK_E_INVALID and msg.endswith(DEVICE_REFUSALS), f"{where}: status {rc} '{msg}', the oracle's containers break the {o['refused']} invariant"
                    assert batch is None, f"{where}: a refused upload left a batch"
                    n_device += 1
                else:
                    assert rc == L.FBK_OK, f"{where}: status {rc} '{msg}' for containers the oracle finds in order"
                    assert np.array_equal(bits_np(batch), o["bits"]), where
                    batch.free()
                    n_equal += 1
            if rc != L.FBK_OK:  # a refusal must not leak state into the context
                n_refused += 1
                rc2, msg2, b2, ids2 = upload(gpu_ctx, case, good)
                assert rc2 == L.FBK_OK, f"{where}: the known-good image after the refusal: {msg2}"
                assert ids2.tolist() == [0, 5] and np.array_equal(bits_np(b2), good_np), f"{where}: the known-good image after the refusal"
                b2.free()
    assert n_refused and n_device and n_equal, (D.SEED, it, n_refused, n_device, n_equal)
