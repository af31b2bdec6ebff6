"""fst_shortest_path_lhs_batch and fst_device_shortest_path_lhs as far as no GPU is needed:
symbols, the header, the Python mirror and every argument check (they run before any device
work)."""
import ctypes as C
import inspect
import os
import re

import pytest

import libfst_amd as F
import libfst_amd.fst as FF
from test_lhs_batch_api import assert_invalid, mutated, two_items

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def poisoned():
    """An error return must leave the struct zeroed."""
    res = FF.FstBatchResult()
    res.num_strings = 77
    res.total_arcs = 99
    return res


def call_sp(lhs, n=1, flags=0):
    opts = FF.FstBatchOptions(-1, 0, flags, 0, 0)
    res = poisoned()
    cs = lhs.c_struct() if lhs is not None else None
    rc = F.lib().fst_shortest_path_lhs_batch(C.byref(cs) if cs is not None else None, n,
                                             C.byref(opts), C.byref(res))
    return rc, res


def test_symbols_header_and_mirror_parity():
    for name in ("fst_shortest_path_lhs_batch", "fst_device_shortest_path_lhs"):
        assert hasattr(F.lib(), name)
        assert name in FF.SIGNATURES
    with open(os.path.join(REPO, "include", "fst_batch.h")) as fh:
        header = fh.read()
    assert re.search(r"FstError fst_shortest_path_lhs_batch\(const FstLhsBatch\* lhs, "
                     r"uint32_t n,\s+const FstBatchOptions\* opts, FstBatchResult\* out\);",
                     header)
    assert re.search(r"FstError fst_device_shortest_path_lhs\(const FstLhsBatch\* d_lhs, "
                     r"uint32_t n,\s+const FstBatchOptions\* opts, const FstDeviceBatch\* out,"
                     r"\s+void\* stream\);", header)
    assert re.search(r"12 = fst_shortest_path_lhs_batch", header)      # FstLaunchStats.engine
    res, args = FF.SIGNATURES["fst_shortest_path_lhs_batch"]
    assert res is C.c_int and len(args) == 4
    res, args = FF.SIGNATURES["fst_device_shortest_path_lhs"]
    assert res is C.c_int and len(args) == 5
    assert callable(F.shortest_path_lhs_batch)
    assert F.shortest_path_lhs_batch is FF.shortest_path_lhs_batch
    params = inspect.signature(F.shortest_path_lhs_batch).parameters
    assert params["n"].default == 1
    # it takes what connect_lhs_batch takes
    assert set(inspect.signature(F.connect_lhs_batch).parameters) <= set(params)


def test_null_pointers():
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    assert F.lib().fst_shortest_path_lhs_batch(C.byref(cs), 1, C.byref(opts),
                                               None) == FF.FST_INVALID_ARG
    assert_invalid(*call_sp(None))
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        res = poisoned()
        rc = F.lib().fst_shortest_path_lhs_batch(C.byref(cs), 1, C.byref(opts), C.byref(res))
        assert_invalid(rc, res)


@pytest.mark.parametrize("what,change", [
    ("decreasing state_offsets", dict(state_offsets=(1, 6))),
    ("decreasing arc_offsets", dict(arc_offsets=(2, 0))),
    ("arc_offsets[0] != 0", dict(arc_offsets=(0, 1))),
    ("start beyond the item", dict(start=(0, 2))),
    ("start beyond the second item", dict(start=(1, 3))),
    ("nextstate beyond the item", dict(nextstates=(0, 2))),
    ("nextstate of another item's range", dict(nextstates=(3, 3))),
])
def test_malformed_batches(what, change):
    for n in (1, 0, 2):                      # the validator runs before n is looked at
        assert_invalid(*call_sp(mutated(**change), n=n))


def test_item_size_limits():
    lhs = F.LhsBatch([0, 1 << 30], [0], [0.0], [0, 0], [], [], [], [])
    assert_invalid(*call_sp(lhs))
    lhs = F.LhsBatch([0, 1], [0], [0.0], [0, 1 << 32], [1], [1], [0.0], [0])
    assert_invalid(*call_sp(lhs))


def test_unknown_option_flags():
    lhs = F.LhsBatch.from_fsts(two_items())
    for fl in (2, 0x80000001):
        assert_invalid(*call_sp(lhs, flags=fl))


def test_empty_batch_is_an_ok_result():
    for n in (1, 0, 2):
        rc, res = call_sp(F.LhsBatch.from_fsts([]), n=n)
        assert rc == FF.FST_OK
        assert res.num_strings == 0 and res.total_arcs == 0
        assert res.path_offsets[0] == 0
        F.lib().fst_batch_result_free(C.byref(res))
        assert bytes(res) == bytes(C.sizeof(res))
    got = F.shortest_path_lhs_batch(F.LhsBatch.from_fsts([]))
    assert len(got.status) == 0 and got.offsets.tolist() == [0]


def test_device_entry_argument_checks():
    one = 8  # a non-null address the checks never dereference
    lhs = FF.FstLhsBatch(1, one, one, one, one, one, one, one, one)
    out = FF.FstDeviceBatch()
    op = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    fn = F.lib().fst_device_shortest_path_lhs
    assert fn(None, 1, C.byref(op), C.byref(out), None) == FF.FST_INVALID_ARG
    assert fn(C.byref(lhs), 1, C.byref(op), None, None) == FF.FST_INVALID_ARG
    assert fn(C.byref(lhs), 1, C.byref(op), C.byref(out), None) == FF.FST_INVALID_ARG  # null arrays
    bad = FF.FstBatchOptions(-1, 0, 2, 0, 0)
    assert fn(C.byref(lhs), 1, C.byref(bad), C.byref(out), None) == FF.FST_INVALID_ARG
    for field in ("state_offsets", "start", "arc_offsets"):
        cs = FF.FstLhsBatch(1, one, one, one, one, one, one, one, one)
        setattr(cs, field, None)
        assert fn(C.byref(cs), 1, C.byref(op), C.byref(out), None) == FF.FST_INVALID_ARG
