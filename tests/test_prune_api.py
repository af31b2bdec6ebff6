"""fst_prune_lhs_batch and fst_device_prune_lhs as far as no GPU is needed: symbols, the header,
the Python mirror, every argument check (they run before any device work)."""
import ctypes as C
import math
import os
import re

import pytest

import libfst_amd as F
import libfst_amd.fst as FF
from test_lattice_batch_api import assert_invalid, poisoned
from test_lhs_batch_api import mutated, two_items

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan


def call_prune(lhs, beam, flags=0):
    opts = FF.FstBatchOptions(-1, 0, flags, 0, 0)
    res = poisoned()
    cs = lhs.c_struct() if lhs is not None else None
    rc = F.lib().fst_prune_lhs_batch(C.byref(cs) if cs is not None else None, beam,
                                     C.byref(opts), C.byref(res))
    return rc, res


def test_symbols_header_and_mirror_parity():
    for name in ("fst_prune_lhs_batch", "fst_device_prune_lhs"):
        assert hasattr(F.lib(), name)
        assert name in FF.SIGNATURES
    with open(os.path.join(REPO, "include", "fst_batch.h")) as fh:
        header = fh.read()
    assert re.search(r"FstError fst_prune_lhs_batch\(const FstLhsBatch\* lhs, double beam, "
                     r"const FstBatchOptions\* opts,\s+FstLatticeBatch\* out\);", header)
    assert re.search(r"FstError fst_device_prune_lhs\(const FstLhsBatch\* d_lhs, double beam, "
                     r"const FstBatchOptions\* opts,\s+const FstDeviceLattices\* out, "
                     r"uint64_t needed\[2\], void\* stream\);", header)
    assert re.search(r"15 = fst_prune_lhs_batch and fst_device_prune_lhs", header)
    res, args = FF.SIGNATURES["fst_prune_lhs_batch"]
    assert res is C.c_int and len(args) == 4 and args[1] is C.c_double
    res, args = FF.SIGNATURES["fst_device_prune_lhs"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.c_double
    assert callable(F.prune_lhs_batch)


@pytest.mark.parametrize("beam", [NAN, -1.0, -INF, -1e-300])
def test_bad_beam_is_refused_before_the_batch_is_read(beam):
    assert_invalid(*call_prune(F.LhsBatch.from_fsts(two_items()), beam))
    # before lhs's arrays are read: pointers nothing may dereference
    cs = FF.FstLhsBatch(3, 8, 8, 8, 8, 8, 8, 8, 8)
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    res = poisoned()
    assert_invalid(F.lib().fst_prune_lhs_batch(C.byref(cs), beam, C.byref(opts), C.byref(res)),
                   res)
    with pytest.raises(RuntimeError, match="fst_prune_lhs_batch failed"):
        F.prune_lhs_batch(F.LhsBatch.from_fsts(two_items()), beam)


def test_null_pointers():
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    assert F.lib().fst_prune_lhs_batch(C.byref(cs), 1.0, C.byref(opts), None) == FF.FST_INVALID_ARG
    assert_invalid(*call_prune(None, 1.0))
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        res = poisoned()
        rc = F.lib().fst_prune_lhs_batch(C.byref(cs), 1.0, C.byref(opts), C.byref(res))
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
    assert_invalid(*call_prune(mutated(**change), 1.0))
    with pytest.raises(RuntimeError, match="fst_prune_lhs_batch failed"):
        F.prune_lhs_batch(mutated(**change), 1.0)


def test_unknown_option_flags():
    lhs = F.LhsBatch.from_fsts(two_items())
    for fl in (2, 0x80000001):
        assert_invalid(*call_prune(lhs, 1.0, flags=fl))


@pytest.mark.parametrize("beam", [0.0, -0.0, 2.5, INF])
def test_empty_batch_is_an_ok_result(beam):
    """-0.0 is a valid beam; zero items end at the empty result before any device work."""
    rc, res = call_prune(F.LhsBatch.from_fsts([]), beam)
    assert rc == FF.FST_OK
    assert res.fsts.num_fsts == 0 and res.total_states == 0 and res.total_arcs == 0
    so = C.cast(res.fsts.state_offsets, C.POINTER(C.c_uint64))
    ao = C.cast(res.fsts.arc_offsets, C.POINTER(C.c_uint64))
    assert so[0] == 0 and ao[0] == 0
    F.lib().fst_lattice_batch_free(C.byref(res))
    assert bytes(res) == bytes(C.sizeof(res))
    got = F.prune_lhs_batch(F.LhsBatch.from_fsts([]), beam)
    assert len(got) == 0 and got.state_offsets.tolist() == [0] and got.arc_offsets.tolist() == [0]


def test_device_entry_argument_checks():
    one = 8  # a non-null address the checks never dereference
    lhs = FF.FstLhsBatch(1, one, one, one, one, one, one, one, one)
    full = FF.FstDeviceLattices(one, one, one, one, one, one, one, one, one, 4, 4)
    needed = (C.c_uint64 * 2)(7, 7)
    op = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    L = F.lib()
    for beam in (NAN, -1.0, -INF):
        assert L.fst_device_prune_lhs(C.byref(lhs), beam, C.byref(op), C.byref(full), needed,
                                      None) == FF.FST_INVALID_ARG
    assert L.fst_device_prune_lhs(None, 1.0, C.byref(op), C.byref(full), needed,
                                  None) == FF.FST_INVALID_ARG
    assert L.fst_device_prune_lhs(C.byref(lhs), 1.0, C.byref(op), None, needed,
                                  None) == FF.FST_INVALID_ARG
    assert L.fst_device_prune_lhs(C.byref(lhs), 1.0, C.byref(op), C.byref(full), None,
                                  None) == FF.FST_INVALID_ARG
    bad = FF.FstBatchOptions(-1, 0, 2, 0, 0)
    assert L.fst_device_prune_lhs(C.byref(lhs), 1.0, C.byref(bad), C.byref(full), needed,
                                  None) == FF.FST_INVALID_ARG
    for field in ("status", "state_offsets", "start", "final_weights", "arc_offsets", "ilabels",
                  "olabels", "weights", "nextstates"):
        o = FF.FstDeviceLattices(one, one, one, one, one, one, one, one, one, 4, 4)
        setattr(o, field, None)
        assert L.fst_device_prune_lhs(C.byref(lhs), 1.0, C.byref(op), C.byref(o), needed,
                                      None) == FF.FST_INVALID_ARG
    nostart = FF.FstLhsBatch(1, one, None, one, one, one, one, one, one)
    assert L.fst_device_prune_lhs(C.byref(nostart), 1.0, C.byref(op), C.byref(full), needed,
                                  None) == FF.FST_INVALID_ARG
    assert list(needed) == [7, 7]
