"""The lattice batch entries (fst_compose_frozen_batch, fst_compose_frozen_lhs_batch,
fst_lattice_batch_free, fst_device_compose_frozen): symbols, struct layouts and every
host-side argument check.  No GPU: the checks run before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libfst_amd as F
import libfst_amd.fst as FF
from test_lhs_batch_api import Handle, mutated, small_rhs, two_items

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ("fst_compose_frozen_batch", "fst_compose_frozen_lhs_batch", "fst_lattice_batch_free")
DEVICE = "fst_device_compose_frozen"


def poisoned():
    res = FF.FstLatticeBatch()
    res.fsts.num_fsts = 77       # an error return must leave the struct zeroed
    res.total_states = 5
    res.total_arcs = 99
    return res


def call_lhs(rhs, lhs, lattice_flags=0, flags=0):
    opts = FF.FstBatchOptions(-1, 0, flags, 0, 0)
    res = poisoned()
    cs = lhs.c_struct() if lhs is not None else None
    rc = F.lib().fst_compose_frozen_lhs_batch(rhs.h, C.byref(cs) if cs is not None else None,
                                              lattice_flags, C.byref(opts), C.byref(res))
    return rc, res


def call_chain(rhs, labels, offsets, lattice_flags=0, flags=0, num=None):
    opts = FF.FstBatchOptions(-1, 0, flags, 0, 0)
    res = poisoned()
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    n = num if num is not None else (len(off) - 1 if off is not None else 0)
    rc = F.lib().fst_compose_frozen_batch(rhs.h, None if lab is None else lab.ctypes.data,
                                          None if off is None else off.ctypes.data, n,
                                          lattice_flags, C.byref(opts), C.byref(res))
    return rc, res


def assert_invalid(rc, res):
    assert rc == FF.FST_INVALID_ARG
    assert bytes(res) == bytes(C.sizeof(res))


def header_fields(name):
    with open(os.path.join(REPO, "include", "fst_batch.h")) as fh:
        header = fh.read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        # `uint64_t a, b` declares two fields
        for part in decl.split(","):
            out.append(re.sub(r"[\s*]+", " ", part).strip().split(" ")[-1])
    return out


def test_symbols_and_struct_layouts():
    L = F.lib()
    for name in HOST + (DEVICE,):
        assert hasattr(L, name)
        assert name in FF.SIGNATURES
    fields = header_fields("FstLatticeBatch")
    assert fields == [f[0] for f in FF.FstLatticeBatch._fields_]
    assert fields == ["fsts", "status", "total_states", "total_arcs"]
    assert FF.FstLatticeBatch.fsts.offset == 0
    assert FF.FstLatticeBatch.status.offset == C.sizeof(FF.FstLhsBatch) == 72
    assert C.sizeof(FF.FstLatticeBatch) == 72 + 8 + 16
    fields = header_fields("FstDeviceLattices")
    assert fields == [f[0] for f in FF.FstDeviceLattices._fields_]
    assert fields == ["status", "state_offsets", "start", "final_weights", "arc_offsets",
                      "ilabels", "olabels", "weights", "nextstates", "state_capacity",
                      "arc_capacity"]
    assert C.sizeof(FF.FstDeviceLattices) == 11 * 8
    assert FF.FST_LATTICE_PROJECT_OUTPUT == 1 == F.FST_LATTICE_PROJECT_OUTPUT


def test_null_pointers():
    rhs = small_rhs()
    L = F.lib()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()
    off = np.array([0, 1, 2], np.uint64)
    lab = np.array([1, 1], np.uint32)
    # a null `out`
    assert L.fst_compose_frozen_lhs_batch(rhs.h, C.byref(cs), 0, C.byref(opts),
                                          None) == FF.FST_INVALID_ARG
    assert L.fst_compose_frozen_batch(rhs.h, lab.ctypes.data, off.ctypes.data, 2, 0,
                                      C.byref(opts), None) == FF.FST_INVALID_ARG
    # a null lhs, null arrays of it
    assert_invalid(*call_lhs(rhs, None))
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        res = poisoned()
        rc = L.fst_compose_frozen_lhs_batch(rhs.h, C.byref(cs), 0, C.byref(opts), C.byref(res))
        assert_invalid(rc, res)
    # null offsets; null labels of a batch that has labels
    assert_invalid(*call_chain(rhs, lab, None, num=2))
    assert_invalid(*call_chain(rhs, None, off))


@pytest.mark.parametrize("what,change", [
    ("decreasing state_offsets", dict(state_offsets=(1, 6))),
    ("decreasing arc_offsets", dict(arc_offsets=(2, 0))),
    ("arc_offsets[0] != 0", dict(arc_offsets=(0, 1))),
    ("start beyond the item", dict(start=(0, 2))),
    ("start beyond the second item", dict(start=(1, 3))),
    ("nextstate beyond the item", dict(nextstates=(0, 2))),
    ("nextstate of another item's range", dict(nextstates=(3, 3))),
])
def test_malformed_lhs_batches(what, change):
    assert_invalid(*call_lhs(small_rhs(), mutated(**change)))


def test_decreasing_chain_offsets():
    rhs = small_rhs()
    assert_invalid(*call_chain(rhs, [1, 1, 1], [0, 2, 1, 3]))
    assert_invalid(*call_chain(rhs, [1, 1, 1], [3, 0]))


def test_unknown_flags_and_bad_rhs():
    rhs = small_rhs()
    lhs = F.LhsBatch.from_fsts(two_items())
    lab, off = [1, 1], [0, 1, 2]
    for lf in (2, 0x80000000, 3):                       # unknown bits in lattice_flags
        assert_invalid(*call_lhs(rhs, lhs, lattice_flags=lf))
        assert_invalid(*call_chain(rhs, lab, off, lattice_flags=lf))
    for fl in (2, 0x80000001):                          # unknown bits in opts->flags
        assert_invalid(*call_lhs(rhs, lhs, flags=fl))
        assert_invalid(*call_chain(rhs, lab, off, flags=fl))
    bad = Handle(F.FST_INVALID_HANDLE)
    assert_invalid(*call_lhs(bad, lhs))
    assert_invalid(*call_chain(bad, lab, off))
    assert_invalid(*call_chain(bad, [], [0]))           # checked before the empty result too
    dead = small_rhs()
    h, dead.h = dead.h, F.FST_INVALID_HANDLE
    F.lib().fst_free(h)
    assert_invalid(*call_lhs(Handle(h), lhs))
    assert_invalid(*call_chain(Handle(h), lab, off))


def test_empty_batch_is_an_ok_result():
    rhs = small_rhs()
    for lf in (0, FF.FST_LATTICE_PROJECT_OUTPUT):
        for rc, res in (call_lhs(rhs, F.LhsBatch.from_fsts([]), lattice_flags=lf),
                        call_chain(rhs, [], [0], lattice_flags=lf),
                        call_chain(rhs, None, [7], lattice_flags=lf)):
            assert rc == FF.FST_OK
            assert res.fsts.num_fsts == 0 and res.total_states == 0 and res.total_arcs == 0
            so = C.cast(res.fsts.state_offsets, C.POINTER(C.c_uint64))
            ao = C.cast(res.fsts.arc_offsets, C.POINTER(C.c_uint64))
            assert so[0] == 0 and ao[0] == 0
            F.lib().fst_lattice_batch_free(C.byref(res))
            assert bytes(res) == bytes(C.sizeof(res))   # freed: zeroed, a second free is a no-op
            F.lib().fst_lattice_batch_free(C.byref(res))
    got = F.compose_frozen_lhs_batch(rhs, F.LhsBatch.from_fsts([]))
    assert len(got) == 0 and got.state_offsets.tolist() == [0] and got.arc_offsets.tolist() == [0]
    got = F.compose_frozen_batch(rhs, [], [0], project_output=True)
    assert len(got) == 0 and got.state_offsets.tolist() == [0] and got.arc_offsets.tolist() == [0]
    assert len(got.as_lhs()) == 0


def test_device_entry_argument_checks():
    """What the host can check of the device form: nulls, flags, the handle (all before any
    device work, so no GPU is needed)."""
    rhs = small_rhs()
    L = F.lib()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    needed = (C.c_uint64 * 2)(7, 7)
    one = 8  # a non-null address the checks never dereference
    full = FF.FstDeviceLattices(one, one, one, one, one, one, one, one, one, 4, 4)

    def dev(h=rhs.h, offsets=one, lf=0, o=full, need=needed, fl=0):
        op = FF.FstBatchOptions(-1, 0, fl, 0, 0)
        return L.fst_device_compose_frozen(h, one, offsets, 1, 4, lf, C.byref(op),
                                           C.byref(o) if o is not None else None, need, None)

    assert dev(o=None) == FF.FST_INVALID_ARG
    assert dev(need=None) == FF.FST_INVALID_ARG
    assert dev(offsets=None) == FF.FST_INVALID_ARG
    assert dev(lf=2) == FF.FST_INVALID_ARG
    assert dev(fl=2) == FF.FST_INVALID_ARG
    assert dev(h=F.FST_INVALID_HANDLE) == FF.FST_INVALID_ARG
    for field in ("status", "state_offsets", "start", "final_weights", "arc_offsets", "ilabels",
                  "olabels", "weights", "nextstates"):
        o = FF.FstDeviceLattices(one, one, one, one, one, one, one, one, one, 4, 4)
        setattr(o, field, None)
        assert dev(o=o) == FF.FST_INVALID_ARG, field
    del opts
