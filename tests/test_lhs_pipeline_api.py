"""The lhs pipeline entries (fst_pipeline_lhs_batch, fst_normalize_lhs_batch) and the
device-resident lhs entry (fst_device_compose_shortest_path_lhs): symbols and every host-side
argument check.  No GPU: the checks run before any device work."""
import ctypes as C

import pytest

import libfst_amd as F
import libfst_amd.fst as FF
from test_lhs_batch_api import Handle, mutated, small_rhs, two_items

ENTRIES = ["pipeline", "normalize"]


def call(entry, stages, lhs, n=1, flags=0, semantics=F.FST_SEM_LAZY, num_stages=None,
         null_stages=False):
    """(rc, result struct) of one host entry; the struct is poisoned first: an error return
    must leave it zeroed."""
    hs = (C.c_uint64 * max(len(stages), 1))(*[s.h for s in stages])
    ns = len(stages) if num_stages is None else num_stages
    opts = FF.FstBatchOptions(-1, semantics, flags, 0, 0)
    cs = lhs.c_struct()
    if entry == "pipeline":
        res = FF.FstBatchResult()
        res.num_strings, res.total_arcs = 77, 99
        rc = F.lib().fst_pipeline_lhs_batch(None if null_stages else hs, ns, C.byref(cs), n,
                                            C.byref(opts), C.byref(res))
    else:
        res = FF.FstTextResult()
        res.num_strings, res.total_bytes = 77, 99
        rc = F.lib().fst_normalize_lhs_batch(None if null_stages else hs, ns, C.byref(cs),
                                             C.byref(opts), C.byref(res))
    return rc, res


def assert_invalid(rc, res):
    assert rc == FF.FST_INVALID_ARG
    assert bytes(res) == bytes(C.sizeof(res))


def test_symbols():
    L = F.lib()
    for name in ("fst_pipeline_lhs_batch", "fst_normalize_lhs_batch",
                 "fst_device_compose_shortest_path_lhs"):
        assert hasattr(L, name)
        assert name in FF.SIGNATURES
    assert callable(F.pipeline_lhs_batch) and callable(F.normalize_lhs_batch)


@pytest.mark.parametrize("entry", ENTRIES)
def test_stage_arguments(entry):
    rhs = small_rhs()
    lhs = F.LhsBatch.from_fsts(two_items())
    assert_invalid(*call(entry, [rhs], lhs, num_stages=0))
    assert_invalid(*call(entry, [rhs], lhs, null_stages=True))
    assert_invalid(*call(entry, [rhs, Handle(F.FST_INVALID_HANDLE)], lhs))
    dead = small_rhs()
    h, dead.h = dead.h, F.FST_INVALID_HANDLE
    F.lib().fst_free(h)
    assert_invalid(*call(entry, [rhs, Handle(h)], lhs))
    assert_invalid(*call(entry, [Handle(F.FST_INVALID_HANDLE), rhs], lhs))


@pytest.mark.parametrize("entry", ENTRIES)
def test_unknown_flags(entry):
    rhs = small_rhs()
    lhs = F.LhsBatch.from_fsts(two_items())
    assert_invalid(*call(entry, [rhs, rhs], lhs, flags=2))
    assert_invalid(*call(entry, [rhs, rhs], lhs, flags=0x80000001))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("what,change", [
    ("decreasing state_offsets", dict(state_offsets=(1, 6))),
    ("decreasing arc_offsets", dict(arc_offsets=(2, 0))),
    ("arc_offsets[0] != 0", dict(arc_offsets=(0, 1))),
    ("start beyond the item", dict(start=(0, 2))),
    ("start beyond the second item", dict(start=(1, 3))),
    ("nextstate equal to the state count", dict(nextstates=(0, 2))),
    ("nextstate of another item's range", dict(nextstates=(3, 3))),
])
def test_malformed_batches(entry, what, change):
    rhs = small_rhs()
    assert_invalid(*call(entry, [rhs, rhs], mutated(**change)))


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_lhs_pointers_and_size_limits(entry):
    rhs = small_rhs()
    lhs = F.LhsBatch.from_fsts(two_items())
    L = F.lib()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    hs = (C.c_uint64 * 1)(rhs.h)
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        if entry == "pipeline":
            res = FF.FstBatchResult()
            res.num_strings = 5
            rc = L.fst_pipeline_lhs_batch(hs, 1, C.byref(cs), 1, C.byref(opts), C.byref(res))
        else:
            res = FF.FstTextResult()
            res.num_strings = 5
            rc = L.fst_normalize_lhs_batch(hs, 1, C.byref(cs), C.byref(opts), C.byref(res))
        assert_invalid(rc, res)
    # a null lhs, a null out
    if entry == "pipeline":
        res = FF.FstBatchResult()
        res.num_strings = 5
        assert_invalid(L.fst_pipeline_lhs_batch(hs, 1, None, 1, C.byref(opts), C.byref(res)), res)
        cs = lhs.c_struct()
        assert L.fst_pipeline_lhs_batch(hs, 1, C.byref(cs), 1, C.byref(opts),
                                        None) == FF.FST_INVALID_ARG
    else:
        res = FF.FstTextResult()
        res.num_strings = 5
        assert_invalid(L.fst_normalize_lhs_batch(hs, 1, None, C.byref(opts), C.byref(res)), res)
        cs = lhs.c_struct()
        assert L.fst_normalize_lhs_batch(hs, 1, C.byref(cs), C.byref(opts),
                                         None) == FF.FST_INVALID_ARG
    # 2^30 states in one item, 2^32 arcs on one state: checked before the arrays are read
    assert_invalid(*call(entry, [rhs], F.LhsBatch([0, 1 << 30], [0], [0.0], [0, 0], [], [], [], [])))
    assert_invalid(*call(entry, [rhs],
                         F.LhsBatch([0, 1], [0], [0.0], [0, 1 << 32], [1], [1], [0.0], [0])))


def test_empty_batch_is_an_ok_result():
    rhs = small_rhs()
    lhs = F.LhsBatch.from_fsts([])
    for sem in (F.FST_SEM_LAZY, F.FST_SEM_EAGER):
        rc, res = call("pipeline", [rhs, rhs], lhs, semantics=sem)
        assert rc == FF.FST_OK
        assert res.num_strings == 0 and res.total_arcs == 0 and res.path_offsets[0] == 0
        F.lib().fst_batch_result_free(C.byref(res))
        rc, res = call("normalize", [rhs, rhs], lhs, semantics=sem)
        assert rc == FF.FST_OK
        assert res.num_strings == 0 and res.total_bytes == 0 and res.text_offsets[0] == 0
        F.lib().fst_text_result_free(C.byref(res))
    got = F.pipeline_lhs_batch([rhs, rhs], lhs)
    assert len(got.status) == 0 and got.offsets.tolist() == [0]
    txt = F.normalize_lhs_batch([rhs], lhs)
    assert len(txt.status) == 0 and txt.offsets.tolist() == [0] and txt.texts() == []
    # the stages are still checked for an empty batch
    assert_invalid(*call("pipeline", [rhs, Handle(F.FST_INVALID_HANDLE)], lhs))
    assert_invalid(*call("normalize", [rhs], lhs, num_stages=0))


def test_device_entry_null_arguments():
    rhs = small_rhs()
    L = F.lib()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()        # (host pointers: the call must return before it looks at them)
    out = FF.FstDeviceBatch()
    assert L.fst_device_compose_shortest_path_lhs(rhs.h, C.byref(cs), 1, C.byref(opts), None,
                                                  None) == FF.FST_INVALID_ARG
    assert L.fst_device_compose_shortest_path_lhs(rhs.h, None, 1, C.byref(opts), C.byref(out),
                                                  None) == FF.FST_INVALID_ARG
    # unknown flags, a null arc cursor, an invalid handle: refused on the host as well
    bad = FF.FstBatchOptions(-1, 0, 2, 0, 0)
    assert L.fst_device_compose_shortest_path_lhs(rhs.h, C.byref(cs), 1, C.byref(bad),
                                                  C.byref(out), None) == FF.FST_INVALID_ARG
    assert L.fst_device_compose_shortest_path_lhs(rhs.h, C.byref(cs), 1, C.byref(opts),
                                                  C.byref(out), None) == FF.FST_INVALID_ARG
    out.arc_cursor = 8
    empty = FF.FstLhsBatch()
    assert L.fst_device_compose_shortest_path_lhs(F.FST_INVALID_HANDLE, C.byref(empty), 1,
                                                  C.byref(opts), C.byref(out),
                                                  None) == FF.FST_INVALID_ARG
