"""fst_posterior_lhs_batch, fst_device_posterior_lhs and fst_batch_result_path_costs as far as no
GPU is needed: symbols, the header, the Python mirror, every argument check (they run before any
device work), the empty batch, and the host helper against a numpy fold bit for bit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import libfst_amd as F
import libfst_amd.fst as FF
from test_lattice_batch_api import assert_invalid, header_fields
from test_lhs_batch_api import mutated, two_items

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan


def poisoned():
    res = FF.FstPosteriorResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))   # an error return must leave the struct zeroed
    return res


def call(lhs, flags=0):
    opts = FF.FstBatchOptions(-1, 0, flags, 0, 0)
    res = poisoned()
    cs = lhs.c_struct() if lhs is not None else None
    rc = F.lib().fst_posterior_lhs_batch(C.byref(cs) if cs is not None else None, C.byref(opts),
                                         C.byref(res))
    return rc, res


def test_symbols_header_and_mirror_parity():
    for name in ("fst_posterior_lhs_batch", "fst_posterior_result_free",
                 "fst_device_posterior_lhs", "fst_batch_result_path_costs"):
        assert hasattr(F.lib(), name)
        assert name in FF.SIGNATURES
    with open(os.path.join(REPO, "include", "fst_batch.h")) as fh:
        header = fh.read()
    assert re.search(r"FstError fst_posterior_lhs_batch\(const FstLhsBatch\* lhs, "
                     r"const FstBatchOptions\* opts,\s+FstPosteriorResult\* out\);", header)
    assert re.search(r"FstError fst_device_posterior_lhs\(const FstLhsBatch\* d_lhs, "
                     r"const FstBatchOptions\* opts,\s+const FstDevicePosteriors\* out, "
                     r"void\* stream\);", header)
    assert re.search(r"FstError fst_batch_result_path_costs\(const FstBatchResult\* paths, "
                     r"uint32_t per,\s+const double\* total, uint32_t num_fsts, double\* out\);",
                     header)
    assert re.search(r"16 = fst_posterior_lhs_batch and fst_device_posterior_lhs", header)
    assert header_fields("FstPosteriorResult") == [f[0] for f in FF.FstPosteriorResult._fields_]
    assert header_fields("FstDevicePosteriors") == [f[0] for f in FF.FstDevicePosteriors._fields_]
    assert C.sizeof(FF.FstPosteriorResult) == 64 and C.sizeof(FF.FstDevicePosteriors) == 40
    assert callable(F.posterior_lhs_batch) and callable(F.batch_result_path_costs)


def test_null_pointers():
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    assert F.lib().fst_posterior_lhs_batch(C.byref(cs), C.byref(opts), None) == FF.FST_INVALID_ARG
    assert_invalid(*call(None))
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        res = poisoned()
        assert_invalid(F.lib().fst_posterior_lhs_batch(C.byref(cs), C.byref(opts), C.byref(res)),
                       res)


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
    assert_invalid(*call(mutated(**change)))
    with pytest.raises(RuntimeError, match="fst_posterior_lhs_batch failed"):
        F.posterior_lhs_batch(mutated(**change))


def test_unknown_option_flags():
    lhs = F.LhsBatch.from_fsts(two_items())
    for fl in (2, 0x80000001):
        assert_invalid(*call(lhs, flags=fl))


def test_empty_batch_is_an_ok_result():
    """Zero items end at the empty result before any device work."""
    rc, res = call(F.LhsBatch.from_fsts([]))
    assert rc == FF.FST_OK
    assert res.num_fsts == 0 and res.total_states == 0 and res.total_arcs == 0
    F.lib().fst_posterior_result_free(C.byref(res))
    assert bytes(res) == bytes(C.sizeof(res))
    F.lib().fst_posterior_result_free(C.byref(res))   # freeing a zeroed result is harmless
    F.lib().fst_posterior_result_free(None)
    got = F.posterior_lhs_batch(F.LhsBatch.from_fsts([]))
    assert len(got) == 0 and len(got.total) == 0 and len(got.alpha) == 0 and len(got.arc_cost) == 0


def test_device_entry_argument_checks():
    one = 8  # a non-null address the checks never dereference
    lhs = FF.FstLhsBatch(1, one, one, one, one, one, one, one, one)
    full = FF.FstDevicePosteriors(one, one, one, one, one)
    op = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    L = F.lib()
    assert L.fst_device_posterior_lhs(None, C.byref(op), C.byref(full), None) == FF.FST_INVALID_ARG
    assert L.fst_device_posterior_lhs(C.byref(lhs), C.byref(op), None, None) == FF.FST_INVALID_ARG
    bad = FF.FstBatchOptions(-1, 0, 2, 0, 0)
    assert L.fst_device_posterior_lhs(C.byref(lhs), C.byref(bad), C.byref(full),
                                      None) == FF.FST_INVALID_ARG
    for field in ("status", "total"):
        o = FF.FstDevicePosteriors(one, one, one, one, one)
        setattr(o, field, None)
        assert L.fst_device_posterior_lhs(C.byref(lhs), C.byref(op), C.byref(o),
                                          None) == FF.FST_INVALID_ARG
    nostart = FF.FstLhsBatch(1, one, None, one, one, one, one, one, one)
    assert L.fst_device_posterior_lhs(C.byref(nostart), C.byref(op), C.byref(full),
                                      None) == FF.FST_INVALID_ARG


# ---- fst_batch_result_path_costs -----------------------------------------------------------------

def paths():
    """Three items, two strings each; string 3 is EMPTY, string 4 UNSUPPORTED with stale arcs."""
    status = np.array([0, 0, 0, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED, 0], np.int32)
    offsets = np.array([0, 3, 3, 7, 7, 9, 10], np.uint64)
    rng = np.random.default_rng(5)
    weights = rng.normal(0.0, 3.0, 10) * 0.1 + 0.3
    weights[1] = -0.0
    finals = np.array([0.7, -1.3, 0.1, INF, 0.2, -0.0])
    return F.BatchResult(status, offsets, np.zeros(10, np.uint32), np.zeros(10, np.uint32),
                         weights, finals)


def test_path_costs_against_a_numpy_fold():
    r = paths()
    total = np.array([-0.4, 1.1, 0.3])
    got = F.batch_result_path_costs(r, 2, total)
    exp = np.full(6, INF)
    for s in range(6):
        if r.status[s] != F.FST_PATH_OK:
            continue
        c = np.float64(0.0)
        for a in range(int(r.offsets[s]), int(r.offsets[s + 1])):
            c = c + r.weights[a]
        exp[s] = (c + r.finals[s]) - total[s // 2]
    assert got.view(np.uint64).tolist() == exp.view(np.uint64).tolist()
    assert got[3] == INF and got[4] == INF and got[1] == -1.3 - -0.4
    # per = 6 over one item
    one = F.batch_result_path_costs(r, 6, np.array([0.0]))
    assert one[3] == INF and one[1] == -1.3


def test_path_costs_argument_checks():
    r = paths()
    total = np.zeros(3)
    out = np.zeros(6)
    cast = lambda a, ct: C.cast(a.ctypes.data, C.POINTER(ct))
    src = FF.FstBatchResult(6, cast(r.status, C.c_int32), cast(r.offsets, C.c_uint64),
                            cast(r.ilabels, C.c_uint32), cast(r.olabels, C.c_uint32),
                            cast(r.weights, C.c_double), cast(r.finals, C.c_double), 10)
    L = F.lib()
    t, o = total.ctypes.data, out.ctypes.data
    assert L.fst_batch_result_path_costs(C.byref(src), 2, t, 3, o) == FF.FST_OK
    assert L.fst_batch_result_path_costs(None, 2, t, 3, o) == FF.FST_INVALID_ARG
    assert L.fst_batch_result_path_costs(C.byref(src), 2, None, 3, o) == FF.FST_INVALID_ARG
    assert L.fst_batch_result_path_costs(C.byref(src), 2, t, 3, None) == FF.FST_INVALID_ARG
    assert L.fst_batch_result_path_costs(C.byref(src), 0, t, 3, o) == FF.FST_INVALID_ARG
    assert L.fst_batch_result_path_costs(C.byref(src), 2, t, 2, o) == FF.FST_INVALID_ARG
    assert L.fst_batch_result_path_costs(C.byref(src), 3, t, 3, o) == FF.FST_INVALID_ARG
    with pytest.raises(RuntimeError, match="fst_batch_result_path_costs failed"):
        F.batch_result_path_costs(r, 4, total)
