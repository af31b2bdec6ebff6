"""connect on the host side: the model of tests/connect_model.py against the reference's known
answers (src/ops/connect.zig:128-181) and the edge cases of its definition, then
fst_connect_lhs_batch and FST_LATTICE_CONNECT as far as no GPU is needed: symbols, the Python
mirror, every argument check (they run before any device work)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import connect_model as CM
import libfst_amd as F
import libfst_amd.fst as FF
from test_lattice_batch_api import assert_invalid, call_chain, call_lhs, poisoned
from test_lhs_batch_api import mutated, small_rhs, two_items

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
NO_STATE = F.FST_NO_STATE


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


# ---- the model: the reference's three known answers ----------------------------------------

def dead_end_fst():
    """connect.zig:133-142: 0 -1-> 1 -2-> 2 (final), 0 -3-> 3 (a dead end)."""
    return 0, [INF, INF, 0.0, INF], [[(1, 1, 0.0, 1), (3, 3, 0.0, 3)], [(2, 2, 0.0, 2)], [], []]


def test_model_removes_the_dead_end():
    t = CM.connect_lists(*dead_end_fst())
    assert len(t.finals) == 3 and t.start == 0 and (t.states_in, t.arcs_in) == (4, 3)
    assert CM.to_lists(t) == (0, bits([INF, INF, 0.0]),
                              [[(1, 1, bits([0.0])[0], 1)], [(2, 2, bits([0.0])[0], 2)], []])


def test_model_keeps_a_connected_fst():
    fst = (0, [INF, 0.0], [[(1, 1, 0.0, 1)], []])
    t = CM.connect_lists(*fst)
    assert len(t.finals) == 2 and t.start == 0
    assert CM.to_lists(t) == (0, bits(fst[1]), [[(1, 1, bits([0.0])[0], 1)], []])


def test_model_empty_in_empty_out():
    for fst in ((None, [], []), (NO_STATE, [], []), (None, [0.0], [[]])):
        t = CM.connect_lists(*fst)
        assert t.start == NO_STATE and len(t.finals) == 0 and t.off.tolist() == [0]


# ---- the model: the edge cases of the definition ---------------------------------------------

def test_model_minus_inf_is_not_final_and_comes_out_plus_inf():
    # 0 -> 1 (final 0.5); state 0's own final weight is -inf: kept, but not final
    t = CM.connect_lists(0, [-INF, 0.5], [[(1, 1, 0.0, 1)], []])
    assert bits(t.finals) == bits([INF, 0.5])
    # alone, a -inf final makes nothing final: empty
    assert CM.connect_lists(0, [-INF], [[]]).start == NO_STATE


def test_model_nan_final_is_final():
    t = CM.connect_lists(0, [INF, NAN], [[(1, 2, NAN, 1)], []])
    assert len(t.finals) == 2 and bits(t.finals) == bits([INF, NAN])
    assert bits(t.w) == bits([NAN])                 # weights are copied, never compared


def test_model_start_not_coaccessible_is_empty():
    # the final state 2 is not reachable from 0, and 0 reaches no final state
    t = CM.connect_lists(0, [INF, INF, 0.0], [[(1, 1, 0.0, 1)], [], [(1, 1, 0.0, 2)]])
    assert t.start == NO_STATE and len(t.finals) == 0 and len(t.next) == 0


def test_model_unreachable_final_component_is_dropped():
    # 1 -> 2 (final) is a component of its own; the start is 3 -> 0 (final)
    t = CM.connect_lists(3, [0.25, INF, 0.0, INF],
                         [[], [(7, 7, 1.0, 2)], [], [(5, 6, -0.0, 0)]])
    # kept: 0 and 3, renumbered 0 and 1 in increasing old id; the start is the new 1
    assert t.start == 1 and bits(t.finals) == bits([0.25, INF])
    assert CM.to_lists(t)[2] == [[], [(5, 6, bits([-0.0])[0], 0)]]


def test_model_self_loop_on_a_dead_state_is_dropped():
    t = CM.connect_lists(0, [INF, INF, 1.0],
                         [[(1, 1, 0.0, 1), (2, 2, 0.0, 2)], [(9, 9, 0.0, 1)], [(3, 3, 0.5, 2)]])
    assert len(t.finals) == 2 and t.next.tolist() == [1, 1]      # 0 -> 2', and 2's own loop
    assert t.il.tolist() == [2, 3]


# ---- the entry: symbols, the mirror, the argument checks -------------------------------------

def call_connect(lhs, flags=0):
    opts = FF.FstBatchOptions(-1, 0, flags, 0, 0)
    res = poisoned()
    cs = lhs.c_struct() if lhs is not None else None
    rc = F.lib().fst_connect_lhs_batch(C.byref(cs) if cs is not None else None, C.byref(opts),
                                       C.byref(res))
    return rc, res


def test_symbol_header_and_mirror_parity():
    assert hasattr(F.lib(), "fst_connect_lhs_batch")
    assert "fst_connect_lhs_batch" in FF.SIGNATURES
    with open(os.path.join(REPO, "include", "fst_batch.h")) as fh:
        header = fh.read()
    assert re.search(r"FstError fst_connect_lhs_batch\(const FstLhsBatch\* lhs, "
                     r"const FstBatchOptions\* opts,\s+FstLatticeBatch\* out\);", header)
    m = re.search(r"#define FST_LATTICE_CONNECT (\d+)u", header)
    assert m and int(m.group(1)) == 4 == FF.FST_LATTICE_CONNECT == F.FST_LATTICE_CONNECT
    res, args = FF.SIGNATURES["fst_connect_lhs_batch"]
    assert res is C.c_int and len(args) == 3
    assert callable(F.connect_lhs_batch)
    import inspect
    for fn in (F.compose_frozen_batch, F.compose_frozen_lhs_batch):
        assert inspect.signature(fn).parameters["connect"].default is False


def test_connect_null_pointers():
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    assert F.lib().fst_connect_lhs_batch(C.byref(cs), C.byref(opts), None) == FF.FST_INVALID_ARG
    assert_invalid(*call_connect(None))
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        res = poisoned()
        rc = F.lib().fst_connect_lhs_batch(C.byref(cs), C.byref(opts), C.byref(res))
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
def test_connect_malformed_batches(what, change):
    assert_invalid(*call_connect(mutated(**change)))


def test_connect_unknown_option_flags():
    lhs = F.LhsBatch.from_fsts(two_items())
    for fl in (2, 0x80000001):
        assert_invalid(*call_connect(lhs, flags=fl))


def test_connect_empty_batch_is_an_ok_result():
    rc, res = call_connect(F.LhsBatch.from_fsts([]))
    assert rc == FF.FST_OK
    assert res.fsts.num_fsts == 0 and res.total_states == 0 and res.total_arcs == 0
    so = C.cast(res.fsts.state_offsets, C.POINTER(C.c_uint64))
    ao = C.cast(res.fsts.arc_offsets, C.POINTER(C.c_uint64))
    assert so[0] == 0 and ao[0] == 0
    F.lib().fst_lattice_batch_free(C.byref(res))
    assert bytes(res) == bytes(C.sizeof(res))
    got = F.connect_lhs_batch(F.LhsBatch.from_fsts([]))
    assert len(got) == 0 and got.state_offsets.tolist() == [0] and got.arc_offsets.tolist() == [0]


def test_lattice_flag_4_is_known_and_bit_1_is_not():
    """Zero items, so the calls end at the argument check or at the empty result."""
    rhs = small_rhs()
    none = F.LhsBatch.from_fsts([])
    for lf in (4, 5):
        for rc, res in (call_lhs(rhs, none, lattice_flags=lf),
                        call_chain(rhs, [], [0], lattice_flags=lf)):
            assert rc == FF.FST_OK and res.fsts.num_fsts == 0
            F.lib().fst_lattice_batch_free(C.byref(res))
    for lf in (2, 3, 6, 8):
        assert_invalid(*call_lhs(rhs, none, lattice_flags=lf))
        assert_invalid(*call_chain(rhs, [], [0], lattice_flags=lf))
    got = F.compose_frozen_batch(rhs, [], [0], project_output=True, connect=True)
    assert len(got) == 0 and got.state_offsets.tolist() == [0]
    got = F.compose_frozen_lhs_batch(rhs, none, connect=True)
    assert len(got) == 0 and got.arc_offsets.tolist() == [0]


def test_device_entry_flag_check():
    rhs = small_rhs()
    one = 8  # a non-null address the checks never dereference
    full = FF.FstDeviceLattices(one, one, one, one, one, one, one, one, one, 4, 4)
    needed = (C.c_uint64 * 2)(7, 7)
    op = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    for lf in (2, 3, 6, 8):
        assert F.lib().fst_device_compose_frozen(rhs.h, one, one, 1, 4, lf, C.byref(op),
                                                 C.byref(full), needed, None) == FF.FST_INVALID_ARG
