"""fst_nbest_unique_lhs_batch and fst_device_nbest_unique_lhs as far as no GPU is needed: symbols,
the header, the Python mirror and every argument check of the plain entries (test_nbest_api.py)
on the new ones; they run before any device work."""
import ctypes as C
import inspect
import os
import re

import pytest

import libfst_amd as F
import libfst_amd.fst as FF
from libfst_amd import synthetic as SY
from test_lhs_batch_api import assert_invalid, mutated, two_items
from test_shortest_path_batch_api import poisoned

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def call_unique(lhs, n=2, flags=0):
    opts = FF.FstBatchOptions(-1, 0, flags, 0, 0)
    res = poisoned()
    cs = lhs.c_struct() if lhs is not None else None
    rc = F.lib().fst_nbest_unique_lhs_batch(C.byref(cs) if cs is not None else None, n,
                                            C.byref(opts), C.byref(res))
    return rc, res


def test_symbols_header_and_mirror_parity():
    for name in ("fst_nbest_unique_lhs_batch", "fst_device_nbest_unique_lhs"):
        assert hasattr(F.lib(), name)
        assert name in FF.SIGNATURES
    with open(os.path.join(REPO, "include", "fst_batch.h")) as fh:
        header = fh.read()
    assert re.search(r"FstError fst_nbest_unique_lhs_batch\(const FstLhsBatch\* lhs, uint32_t n,\s+"
                     r"const FstBatchOptions\* opts,\s+FstBatchResult\* out\);", header)
    assert re.search(r"FstError fst_device_nbest_unique_lhs\(const FstLhsBatch\* d_lhs, "
                     r"uint32_t n,\s+const FstBatchOptions\* opts,\s+"
                     r"const FstDeviceBatch\* out,\s+void\* stream\);", header)
    assert re.search(r"14 = fst_nbest_unique_lhs_batch", header)       # FstLaunchStats.engine
    # the contract is in the header: the definition and why the lists lose nothing
    for phrase in ("sequence of its non-epsilon olabels", "does not depend on n",
                   "Drop every path whose output text equals that of an earlier path",
                   "pairwise different output texts", "only the least in (g, a, r) order is",
                   "whose text was already chosen is passed over"):
        assert phrase in header, phrase
    assert FF.SIGNATURES["fst_nbest_unique_lhs_batch"] == FF.SIGNATURES["fst_nbest_lhs_batch"]
    assert FF.SIGNATURES["fst_device_nbest_unique_lhs"] == FF.SIGNATURES["fst_device_nbest_lhs"]
    # the mirror: nbest_lhs_batch keeps its parameters, its sibling has the same ones
    assert F.nbest_unique_lhs_batch is FF.nbest_unique_lhs_batch
    assert inspect.signature(F.nbest_unique_lhs_batch).parameters.keys() == \
        inspect.signature(F.nbest_lhs_batch).parameters.keys()


def test_null_pointers():
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    fn = F.lib().fst_nbest_unique_lhs_batch
    assert fn(C.byref(cs), 2, C.byref(opts), None) == FF.FST_INVALID_ARG
    assert_invalid(*call_unique(None))
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        res = poisoned()
        assert_invalid(fn(C.byref(cs), 2, C.byref(opts), C.byref(res)), res)


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
    for n in (1, 2, 16):
        assert_invalid(*call_unique(mutated(**change), n=n))


def test_item_size_limits():
    lhs = F.LhsBatch([0, 1 << 30], [0], [0.0], [0, 0], [], [], [], [])
    assert_invalid(*call_unique(lhs))
    lhs = F.LhsBatch([0, 1], [0], [0.0], [0, 1 << 32], [1], [1], [0.0], [0])
    assert_invalid(*call_unique(lhs))


def test_n_out_of_range():
    lhs = F.LhsBatch.from_fsts(two_items())
    for n in (0, 17, 0xFFFFFFFF):
        assert_invalid(*call_unique(lhs, n=n))
    for n in (0, 17):                        # the empty batch too
        assert_invalid(*call_unique(F.LhsBatch.from_fsts([]), n=n))
    with pytest.raises(RuntimeError):
        F.nbest_unique_lhs_batch(lhs, 0)


def test_slot_count_overflow():
    """num_fsts * n >= 2^32 is refused before lhs's arrays are read."""
    lhs = F.LhsBatch.from_fsts(two_items())
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    for num, n in ((1 << 28, 16), (1 << 31, 2), (0xFFFFFFFF, 2), ((1 << 32) // 3 + 1, 3)):
        cs = lhs.c_struct()
        cs.num_fsts = num
        res = poisoned()
        rc = F.lib().fst_nbest_unique_lhs_batch(C.byref(cs), n, C.byref(opts), C.byref(res))
        assert_invalid(rc, res)


def test_unknown_option_flags():
    lhs = F.LhsBatch.from_fsts(two_items())
    for fl in (2, 0x80000001):
        assert_invalid(*call_unique(lhs, flags=fl))


def test_empty_batch_is_an_ok_result():
    for n in (1, 2, 16):
        rc, res = call_unique(F.LhsBatch.from_fsts([]), n=n)
        assert rc == FF.FST_OK
        assert res.num_strings == 0 and res.total_arcs == 0
        assert res.path_offsets[0] == 0
        F.lib().fst_batch_result_free(C.byref(res))
        assert bytes(res) == bytes(C.sizeof(res))
    got = F.nbest_unique_lhs_batch(F.LhsBatch.from_fsts([]), 4)
    assert len(got.status) == 0 and got.offsets.tolist() == [0]


def test_device_entry_argument_checks():
    one = 8  # a non-null address the checks never dereference
    lhs = FF.FstLhsBatch(1, one, one, one, one, one, one, one, one)
    out = FF.FstDeviceBatch()
    full = FF.FstDeviceBatch(one, one, one, one, one, one, one, 0, one, None)
    op = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    fn = F.lib().fst_device_nbest_unique_lhs
    assert fn(None, 2, C.byref(op), C.byref(full), None) == FF.FST_INVALID_ARG
    assert fn(C.byref(lhs), 2, C.byref(op), None, None) == FF.FST_INVALID_ARG
    assert fn(C.byref(lhs), 2, C.byref(op), C.byref(out), None) == FF.FST_INVALID_ARG  # null arrays
    bad = FF.FstBatchOptions(-1, 0, 2, 0, 0)
    assert fn(C.byref(lhs), 2, C.byref(bad), C.byref(full), None) == FF.FST_INVALID_ARG
    for n in (0, 17):
        assert fn(C.byref(lhs), n, C.byref(op), C.byref(full), None) == FF.FST_INVALID_ARG
    big = FF.FstLhsBatch(1 << 28, one, one, one, one, one, one, one, one)
    assert fn(C.byref(big), 16, C.byref(op), C.byref(full), None) == FF.FST_INVALID_ARG
    for field in ("state_offsets", "start", "arc_offsets"):
        cs = FF.FstLhsBatch(1, one, one, one, one, one, one, one, one)
        setattr(cs, field, None)
        assert fn(C.byref(cs), 2, C.byref(op), C.byref(full), None) == FF.FST_INVALID_ARG


def test_respelled_union():
    """The generator of repeat-rich items: a prefix tree of up to k spellings of one text."""
    import numpy as np
    rng = np.random.default_rng(1)
    start, finals, arcs = SY.respelled_union(rng, "ab 42 c7", 6)
    hyps = []

    def walk(s, text):
        if finals[s] != SY.INF:
            hyps.append(text)
        for il, ol, _, nx in arcs[s]:
            assert il == ol
            walk(nx, text + chr(il - 1))

    walk(start, "")
    assert "ab 42 c7" in hyps and 2 <= len(hyps) <= 6 and len(set(hyps)) == len(hyps)
    digits = {w: str(d) for d, w in enumerate(SY.WORDS)}
    for h in hyps:
        for w, d in digits.items():
            h = h.replace(w, d)
        assert h == "ab 42 c7"
    # no digit: one hypothesis
    assert sum(f != SY.INF for f in SY.respelled_union(rng, "abc", 4)[1]) == 1
