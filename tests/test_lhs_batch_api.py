"""The lhs batch entries (fst_compose_frozen_shortest_path_lhs_batch and its handles form):
symbols, struct layout and every host-side argument check.  No GPU: the checks run before
any device work."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import libfst_amd as F
import libfst_amd.fst as FF
from libfst_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


def small_rhs() -> F.Fst:
    m = F.MutableFst()
    s = m.add_state()
    m.set_start(s)
    m.set_final(s, 0.0)
    m.add_arc(s, 1, 2, 0.5, s)
    return m.freeze()


def two_items():
    """Two valid lhs: a 2-state acceptor of label 1 and a 3-state fork."""
    return [(0, [INF, 0.0], [[(1, 1, 0.25, 1)], []]),
            (0, [INF, 0.0, 1.0], [[(1, 1, 0.0, 1), (1, 0, 0.5, 2)], [], [(0, 1, 0.0, 1)]])]


def call(rhs, lhs: F.LhsBatch, n=1, flags=0, semantics=F.FST_SEM_LAZY):
    opts = FF.FstBatchOptions(-1, semantics, flags, 0, 0)
    res = FF.FstBatchResult()
    # poison: an error return must leave the struct zeroed
    res.num_strings = 77
    res.total_arcs = 99
    cs = lhs.c_struct()
    rc = F.lib().fst_compose_frozen_shortest_path_lhs_batch(rhs.h, C.byref(cs), n, C.byref(opts),
                                                            C.byref(res))
    return rc, res


def assert_invalid(rc, res):
    assert rc == FF.FST_INVALID_ARG
    assert bytes(res) == bytes(C.sizeof(res))


def test_symbols_and_struct_layout():
    L = F.lib()
    for name in ("fst_compose_frozen_shortest_path_lhs_batch",
                 "fst_compose_frozen_shortest_path_handles_batch"):
        assert hasattr(L, name)
        assert name in FF.SIGNATURES
    with open(os.path.join(REPO, "include", "fst_batch.h")) as fh:
        header = fh.read()
    body = re.search(r"typedef struct \{([^}]*)\} FstLhsBatch;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"[\s*]+", " ", d).strip().split(" ")[-1] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in FF.FstLhsBatch._fields_]
    assert fields == ["num_fsts", "state_offsets", "start", "final_weights", "arc_offsets",
                      "ilabels", "olabels", "weights", "nextstates"]
    assert C.sizeof(FF.FstLhsBatch) == 72          # u32 + pad, then eight pointers
    assert FF.FstLhsBatch.state_offsets.offset == 8


def test_from_fsts_builds_the_concatenated_csr():
    lhs = F.LhsBatch.from_fsts(two_items())
    assert len(lhs) == 2
    assert lhs.state_offsets.tolist() == [0, 2, 5]
    assert lhs.arc_offsets.tolist() == [0, 1, 1, 3, 3, 4]
    assert lhs.start.tolist() == [0, 0]
    assert lhs.nextstates.tolist() == [1, 1, 2, 1]     # local to each lhs
    same = F.LhsBatch.from_arrays(lhs.state_offsets, lhs.start, lhs.final_weights,
                                  lhs.arc_offsets, lhs.ilabels, lhs.olabels, lhs.weights,
                                  lhs.nextstates)
    assert same.olabels.tolist() == [1, 1, 0, 1]
    none = F.LhsBatch.from_fsts([(None, [0.0], [[]])])
    assert none.start.tolist() == [F.FST_NO_STATE]


def test_null_pointers():
    rhs = small_rhs()
    L = F.lib()
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    res = FF.FstBatchResult()
    lhs = F.LhsBatch.from_fsts(two_items())
    cs = lhs.c_struct()
    assert L.fst_compose_frozen_shortest_path_lhs_batch(rhs.h, C.byref(cs), 1, C.byref(opts),
                                                        None) == FF.FST_INVALID_ARG
    res.num_strings = 5
    assert L.fst_compose_frozen_shortest_path_lhs_batch(rhs.h, None, 1, C.byref(opts),
                                                        C.byref(res)) == FF.FST_INVALID_ARG
    assert bytes(res) == bytes(C.sizeof(res))
    for field in ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
                  "weights", "nextstates"):
        cs = lhs.c_struct()
        setattr(cs, field, None)
        res = FF.FstBatchResult()
        res.num_strings = 5
        rc = L.fst_compose_frozen_shortest_path_lhs_batch(rhs.h, C.byref(cs), 1, C.byref(opts),
                                                          C.byref(res))
        assert_invalid(rc, res)


def mutated(**kw) -> F.LhsBatch:
    lhs = F.LhsBatch.from_fsts(two_items())
    for k, (idx, val) in kw.items():
        getattr(lhs, k)[idx] = val
    return lhs


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
    assert_invalid(*call(small_rhs(), mutated(**change)))


def test_item_size_limits():
    rhs = small_rhs()
    # 2^30 states in one item: the state offsets alone say so, and that check comes before
    # anything reads the per-state arrays (which are therefore not 2^30 long here)
    lhs = F.LhsBatch([0, 1 << 30], [0], [0.0], [0, 0], [], [], [], [])
    assert_invalid(*call(rhs, lhs))
    lhs = F.LhsBatch([0, 2, 2 + (1 << 30)], [0, 0], [0.0, 0.0], [0, 0, 0], [], [], [], [])
    assert_invalid(*call(rhs, lhs))
    # 2^32 arcs on one state (the check comes before the arcs are read)
    lhs = F.LhsBatch([0, 1], [0], [0.0], [0, 1 << 32], [1], [1], [0.0], [0])
    assert_invalid(*call(rhs, lhs))


class Handle:
    def __init__(self, h):
        self.h = h


def test_unknown_flags_and_bad_rhs():
    rhs = small_rhs()
    lhs = F.LhsBatch.from_fsts(two_items())
    assert_invalid(*call(rhs, lhs, flags=2))
    assert_invalid(*call(rhs, lhs, flags=0x80000001))
    assert_invalid(*call(Handle(F.FST_INVALID_HANDLE), lhs))
    dead = small_rhs()
    h, dead.h = dead.h, F.FST_INVALID_HANDLE
    F.lib().fst_free(h)
    assert_invalid(*call(Handle(h), lhs))


def test_empty_batch_is_an_ok_result():
    rhs = small_rhs()
    lhs = F.LhsBatch.from_fsts([])
    for sem in (F.FST_SEM_LAZY, F.FST_SEM_EAGER):
        rc, res = call(rhs, lhs, semantics=sem)
        assert rc == FF.FST_OK
        assert res.num_strings == 0 and res.total_arcs == 0
        assert res.path_offsets[0] == 0
        F.lib().fst_batch_result_free(C.byref(res))
    got = F.compose_frozen_shortest_path_lhs_batch(rhs, lhs)
    assert len(got.status) == 0 and got.offsets.tolist() == [0]
    got = F.compose_frozen_shortest_path_handles_batch(rhs, [])
    assert len(got.status) == 0 and got.offsets.tolist() == [0]


def test_handles_entry_with_one_invalid_handle():
    rhs = small_rhs()
    good = F.MutableFst.compile_string(b"ab")
    hs = (C.c_uint64 * 3)(good.h, F.FST_INVALID_HANDLE, good.h)
    opts = FF.FstBatchOptions(-1, 0, 0, 0, 0)
    res = FF.FstBatchResult()
    res.num_strings = 9
    rc = F.lib().fst_compose_frozen_shortest_path_handles_batch(rhs.h, hs, 3, 1, C.byref(opts),
                                                                C.byref(res))
    assert_invalid(rc, res)
    rc = F.lib().fst_compose_frozen_shortest_path_handles_batch(rhs.h, None, 3, 1, C.byref(opts),
                                                                C.byref(res))
    assert_invalid(rc, res)
    with pytest.raises(RuntimeError):
        F.compose_frozen_shortest_path_handles_batch(rhs, [good, Handle(F.FST_INVALID_HANDLE)])


def test_generators_give_valid_items():
    rng = np.random.default_rng(5)
    texts = synthetic.utterances(rng, 6, 1, 12)
    items = [synthetic.confusion_network(rng, t, 4, 0.3) for t in texts]
    items.append(synthetic.nbest_union(rng, ["abc", "abd", "ab", "xyz", "abc"]))
    for (start, finals, arcs), t in zip(items, texts):
        assert start == 0 and len(finals) == len(t) + 1 and finals[-1] == 0.0
        assert all(f == INF for f in finals[:-1])
        for k, al in enumerate(arcs[:-1]):
            assert 1 <= len(al) <= 5 and all(a[3] == k + 1 for a in al)
            assert al[0][0] == ord(t[k]) + 1 and al[0][1] == al[0][0]
            if len(al) == 1:
                assert al[0][2] == 0.0 and not math.copysign(1.0, al[0][2]) < 0   # One, not -0.0
            else:                                                          # -log p, non-dyadic
                assert all(a[2] > 0 and a[2] != round(a[2]) for a in al)
                assert abs(sum(math.exp(-a[2]) for a in al) - 1.0) < 1e-12
            assert all(a[0] == a[1] for a in al)
            assert sum(1 for a in al if a[0] == 0) <= 1                    # the skip arc
    start, finals, arcs = items[-1]
    assert sum(1 for f in finals if f != INF) == 4       # one final per distinct hypothesis
    assert len(finals) == 1 + 3 + 1 + 3                  # root, a-b-c, d, x-y-z
    lhs = F.LhsBatch.from_fsts(items)
    assert len(lhs) == len(items) and int(lhs.arc_offsets[-1]) == len(lhs.ilabels)
