"""GPU: the lattice batch entries (fst_compose_frozen_batch, fst_compose_frozen_lhs_batch,
fst_device_compose_frozen) against the CPU oracle, item by item, bit for bit.

The expected value of every item is O.compose_csr(lhs, blob): start, state count, final-weight
bit patterns, and per state the (ilabel, olabel, weight bits, nextstate) list (compared as
arrays: the per-state arc ranges and the four arc arrays).  Every item of every batch is
compared.  The tests sit on what the batch adds to the single call's kernel: the emission into
the shared arena, the compaction into item order, the tier hand-over, arena growth, shards.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import libfst_amd as F
import libfst_amd.fst as FF
import oracle_ffi as O
from libfst_amd import synthetic as SY
from test_gpu_lhs_batch import (assert_shards_do_not_show, batch_of, bits, expect, got_item,
                                tagger_rhs)
from test_gpu_lhs_device import DeviceOut
from test_gpu_parity import load_blob, random_rhs, to_product

pytestmark = pytest.mark.gpu

EAGER, LAZY = F.FST_SEM_EAGER, F.FST_SEM_LAZY
INF = math.inf
OK, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_UNSUPPORTED
NO_STATE = F.FST_NO_STATE
ARRAYS = ("status", "state_offsets", "start", "final_weights", "arc_offsets", "ilabels",
          "olabels", "weights", "nextstates")


def chain_fst(labels) -> O.Fst:
    """The fst_compile_string-style chain of a label sequence (src/string.zig:24-50)."""
    L = len(labels)
    f = O.Fst(start=0, finals=[INF] * L + [0.0], arcs=[[] for _ in range(L + 1)])
    for k, l in enumerate(labels):
        f.arcs[k] = [(int(l), int(l), 0.0, k + 1)]
    return f


def csr_of(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        np.cumsum([len(s) for s in seqs], out=off[1:])
    lab = np.array([l for s in seqs for l in s], np.uint32)
    return lab, off


def oracle(lhs: O.Fst, blob: bytes) -> O.Csr:
    rc, c = O.compose_csr(lhs, blob)
    assert rc == O.OR_OK
    return c


def assert_item(got: F.LatticeBatch, i, c: O.Csr, project=False):
    """Item i of the batch equals the oracle's lattice, bit for bit."""
    assert int(got.status[i]) == OK, (i, int(got.status[i]))
    s0, s1 = int(got.state_offsets[i]), int(got.state_offsets[i + 1])
    ns = len(c.finals)
    assert s1 - s0 == ns, (i, s1 - s0, ns)
    assert int(got.start[i]) == (c.start if ns else NO_STATE), i
    if ns:
        assert c.start == 0
    assert np.array_equal(bits(got.final_weights[s0:s1]), bits(c.finals)), i
    ao = got.arc_offsets[s0:s1 + 1]
    a0, a1 = int(ao[0]), int(ao[-1])
    assert np.array_equal(ao - ao[0], c.off), i          # per state its arc range
    assert a1 - a0 == len(c.arcs), i
    assert np.array_equal(got.ilabels[a0:a1], c.arcs["ol"] if project else c.arcs["il"]), i
    assert np.array_equal(got.olabels[a0:a1], c.arcs["ol"]), i
    assert np.array_equal(bits(got.weights[a0:a1]), bits(c.arcs["w"])), i
    assert np.array_equal(got.nextstates[a0:a1], c.arcs["next"]), i


def assert_layout(got: F.LatticeBatch):
    """The FstLhsBatch invariants: offsets start at 0, are monotone and close on the totals."""
    assert int(got.state_offsets[0]) == 0 and int(got.arc_offsets[0]) == 0
    assert np.all(np.diff(got.state_offsets.astype(np.int64)) >= 0)
    assert np.all(np.diff(got.arc_offsets.astype(np.int64)) >= 0)
    assert len(got.final_weights) == int(got.state_offsets[-1])
    assert len(got.arc_offsets) == len(got.final_weights) + 1
    assert len(got.ilabels) == int(got.arc_offsets[-1])


def check_lhs(rhs, blob, fsts, exp=None, project=False, **kw):
    got = F.compose_frozen_lhs_batch(rhs, batch_of(fsts), project_output=project, **kw)
    assert len(got) == len(fsts)
    assert_layout(got)
    exp = exp if exp is not None else [oracle(f, blob) for f in fsts]
    for i, c in enumerate(exp):
        assert_item(got, i, c, project)
    return got, exp


def check_chain(rhs, blob, seqs, exp=None, project=False, **kw):
    got = F.compose_frozen_batch(rhs, *csr_of(seqs), project_output=project, **kw)
    assert len(got) == len(seqs)
    assert_layout(got)
    exp = exp if exp is not None else [oracle(chain_fst(s), blob) for s in seqs]
    for i, c in enumerate(exp):
        assert_item(got, i, c, project)
    return got, exp


def same_bytes(a: F.LatticeBatch, b: F.LatticeBatch):
    for name in ARRAYS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


def route_cols(capfd):
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lattice batch:" in ln]
    assert lines, err
    m = re.search(r"lattice batch: items (\d+) \| tiny128 (\d+) tiny256 (\d+) tier0 (\d+) "
                  r"tier1\+ (\d+)", lines[-1])
    return int(m.group(1)), [int(m.group(k)) for k in range(2, 6)], lines


# ---- 1. known answers --------------------------------------------------------------------

def test_known_answers_through_both_entries():
    a1 = O.compile_string(b"123")                              # compose-shortest-path.zig:447-471
    a2 = O.compile_string_transducer(b"abcde", b"xy")          # epsilon outputs
    a3 = O.compile_string(b"xy")
    seqs = [[b + 1 for b in s] for s in (b"123", b"xy")]
    for rhs_fst in (O.compile_string_transducer(b"123", b"abc"),
                    O.compile_string_transducer(b"xy", b"uvw")):
        blob = O.freeze(rhs_fst)
        rhs = load_blob(blob)
        via_lhs, exp = check_lhs(rhs, blob, [a1, a2, a3])
        via_chain, _ = check_chain(rhs, blob, seqs, exp=[exp[0], exp[2]])
        assert via_lhs.item(0) == via_chain.item(0) and via_lhs.item(2) == via_chain.item(1)
        # ... and the single call, read back through the handle API
        for i, a in enumerate((a1, a2, a3)):
            single = F.compose_frozen(to_product(a), rhs)
            start, finals, arcs = single.to_lists()
            g_start, g_finals, g_arcs = via_lhs.item(i)
            assert g_start == (start if finals else NO_STATE)
            assert bits(g_finals).tolist() == bits(finals).tolist()
            key = lambda al: [(a, b, int(bits([w])[0]), d) for (a, b, w, d) in al]
            assert [key(al) for al in g_arcs] == [key(al) for al in arcs]
    # the known answer itself: "123" against 123 -> abc is the 4-state chain
    blob = O.freeze(O.compile_string_transducer(b"123", b"abc"))
    got, _ = check_chain(load_blob(blob), blob, [seqs[0]])
    assert F.last_launch_stats().engine == 10
    start, finals, arcs = got.item(0)
    assert start == 0 and len(finals) == 4 and finals[3] == 0.0
    assert [al[0][1] for al in arcs[:3]] == [b + 1 for b in b"abc"]


# ---- 2. degenerate items -------------------------------------------------------------------

def degenerate_items():
    no_states = O.Fst()
    no_start = O.Fst(finals=[0.0, INF], arcs=[[(1, 1, 0.0, 1)], []])
    lone_final = O.Fst(start=0, finals=[0.5], arcs=[[]])
    never_final = O.Fst(start=0, finals=[INF, INF], arcs=[[(1, 1, 0.0, 1)], [(1, 1, 1.0, 0)]])
    plain = O.Fst(start=0, finals=[INF, 0.25], arcs=[[(1, 2, 0.5, 1)], []])
    return [no_states, no_start, lone_final, never_final, plain]


@pytest.mark.parametrize("rhs_has_start", [True, False])
def test_degenerate_items(rhs_has_start):
    r = O.Fst(start=0, finals=[1.5, 0.0],
              arcs=[[(1, 1, 0.25, 1), (2, 3, 0.0, 1)], [(1, 1, 0.0, 1)]]) if rhs_has_start \
        else O.Fst()
    blob = O.freeze(r)
    rhs = load_blob(blob)
    fsts = degenerate_items()
    got, exp = check_lhs(rhs, blob, fsts)
    # the reference's empty FST: OK, zero states, no start
    for i in (0, 1):
        assert len(exp[i].finals) == 0 and int(got.start[i]) == NO_STATE
    if rhs_has_start:
        # (the cycle's two states meet rhs state 0 once and rhs state 1 twice: 3 tuples)
        assert [len(e.finals) for e in exp[2:]] == [1, 3, 2]
        assert got.item(2) == (0, [2.0], [[]])                # times(0.5, 1.5)
        assert all(f == INF for f in got.item(3)[1])          # the never-final cycle, untrimmed
    else:
        assert all(len(e.finals) == 0 for e in exp)
        assert got.start.tolist() == [NO_STATE] * len(fsts)
    # the chain entry: an empty string (the one-state final acceptor) among others
    got, exp = check_chain(rhs, blob, [[], [1], [], [1, 1, 2], [9]])
    if rhs_has_start:
        assert got.item(0) == (0, [1.5], [[]]) and got.item(2) == got.item(0)
        assert len(exp[4].finals) == 1 and got.item(4) == (0, [INF], [[]])


# ---- 3. random sweep -------------------------------------------------------------------------

def odd_weights(rng, f: O.Fst):
    """Negative, -0.0 and +inf weights on some arcs (compose never orders weights)."""
    odd = [-1.5, -0.0, INF, -0.25]
    for al in f.arcs:
        for k, a in enumerate(al):
            if rng.random() < 0.25:
                al[k] = a[:2] + (odd[int(rng.integers(len(odd)))],) + a[3:]
    for s in range(f.num_states):
        if rng.random() < 0.1:
            f.finals[s] = -0.0 if rng.random() < 0.5 else -2.0
    return f


@pytest.fixture(scope="module")
def sweep():
    cases = []
    for seed in range(6):
        rng = np.random.default_rng(8100 + seed)
        frac = seed % 2 == 1
        rhs_fst = random_rhs(rng, int(rng.integers(2, 20)), int(rng.integers(8, 80)), 3, eps=True,
                             frac=frac)
        blob = O.freeze(rhs_fst)
        fsts = [odd_weights(rng, random_rhs(rng, int(rng.integers(1, 11)),
                                            int(rng.integers(1, 31)), 3, eps=True, frac=frac))
                for _ in range(52)]
        seqs = [[int(x) for x in rng.integers(0, 4, int(rng.integers(0, 10)))] for _ in range(10)]
        # input epsilon in the rhs (filter 1: the rhs moves alone); the lhs's output epsilons
        # (filter 2) are counted below
        assert any(a[0] == 0 for al in rhs_fst.arcs for a in al)
        cases.append((blob, fsts, seqs, [oracle(f, blob) for f in fsts],
                      [oracle(chain_fst(s), blob) for s in seqs]))
    return cases


def test_random_sweep(sweep, monkeypatch):
    assert sum(len(c[1]) for c in sweep) >= 300 and len(sweep) >= 6
    f1 = f2 = eps_out = cyc = 0
    for blob, fsts, seqs, exp, exp_chain in sweep:
        rhs = load_blob(blob)
        monkeypatch.delenv("FSTAMD_GRAPH_GRID", raising=False)
        free, _ = check_lhs(rhs, blob, fsts, exp=exp)
        free_chain, _ = check_chain(rhs, blob, seqs, exp=exp_chain)
        monkeypatch.setenv("FSTAMD_GRAPH_GRID", "2")          # many items share a workgroup
        capped, _ = check_lhs(rhs, blob, fsts, exp=exp)
        assert F.last_launch_stats().grid <= 2
        capped_chain, _ = check_chain(rhs, blob, seqs, exp=exp_chain)
        # the order in the arena differs with the grid; the result does not
        same_bytes(free, capped)
        same_bytes(free_chain, capped_chain)
        # what the sweep is meant to hold: lattice arcs on which one side moved alone (an
        # epsilon on the lattice's input or output tape), output epsilons, cycles
        for f, c in zip(fsts, exp):
            eps_out += any(a[1] == 0 for al in f.arcs for a in al)
            cyc += any(a[3] <= s for s, al in enumerate(f.arcs) for a in al)
            f1 += bool(np.any(c.arcs["il"] == 0))
            f2 += bool(np.any(c.arcs["ol"] == 0))
    assert f1 > 20 and f2 > 20 and eps_out > 100 and cyc > 100


# ---- 4. tier boundaries ----------------------------------------------------------------------

def heap_tree(N, rng, B=8):
    """An N-state B-ary tree in heap order with 1:1 arcs: against loop_rhs() its lattice is
    the tree itself (N states, N - 1 arcs, BFS ids = heap ids, ~log_B N levels)."""
    f = O.Fst(start=0, finals=[INF] * N, arcs=[[] for _ in range(N)])
    w = rng.integers(0, 4, size=N)
    for i in range(1, N):
        f.arcs[(i - 1) // B].append((1, 1, float(w[i]), i))
    f.finals[N - 1] = 0.75
    return f


def loop_rhs():
    return O.Fst(start=0, finals=[0.125], arcs=[[(1, 1, 0.5, 0)]])


@pytest.fixture(scope="module")
def tier_case():
    rng = np.random.default_rng(5)
    blob = O.freeze(loop_rhs())
    sizes = (128, 129, 256, 257, 16384, 16385)
    fsts = [heap_tree(N, rng) for N in sizes]
    return blob, fsts, sizes, [oracle(f, blob) for f in fsts]


def test_tier_boundaries(tier_case, monkeypatch, capfd):
    blob, fsts, sizes, exp = tier_case
    # the oracle's own counts, on both sides of the two LDS sizes and of tier 0
    assert [len(c.finals) for c in exp] == [128, 129, 256, 257, 16384, 16385]
    assert [len(c.arcs) for c in exp] == [n - 1 for n in sizes]
    assert len(exp[0].arcs) <= 176 and len(exp[2].arcs) <= 384    # states decide, not arcs
    rhs = load_blob(blob)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    check_lhs(rhs, blob, fsts, exp=exp)
    items, cols, lines = route_cols(capfd)
    assert items == 6 and cols == [6, 5, 3, 1]
    st = F.last_launch_stats()
    assert st.engine == 10 and st.launches == 2 * 4
    # the chain instances: 126 labels are the LDS tiers' longest chain, 127 go to tier 0
    seqs = [[1] * 100, [1] * 126, [1] * 127, [1] * 300]
    got, exp_chain = check_chain(rhs, blob, seqs)
    assert [len(c.finals) for c in exp_chain] == [101, 127, 128, 301]
    items, cols, _ = route_cols(capfd)
    assert items == 4 and cols == [4, 2, 2, 0]
    monkeypatch.setenv("FSTAMD_BFS_TINY", "0")                    # honoured: no LDS tier
    check_chain(rhs, blob, seqs, exp=exp_chain)
    items, cols, _ = route_cols(capfd)
    assert cols == [0, 0, 4, 0]


# ---- 5 / 6. arena growth, shards ---------------------------------------------------------------

@pytest.fixture(scope="module")
def forty():
    rng = np.random.default_rng(23)
    rhs_fst = random_rhs(rng, 9, 50, 3, eps=True)
    blob = O.freeze(rhs_fst)
    fsts = [random_rhs(rng, int(rng.integers(1, 9)), int(rng.integers(1, 25)), 3, eps=True)
            for _ in range(40)]
    seqs = [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, 14)))] for _ in range(40)]
    return (blob, fsts, seqs, [oracle(f, blob) for f in fsts],
            [oracle(chain_fst(s), blob) for s in seqs])


def test_arena_growth(forty, monkeypatch):
    blob, fsts, seqs, exp, exp_chain = forty
    rhs = load_blob(blob)
    plain, _ = check_lhs(rhs, blob, fsts, exp=exp)
    plain_chain, _ = check_chain(rhs, blob, seqs, exp=exp_chain)
    assert int(plain.state_offsets[-1]) > 4 and int(plain.arc_offsets[-1]) > 8
    assert int(plain_chain.state_offsets[-1]) > 4 and int(plain_chain.arc_offsets[-1]) > 8
    monkeypatch.setenv("FSTAMD_LATTICE_ARENA", "4,8")
    grown, _ = check_lhs(rhs, blob, fsts, exp=exp)
    grown_chain, _ = check_chain(rhs, blob, seqs, exp=exp_chain)
    same_bytes(plain, grown)
    same_bytes(plain_chain, grown_chain)


def test_three_shards_equal_one(forty):
    blob, fsts, seqs, exp, exp_chain = forty
    rhs = load_blob(blob)
    one, _ = check_lhs(rhs, blob, fsts, exp=exp)
    three, _ = check_lhs(rhs, blob, fsts, exp=exp, devices=[0], shards=3)
    same_bytes(one, three)
    one, _ = check_chain(rhs, blob, seqs, exp=exp_chain)
    three, _ = check_chain(rhs, blob, seqs, exp=exp_chain, devices=[0], shards=3)
    same_bytes(one, three)


@pytest.mark.parametrize("project_connect", [False, True])
def test_shards_do_not_show_on_the_edge_batch(project_connect):
    rhs = tagger_rhs()
    lhs = F.LhsBatch.from_fsts(SY.edge_networks())
    one = assert_shards_do_not_show(lambda **kw: F.compose_frozen_lhs_batch(
        rhs, lhs, project_output=project_connect, connect=project_connect, **kw))
    assert one.status.tolist().count(F.FST_PATH_OK) >= 44
    assert int(one.status[9]) == F.FST_PATH_UNSUPPORTED                        # (9: the NaN)
    assert int(one.state_offsets[-1]) > 100 and int(one.arc_offsets[-1]) > 200


# ---- 7. projection -----------------------------------------------------------------------------

def test_project_output(forty):
    blob, fsts, seqs, exp, exp_chain = forty
    rhs = load_blob(blob)
    plain, _ = check_lhs(rhs, blob, fsts, exp=exp)
    proj, _ = check_lhs(rhs, blob, fsts, exp=exp, project=True)   # ilabels == oracle olabels
    assert np.array_equal(proj.ilabels, plain.olabels)
    assert not np.array_equal(plain.ilabels, plain.olabels)
    for name in ARRAYS:
        if name != "ilabels":
            assert getattr(plain, name).tobytes() == getattr(proj, name).tobytes(), name
    plain, _ = check_chain(rhs, blob, seqs, exp=exp_chain)
    proj, _ = check_chain(rhs, blob, seqs, exp=exp_chain, project=True)
    assert np.array_equal(proj.ilabels, plain.olabels)
    for name in ARRAYS:
        if name != "ilabels":
            assert getattr(plain, name).tobytes() == getattr(proj, name).tobytes(), name


# ---- 8. cascade ----------------------------------------------------------------------------------

def cascade_stages():
    """A tagger-like rhs1 whose cheaper reading of label 5 (-> 10, cost 1) is the dearer one
    for rhs2 (10 costs 5, 11 costs 0): committing to a 1-best between the stages loses."""
    r1 = O.Fst(start=0, finals=[0.0, INF],
               arcs=[[(5, 10, 1.0, 0), (5, 11, 2.0, 0), (6, 0, 0.5, 1), (7, 13, 0.0, 0)],
                     [(0, 12, 0.25, 0)]])
    r2 = O.Fst(start=0, finals=[0.125],
               arcs=[[(10, 20, 5.0, 0), (11, 21, 0.0, 0), (12, 22, 1.0, 0), (13, 0, 0.5, 0),
                      (13, 23, 2.0, 0)]])
    return r1, r2


def projected(lat: O.Fst) -> O.Fst:
    return O.Fst(start=lat.start, finals=list(lat.finals),
                 arcs=[[(ol, ol, w, nx) for (_, ol, w, nx) in al] for al in lat.arcs])


def total(e):
    """An expect() tuple's total weight: the fold of the arc weights and the final."""
    w = np.array(e[3], np.uint64).view(np.float64)
    return float(np.sum(w)) + float(np.array([e[4]], np.uint64).view(np.float64)[0])


@pytest.fixture(scope="module")
def cascade_case():
    rng = np.random.default_rng(31)
    r1, r2 = cascade_stages()
    b1, b2 = O.freeze(r1), O.freeze(r2)
    seqs = [[5]] + [[int(x) for x in rng.integers(5, 8, int(rng.integers(1, 9)))]
                    for _ in range(23)]
    mids = []
    for s in seqs:
        rc, lat = O.compose(chain_fst(s), b1)
        assert rc == O.OR_OK
        mids.append(projected(lat))
    return b1, b2, seqs, mids


def test_cascade_keeps_the_global_optimum(cascade_case):
    b1, b2, seqs, mids = cascade_case
    rhs1, rhs2 = load_blob(b1), load_blob(b2)
    lat = F.compose_frozen_batch(rhs1, *csr_of(seqs), project_output=True)
    assert np.all(lat.status == OK)
    lhs = lat.as_lhs()
    assert lhs.ilabels.ctypes.data == lat.ilabels.ctypes.data       # the same memory
    results = {}
    for sem in (LAZY, EAGER):
        got = F.compose_frozen_shortest_path_lhs_batch(rhs2, lhs, 1, sem)
        exp = [expect(m, b2, sem) for m in mids]
        for i, e in enumerate(exp):
            assert got_item(got, i) == e, (i, sem)
        results[sem] = exp
    # the pipeline commits to stage 1's 1-best: on item 0 ([5]) the oracle's two stages give
    # 5 -> 10 (1.0) then 10 -> 20 (5.0); the cascade takes 5 -> 11 -> 21 for 2.0
    labels, offsets = csr_of(seqs)
    for sem in (LAZY, EAGER):
        pipe = F.pipeline_batch([rhs1, rhs2], labels, offsets, 1, sem)
        e0 = results[sem][0]
        assert e0[0] == OK and e0[2] == [21] and total(e0) == 2.125
        # in the oracle: stage 1's 1-best, its output tape, stage 2
        rc, p1 = O.compose_shortest_path(chain_fst(seqs[0]), b1, 1)
        il1, ol1, w1, fin1 = O.chain(p1)
        assert ol1 == [10] and sum(w1) + fin1 == 1.0
        rc, p2 = O.compose_shortest_path(chain_fst(ol1), b2, 1)
        il2, ol2, w2, fin2 = O.chain(p2)
        assert ol2 == [20] and sum(w2) + fin2 == 5.125
        assert total(e0) < sum(w2) + fin2 < sum(w1) + fin1 + sum(w2) + fin2
        p = got_item(pipe, 0)
        assert p[0] == OK and p[2] == [20] and total(p) == 5.125 and total(e0) < total(p)


# ---- 9. NaN ----------------------------------------------------------------------------------------

def test_nan_items_are_unsupported(forty):
    blob, fsts, _, exp, _ = forty
    rhs = load_blob(blob)
    nan_arc = O.Fst(start=0, finals=[INF, 0.0], arcs=[[(1, 1, math.nan, 1)], []])
    nan_final = O.Fst(start=0, finals=[math.nan], arcs=[[]])
    items = fsts[:3] + [nan_arc] + fsts[3:6] + [nan_final] + fsts[6:9]
    got = F.compose_frozen_lhs_batch(rhs, batch_of(items))
    assert_layout(got)
    good = [i for i in range(len(items)) if i not in (3, 7)]
    for i, c in zip(good, exp[:9]):
        assert_item(got, i, c)
    for i in (3, 7):
        assert int(got.status[i]) == UNSUPPORTED
        assert int(got.state_offsets[i]) == int(got.state_offsets[i + 1])
        assert int(got.start[i]) == NO_STATE
    # a NaN in the rhs: every item
    nan_rhs = O.Fst(start=0, finals=[0.0], arcs=[[(1, 1, math.nan, 0)]])
    got = F.compose_frozen_batch(load_blob(O.freeze(nan_rhs)), *csr_of([[1], [], [1, 1]]))
    assert got.status.tolist() == [UNSUPPORTED] * 3
    assert got.state_offsets.tolist() == [0] * 4 and got.arc_offsets.tolist() == [0]
    assert got.start.tolist() == [NO_STATE] * 3


# ---- 10. device entry -------------------------------------------------------------------------------

def dev_tensor(a: np.ndarray):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.as_tensor(a.view(signed) if signed else a, device="cuda:0")


class DeviceLattices:
    def __init__(self, num, scap, acap):
        dev = "cuda:0"
        self.num, self.scap, self.acap = num, scap, acap
        z = lambda n, dt: torch.full((max(n, 1),), 77, dtype=dt, device=dev)
        self.status, self.soff, self.start = z(num, torch.int32), z(num + 1, torch.int64), z(num, torch.int32)
        self.fin, self.aoff = z(scap, torch.float64), z(scap + 1, torch.int64)
        self.il, self.ol, self.nx = z(acap, torch.int32), z(acap, torch.int32), z(acap, torch.int32)
        self.w = z(acap, torch.float64)
        self.desc = FF.FstDeviceLattices(
            self.status.data_ptr(), self.soff.data_ptr(), self.start.data_ptr(),
            self.fin.data_ptr(), self.aoff.data_ptr(), self.il.data_ptr(), self.ol.data_ptr(),
            self.w.data_ptr(), self.nx.data_ptr(), scap, acap)

    def arrays(self, ns, na):
        u32 = lambda t, n: t.cpu().numpy().view(np.uint32)[:n]
        return {"status": self.status.cpu().numpy()[:self.num],
                "state_offsets": self.soff.cpu().numpy().view(np.uint64)[:self.num + 1],
                "start": u32(self.start, self.num),
                "final_weights": self.fin.cpu().numpy()[:ns],
                "arc_offsets": self.aoff.cpu().numpy().view(np.uint64)[:ns + 1],
                "ilabels": u32(self.il, na), "olabels": u32(self.ol, na),
                "weights": self.w.cpu().numpy()[:na], "nextstates": u32(self.nx, na)}

    def as_device_lhs(self):
        return FF.FstLhsBatch(self.num, self.soff.data_ptr(), self.start.data_ptr(),
                              self.fin.data_ptr(), self.aoff.data_ptr(), self.il.data_ptr(),
                              self.ol.data_ptr(), self.w.data_ptr(), self.nx.data_ptr())


def run_device(rhs, d_lab, d_off, num, max_len, out: DeviceLattices, project=True):
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    needed = (C.c_uint64 * 2)(0, 0)
    rc = F.lib().fst_device_compose_frozen(
        rhs.h, d_lab.data_ptr(), d_off.data_ptr(), num, max_len,
        FF.FST_LATTICE_PROJECT_OUTPUT if project else 0, C.byref(opts), C.byref(out.desc),
        needed, None)
    assert rc == FF.FST_OK
    return int(needed[0]), int(needed[1])


def test_device_entry(cascade_case):
    b1, b2, seqs, mids = cascade_case
    rhs1, rhs2 = load_blob(b1), load_blob(b2)
    num = len(seqs)
    labels, offsets = csr_of(seqs)
    host = F.compose_frozen_batch(rhs1, labels, offsets, project_output=True)
    ns, na = int(host.state_offsets[-1]), int(host.arc_offsets[-1])
    d_lab, d_off = dev_tensor(labels), dev_tensor(offsets)
    max_len = max(len(s) for s in seqs)

    def equal_host(out):
        got = out.arrays(ns, na)
        for name in ARRAYS:
            assert got[name].tobytes() == getattr(host, name).tobytes(), name

    # ample capacity: the host entry's arrays
    ample = DeviceLattices(num, ns + 100, na + 100)
    assert run_device(rhs1, d_lab, d_off, num, max_len, ample) == (ns, na)
    assert F.last_launch_stats().engine == 10
    equal_host(ample)
    assert int(ample.fin.cpu()[ns]) == 77 and int(ample.il.cpu()[na]) == 77   # nothing past them
    # one short on either side: the exact totals come back, nothing is written past a
    # capacity, and a second call with them succeeds
    for scap, acap in ((ns - 1, na), (ns, na - 1)):
        short = DeviceLattices(num, scap, acap)
        assert run_device(rhs1, d_lab, d_off, num, max_len, short) == (ns, na)
        assert np.array_equal(short.status.cpu().numpy()[:num], host.status)
        assert int(short.fin.cpu()[scap - 1]) == 77 and int(short.il.cpu()[acap - 1]) == 77
    exact = DeviceLattices(num, ns, na)
    assert run_device(rhs1, d_lab, d_off, num, max_len, exact) == (ns, na)
    equal_host(exact)
    # no strings: the two closing offsets and needed = {0, 0}
    none = DeviceLattices(0, 0, 0)
    assert run_device(rhs1, d_lab, d_off, 0, 0, none) == (0, 0)
    assert int(none.soff.cpu()[0]) == 0 and int(none.aoff.cpu()[0]) == 0
    # the arrays chain into the device lhs entry and the text emission: test 8's results
    cs = exact.as_device_lhs()
    for sem in (LAZY, EAGER):
        paths = DeviceOut(num, 16 * na + 1024)
        opts = FF.FstBatchOptions(0, sem, 0, 0, 0)
        rc = F.lib().fst_device_compose_shortest_path_lhs(rhs2.h, C.byref(cs), 1, C.byref(opts),
                                                          C.byref(paths.desc), None)
        assert rc == FF.FST_OK
        exp = [expect(m, b2, sem) for m in mids]
        assert paths.items() == exp
        # ... as text
        dev = "cuda:0"
        cap = 8 * na + 64
        text = torch.zeros(cap, dtype=torch.uint8, device=dev)
        toff = torch.zeros(num + 1, dtype=torch.int64, device=dev)
        tst = torch.zeros(num, dtype=torch.int32, device=dev)
        tw = torch.zeros(num, dtype=torch.float64, device=dev)
        tot = C.c_uint64(0)
        rc = F.lib().fst_device_emit_text(C.byref(paths.desc), num, text.data_ptr(), cap,
                                          toff.data_ptr(), tst.data_ptr(), tw.data_ptr(),
                                          C.byref(tot), None)
        assert rc == FF.FST_OK
        raw, off = bytes(text.cpu().numpy()), toff.cpu().numpy()
        for i, e in enumerate(exp):
            want = bytes(l - 1 for l in e[2] if l != 0) if e[0] == OK else b""
            assert int(tst.cpu()[i]) == e[0] and raw[int(off[i]):int(off[i + 1])] == want, i
        host_paths = F.compose_frozen_shortest_path_lhs_batch(rhs2, host.as_lhs(), 1, sem)
        assert F.batch_result_to_text(host_paths).texts() == \
            [raw[int(off[i]):int(off[i + 1])] for i in range(num)]
