"""GPU: shortest path of a batch of lattices with no compose -- fst_shortest_path_lhs_batch and
fst_device_shortest_path_lhs -- against the CPU oracle's shortestPath (O.shortest_path), item by
item, bit for bit.

"Equal" is always status, path length, ilabels, olabels and the bit patterns of every arc weight
and of the final weight.  The tests sit on what the engine adds: the single call's status order
per item, the 64-state chunks of the wave tier, the hand-over to the frontier tier, the replay
tier's item list, and the identity shortest_path(compose_frozen(x, b)) = the eager 1-best entry.
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
from test_gpu_lattice_batch import DeviceLattices, dev_tensor
from test_gpu_lhs_batch import (assert_shards_do_not_show, batch_of, bits, got_item,
                                same_result)
from test_gpu_lhs_device import DeviceLhs, DeviceOut
from test_gpu_parity import load_blob

pytestmark = pytest.mark.gpu

EAGER = F.FST_SEM_EAGER
INF, NAN = math.inf, math.nan
OK, EMPTY, CYCLE = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_CYCLE
ERROR_N, UNSUPPORTED, FULL = F.FST_PATH_ERROR_N, F.FST_PATH_UNSUPPORTED, F.FST_PATH_OUTPUT_FULL
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)


def has_nan(f: O.Fst):
    return (any(math.isnan(x) for x in f.finals) or
            any(math.isnan(a[2]) for al in f.arcs for a in al))


def expect(f: O.Fst, n=1):
    """(status, ilabels, olabels, weight bits, final bits) of fst_shortest_path(f, n).  The oracle
    reports a NaN only where it compares one (a NaN final weight passes it); the entry's rule is
    the single call's, which refuses an item that holds one anywhere, after its tests of the
    start and of n."""
    rc, ref = O.shortest_path(f, n)
    if rc in (O.OR_OK, O.OR_ERR_CYCLE) and n == 1 and f.start != O.NO_STATE and has_nan(f):
        return (UNSUPPORTED,)
    if rc == O.OR_ERR_UNSUPPORTED_N:
        return (ERROR_N,)
    if rc == O.OR_ERR_CYCLE:
        return (CYCLE,)
    if rc == O.OR_ERR_NAN:
        return (UNSUPPORTED,)
    assert rc == O.OR_OK, rc
    ch = O.chain(ref)
    if ch is None:
        return (EMPTY,)
    il, ol, w, fin = ch
    return (OK, il, ol, bits(w).tolist(), int(bits([fin])[0]))


def items_of(got, num):
    return [got_item(got, i) for i in range(num)]


def check(fsts, n=1, exp=None, lhs=None, **kw):
    lhs = lhs if lhs is not None else batch_of(fsts)
    got = F.shortest_path_lhs_batch(lhs, n, **kw)
    assert len(got.status) == len(fsts) and int(got.offsets[0]) == 0
    exp = exp if exp is not None else [expect(f, n) for f in fsts]
    for i, e in enumerate(exp):
        assert got_item(got, i) == e, (i, n)
    return got, exp


def sp_line(capfd):
    """The last `lattice sp:` route line: (items, wave, frontier, replay)."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lattice sp:" in ln]
    assert lines, err
    m = re.search(r"lattice sp: items (\d+) \| wave (\d+) frontier (\d+) replay (\d+) \| [\d.]+ ms",
                  lines[-1])
    assert m, lines[-1]
    return tuple(int(x) for x in m.groups())


def fst(start, finals, arcs):
    return O.Fst(start=O.NO_STATE if start is None else start, finals=list(finals),
                 arcs=[list(a) for a in arcs])


# ---- 1. known answers and tie rules --------------------------------------------------------------

def known():
    """(item, expected status, expected (ilabels, final weight) or None)."""
    return [
        # shortest-path.zig:143-176: 0 -1-> 1 -2-> 2 beats 0 -5-> 3 -1-> 2
        (fst(0, [INF, INF, 0.0, INF], [[(1, 1, 1.0, 1), (3, 3, 5.0, 3)], [(2, 2, 2.0, 2)], [],
                                       [(4, 4, 1.0, 2)]]), OK, ([1, 2], 0.0)),
        # :178-189: the empty FST
        (O.Fst(), EMPTY, None),
        # :191-216: two arcs into one state, the cheaper one is kept with its labels
        (fst(0, [INF, 0.0], [[(10, 100, 3.0, 1), (11, 101, 1.0, 1)], []]), OK, ([11], 0.0)),
        # two equal-weight paths into state 3: the smaller source id (1, not 2) wins
        (fst(0, [INF, INF, INF, 0.0], [[(7, 7, 1.0, 2), (8, 8, 1.0, 1)], [(5, 5, 1.0, 3)],
                                       [(6, 6, 1.0, 3)], []]), OK, ([8, 5], 0.0)),
        # two tight arcs from the same source: the earlier one wins
        (fst(0, [INF, 0.5], [[(3, 30, 1.0, 1), (4, 40, 1.0, 1), (5, 50, 0.5, 1), (6, 60, 0.5, 1)],
                             []]), OK, ([5], 0.5)),
        # two finals of equal total (1 + 1 = 0.5 + 1.5): the smaller id wins
        (fst(0, [INF, 1.5, 1.0], [[(1, 1, 1.0, 2), (2, 2, 0.5, 1)], [], []]), OK, ([2], 1.5)),
        # the start is its own best final: OK with zero arcs
        (fst(0, [0.25, 0.0], [[(1, 1, 0.5, 1)], []]), OK, ([], 0.25)),
        # a start that is not state 0
        (fst(2, [0.0, INF, INF], [[], [(9, 9, 0.5, 0)], [(4, 4, 1.0, 1), (5, 5, 2.0, 0)]]),
         OK, ([4, 9], 0.0)),
        # unreachable states: 3 -> 4 (final) is a component of its own beside 0 -> 1 (final)
        (fst(0, [INF, 2.0, INF, INF, 0.0], [[(1, 1, 1.0, 1)], [], [(2, 2, 0.0, 0)],
                                            [(3, 3, 0.0, 4)], []]), OK, ([1], 2.0)),
        # a final state reachable only from states the start cannot reach
        (fst(0, [INF, INF, INF, 0.0], [[(1, 1, 1.0, 1)], [], [(2, 2, 0.0, 3)], []]), EMPTY, None),
    ]


def test_known_answers_and_tie_rules():
    cases = known()
    fsts = [c[0] for c in cases]
    got, exp = check(fsts)
    assert F.last_launch_stats().engine == 12
    for i, (f, st, ans) in enumerate(cases):
        assert exp[i][0] == st, i
        if ans is not None:
            assert exp[i][1] == ans[0] and exp[i][4] == int(bits([ans[1]])[0]), i
    # shortest-path.zig:218-229: n = 2 is refused
    got, exp = check([fst(0, [0.0], [[]])], n=2)
    assert exp == [(ERROR_N,)] and F.last_launch_stats().engine == 12
    # an ordinary FstBatchResult: the text helper works on it
    texts = F.batch_result_to_text(F.shortest_path_lhs_batch(batch_of([
        fst(0, [INF, INF, 0.0], [[(ord("h") + 1, ord("o") + 1, 0.0, 1)],
                                 [(ord("i") + 1, ord("k") + 1, 0.0, 2)], []])]))).texts()
    assert texts == [b"ok"]


# ---- 2. status order -----------------------------------------------------------------------------

def status_items():
    plain = lambda: fst(0, [INF, 0.25], [[(1, 2, 0.5, 1)], []])
    no_start = fst(None, [0.0, INF], [[(1, 1, 0.0, 1)], []])
    nan_arc = fst(0, [INF, 0.0], [[(1, 1, NAN, 1)], []])
    nan_final = fst(0, [INF, NAN], [[(1, 1, 1.0, 1)], []])
    return [plain(), no_start, plain(), O.Fst(), nan_arc, plain(), nan_final, plain()]


def test_status_order():
    fsts = status_items()
    for n, want in ((1, [OK, EMPTY, OK, EMPTY, UNSUPPORTED, OK, UNSUPPORTED, OK]),
                    (0, [EMPTY] * 8),
                    (2, [ERROR_N, EMPTY, ERROR_N, EMPTY, ERROR_N, ERROR_N, ERROR_N, ERROR_N])):
        got, exp = check(fsts, n=n)
        assert [e[0] for e in exp] == want, n
        assert F.last_launch_stats().engine == 12
    # the neighbours of the odd items are what they are alone
    alone, _ = check([fsts[0]])
    assert got_item(alone, 0) == got_item(F.shortest_path_lhs_batch(batch_of(fsts)), 2)


# ---- 3. chunk edges ------------------------------------------------------------------------------

def edge_item(n):
    """A forward chain of n states (arcs of weight 1) with tie-making skip arcs s -> s + 2 of
    weight 2, and at every chunk boundary b = 64 k a forward arc b - 2 -> b and a backward arc
    b -> b - 1, both free: state b - 1 is cheaper through the next chunk than along the chain."""
    f = O.Fst(start=0, finals=[INF] * n, arcs=[[] for _ in range(n)])
    f.finals[n - 1] = 0.5
    if n > 2:
        f.finals[n // 2] = 0.5 + (n - 1 - n // 2)            # ties with the last state's total
    for s in range(n - 1):
        f.add_arc(s, 1 + s % 5, 1 + s % 7, 1.0, s + 1)
        if s + 2 < n:
            f.add_arc(s, 6, 1 + s % 3, 2.0, s + 2)
    for b in range(64, n, 64):
        f.add_arc(b - 2, 7, 7, 0.0, b)
        f.add_arc(b, 8, 8, 0.0, b - 1)
    return f


@pytest.fixture(scope="module")
def edges():
    fsts = [edge_item(n) for n in SIZES]
    return fsts, [expect(f) for f in fsts]


def test_chunk_edges(edges, monkeypatch, capfd):
    fsts, exp = edges
    assert all(e[0] == OK for e in exp)
    crossing = sum(n > 64 for n in SIZES)                     # items with a backward arc
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    monkeypatch.delenv("FSTAMD_SP_SWEEPS", raising=False)
    base, _ = check(fsts, exp=exp)
    assert sp_line(capfd) == (len(fsts), len(fsts), 0, 0)     # two sweeps settle each of them
    monkeypatch.setenv("FSTAMD_SP_SWEEPS", "1")               # one sweep: the crossings stay open
    one, _ = check(fsts, exp=exp)
    assert sp_line(capfd) == (len(fsts), len(fsts) - crossing, crossing, 0)
    monkeypatch.setenv("FSTAMD_SP_SWEEPS", "0")               # the frontier tier alone
    none, _ = check(fsts, exp=exp)
    assert sp_line(capfd) == (len(fsts), 0, len(fsts), 0)
    assert same_result(base, one) and same_result(base, none)
    monkeypatch.delenv("FSTAMD_SP_SWEEPS")
    back, _ = check(fsts[::-1], exp=exp[::-1])                # another place in the batch
    assert got_item(back, 1) == got_item(base, len(fsts) - 2)


# ---- 4. random sweep -----------------------------------------------------------------------------

def random_graph(rng, weights):
    n = int(rng.integers(1, 41))
    f = O.Fst(finals=[INF] * n, arcs=[[] for _ in range(n)])
    for s in rng.choice(n, size=min(n, int(rng.integers(0, 4))), replace=False):
        f.finals[int(s)] = float(weights[int(rng.integers(len(weights)))])
    for s in range(n):
        for _ in range(int(rng.integers(0, 5))):
            f.add_arc(s, int(rng.integers(0, 5)), int(rng.integers(0, 5)),
                      float(weights[int(rng.integers(len(weights)))]), int(rng.integers(n)))
    f.start = int(rng.integers(n))
    return f


@pytest.fixture(scope="module")
def graphs():
    rng = np.random.default_rng(20270)     # 100 OK, 87 EMPTY, 13 CYCLE (asserted below)
    dyadic = [0.0, 0.5, 1.0, 1.5]
    tenths = [0.1 * k for k in range(8)]
    fsts = [random_graph(rng, dyadic if k % 2 == 0 else tenths) for k in range(200)]
    return fsts, [expect(f) for f in fsts]


def test_random_sweep(graphs, monkeypatch):
    fsts, exp = graphs
    st = [e[0] for e in exp]
    # the branches are reached, by the oracle alone
    assert st.count(CYCLE) >= 10 and st.count(EMPTY) >= 50 and st.count(OK) >= 90
    assert set(st) == {OK, EMPTY, CYCLE}
    assert sum(e[0] == OK and len(e[1]) >= 3 for e in exp) >= 30
    monkeypatch.delenv("FSTAMD_SP_SWEEPS", raising=False)
    base, _ = check(fsts, exp=exp)
    for budget in ("1", "0"):
        monkeypatch.setenv("FSTAMD_SP_SWEEPS", budget)
        other, _ = check(fsts, exp=exp)
        assert same_result(base, other)


# ---- 5. the backwards-numbered chain -------------------------------------------------------------

def test_backwards_chain_goes_to_the_frontier_tier(monkeypatch, capfd):
    n = 4096
    back = O.Fst(start=n - 1, finals=[INF] * n, arcs=[[] for _ in range(n)])
    back.finals[0] = 0.25
    for s in range(1, n):
        back.add_arc(s, 1 + s % 3, 2 + s % 2, float(s % 2), s - 1)
    back.add_arc(5, 7, 7, 1.0, 5)
    small = [c[0] for c in known()]
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    monkeypatch.delenv("FSTAMD_SP_SWEEPS", raising=False)
    fsts = small[:3] + [back] + small[3:]
    got, exp = check(fsts)
    assert exp[3][0] == OK and len(exp[3][1]) == n - 1
    # a sweep settles one more 64-state chunk of the backwards chain: 64 sweeps, beyond the budget
    assert sp_line(capfd) == (len(fsts), len(fsts) - 1, 1, 0)


# ---- 6. replay tier ------------------------------------------------------------------------------

def replay_items():
    """(item, flagged).  The flagged ones carry a negative arc, -0.0, a +inf arc or a negative
    final weight (kLhsReplay)."""
    # a negative arc out of a state that is settled before the arc is relaxed: 0 -> 1 (1), 0 -> 2
    # (2), 2 -> 1 (-3): state 1 settles at 1, relaxes 1 -> 3, then drops to -1 and is never
    # relaxed again, so 3 keeps 1 + 1 = 2 although -1 + 1 = 0 is the true distance
    settled = fst(0, [INF, INF, INF, 0.0], [[(1, 1, 1.0, 1), (2, 2, 2.0, 2)], [(3, 3, 1.0, 3)],
                                             [(4, 4, -3.0, 1)], []])
    # the same with the cheap way found in time (the negative arc leaves the start)
    in_time = fst(0, [INF, INF, 0.0], [[(1, 1, -1.0, 1), (2, 2, 0.5, 2)], [(3, 3, 1.0, 2)], []])
    minus_zero = fst(0, [INF, 0.0, INF], [[(1, 1, -0.0, 2), (2, 2, 0.0, 1)], [], [(3, 3, 0.0, 1)]])
    inf_arc = fst(0, [INF, 0.0, 0.0], [[(1, 1, INF, 1), (2, 2, 3.0, 2)], [], []])
    neg_final = fst(0, [INF, 1.0, -2.0], [[(1, 1, 0.5, 1), (2, 2, 2.0, 2)], [], []])
    neg_cycle = fst(0, [INF, 0.0], [[(1, 1, 1.0, 1)], [(2, 2, -1.0, 0)]])
    plain = lambda k: fst(0, [INF, INF, 0.5], [[(1, 1, 0.5 * k, 1), (2, 2, 2.0, 2)],
                                               [(3, 3, 1.0, 2)], []])
    return [(plain(1), False), (settled, True), (in_time, True), (plain(2), False),
            (minus_zero, True), (inf_arc, True), (plain(3), False), (neg_final, True),
            (neg_cycle, True), (plain(4), False)]


def test_replay_tier(monkeypatch, capfd):
    cases = replay_items()
    fsts = [c[0] for c in cases]
    flagged = sum(c[1] for c in cases)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    got, exp = check(fsts)
    assert sp_line(capfd) == (len(fsts), len(fsts) - flagged, 0, flagged)
    # the settled-state rule shows: state 1's back-pointer moves to the negative arc after it
    # has settled, so the path is 0 -> 2 -> 1 -> 3 (total 0) under a recorded distance of 2
    assert exp[1][:2] == (OK, [2, 4, 3]) and exp[2][:2] == (OK, [1, 3])
    assert exp[7][:2] == (OK, [2]) and exp[8] == (CYCLE,)
    monkeypatch.setenv("FSTAMD_SP_SWEEPS", "0")               # the budget is not the replay's
    other, _ = check(fsts, exp=exp)
    assert same_result(got, other)


# ---- 7. the identity with the eager engine -------------------------------------------------------

def tagger_blob():
    ns, start, finals, arcs = SY.tagger()
    return O.freeze(O.Fst(start=start, finals=finals, arcs=arcs))


def verbalizer_blob():
    ns, start, finals, arcs = SY.verbalizer()
    return O.freeze(O.Fst(start=start, finals=finals, arcs=arcs))


def assert_identity(rhs, lat: F.LatticeBatch, eager, what):
    """shortest_path(lattice i) = the eager 1-best entry's item i, wherever the compose is OK."""
    num = len(lat)
    got = F.shortest_path_lhs_batch(lat.as_lhs())
    differ = [i for i in range(num)
              if int(lat.status[i]) == OK and got_item(got, i) != got_item(eager, i)]
    assert not differ, (what, differ[:5])
    for i in range(num):                                      # a non-OK lattice owns no states
        if int(lat.status[i]) != OK:
            assert got_item(got, i) == (EMPTY,), (what, i)
    return got


@pytest.fixture(scope="module")
def utterance_case():
    texts = SY.utterances(np.random.default_rng(3), 300)
    return load_blob(tagger_blob()), texts


def test_identity_with_the_eager_chain_entry(utterance_case):
    rhs, texts = utterance_case
    labels, offsets = SY.to_labels(texts)
    eager = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, EAGER)
    assert int(np.sum(eager.status == OK)) > 250
    for connect in (False, True):
        lat = F.compose_frozen_batch(rhs, labels, offsets, connect=connect)
        assert np.all(lat.status == OK)
        got = assert_identity(rhs, lat, eager, ("tagger", connect))
        assert F.last_launch_stats().engine == 12
        assert np.array_equal(got.status, eager.status)
    # the toy verbalizer: dead ends, and whole items without a path
    vrhs = load_blob(verbalizer_blob())
    vtexts = [t.replace("1", "#b").replace("2", "#z") for t in texts][:64]
    labels, offsets = SY.to_labels(vtexts)
    eager = F.compose_frozen_shortest_path_batch(vrhs, labels, offsets, 1, EAGER)
    assert EMPTY in eager.status.tolist() and OK in eager.status.tolist()
    for connect in (False, True):
        lat = F.compose_frozen_batch(vrhs, labels, offsets, connect=connect)
        assert_identity(vrhs, lat, eager, ("verbalizer", connect))


def test_identity_with_the_eager_lhs_entry(utterance_case):
    rhs, texts = utterance_case
    rng = np.random.default_rng(11)
    lhs = F.LhsBatch.from_fsts([SY.confusion_network(rng, t, 4, 0.3) for t in texts[:120]])
    eager = F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, 1, EAGER)
    assert int(np.sum(eager.status == OK)) > 60
    for connect in (False, True):
        lat = F.compose_frozen_lhs_batch(rhs, lhs, connect=connect)
        assert_identity(rhs, lat, eager, ("confusion networks", connect))


# ---- 8. a rescored batch -------------------------------------------------------------------------

def item_fst(lhs: F.LhsBatch, i) -> O.Fst:
    s0, s1 = int(lhs.state_offsets[i]), int(lhs.state_offsets[i + 1])
    ao = lhs.arc_offsets[s0:s1 + 1].astype(np.int64)
    arcs = [list(zip(lhs.ilabels[a:z].tolist(), lhs.olabels[a:z].tolist(),
                     lhs.weights[a:z].tolist(), lhs.nextstates[a:z].tolist()))
            for a, z in zip(ao[:-1].tolist(), ao[1:].tolist())]
    start = int(lhs.start[i]) if s1 > s0 else O.NO_STATE
    return O.Fst(start=start, finals=lhs.final_weights[s0:s1].tolist(), arcs=arcs)


def test_a_rescored_batch(utterance_case):
    rhs, texts = utterance_case
    rng = np.random.default_rng(17)
    cn = F.LhsBatch.from_fsts([SY.confusion_network(rng, t, 4, 0.3) for t in texts[:100]])
    lat = F.compose_frozen_lhs_batch(rhs, cn)
    before = F.shortest_path_lhs_batch(lat.as_lhs())
    plain = lat.as_lhs()
    cost = np.random.default_rng(23).integers(0, 9, len(plain.weights)) * 0.25
    rescored = F.LhsBatch(plain.state_offsets, plain.start, plain.final_weights,
                          plain.arc_offsets, plain.ilabels, plain.olabels, plain.weights + cost,
                          plain.nextstates)
    fsts = [item_fst(rescored, i) for i in range(len(rescored))]
    got, exp = check(fsts, lhs=rescored)
    moved = [i for i in range(len(fsts))
             if exp[i][0] == OK and got_item(before, i)[:3] != exp[i][:3]]
    assert len(moved) >= 1 and sum(e[0] == OK for e in exp) > 50


# ---- 9. grid and shards do not show --------------------------------------------------------------

def test_grid_and_shards_do_not_show(graphs, edges, monkeypatch):
    fsts = graphs[0][:80] + edges[0] + [c[0] for c in replay_items()]
    exp = graphs[1][:80] + edges[1] + [expect(c[0]) for c in replay_items()]
    base, _ = check(fsts, exp=exp)
    monkeypatch.setenv("FSTAMD_GRAPH_GRID", "1")
    one, _ = check(fsts, exp=exp)
    assert same_result(base, one)
    monkeypatch.delenv("FSTAMD_GRAPH_GRID")
    sharded, _ = check(fsts, exp=exp, devices=[0], shards=3)
    assert same_result(base, sharded)
    for name in ("status", "offsets", "ilabels", "olabels", "weights", "finals"):
        assert getattr(base, name).tobytes() == getattr(sharded, name).tobytes(), name
        assert getattr(base, name).tobytes() == getattr(one, name).tobytes(), name


def test_shards_do_not_show_on_the_edge_batch():
    lhs = F.LhsBatch.from_fsts(SY.edge_networks())
    one = assert_shards_do_not_show(lambda **kw: F.shortest_path_lhs_batch(lhs, 1, **kw))
    st = one.status.tolist()
    assert st[13] == EMPTY and st[21] == OK and st.count(OK) >= 45           # (13: no states)
    assert int(one.offsets[22]) == int(one.offsets[21])                       # one state: no arc


# ---- 10. device entry ----------------------------------------------------------------------------

def run_device_sp(cs, num, cap, n=1):
    out = DeviceOut(num, cap)
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    rc = F.lib().fst_device_shortest_path_lhs(C.byref(cs), n, C.byref(opts), C.byref(out.desc),
                                              None)
    assert rc == FF.FST_OK
    return out


def emit_text(paths: DeviceOut, num, cap):
    dev = "cuda:0"
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
    return [raw[int(off[i]):int(off[i + 1])] for i in range(num)], tst.cpu().numpy().tolist()


def test_device_entry(utterance_case):
    rhs, texts = utterance_case
    texts = texts[:96]
    num = len(texts)
    labels, offsets = SY.to_labels(texts)
    host_lat = F.compose_frozen_batch(rhs, labels, offsets)
    host = F.shortest_path_lhs_batch(host_lat.as_lhs())
    host_items = items_of(host, num)
    host_texts = F.batch_result_to_text(host).texts()
    ns, na = int(host_lat.state_offsets[-1]), int(host_lat.arc_offsets[-1])
    # chains -> lattices on the device
    lat = DeviceLattices(num, ns, na)
    needed = (C.c_uint64 * 2)(0, 0)
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    d_lab, d_off = dev_tensor(labels), dev_tensor(offsets)
    rc = F.lib().fst_device_compose_frozen(rhs.h, d_lab.data_ptr(), d_off.data_ptr(), num,
                                           max(len(t) for t in texts), 0, C.byref(opts),
                                           C.byref(lat.desc), needed, None)
    assert rc == FF.FST_OK and (int(needed[0]), int(needed[1])) == (ns, na)
    cs = lat.as_device_lhs()
    # -> 1-best -> text, never leaving the device
    paths = run_device_sp(cs, num, ns)
    assert F.last_launch_stats().engine == 12
    assert paths.items() == host_items
    need = sum(len(e[1]) for e in host_items if e[0] == OK)
    assert paths.cursor() == need == int(host.offsets[-1])
    got_texts, text_status = emit_text(paths, num, 8 * na + 64)
    assert got_texts == host_texts and text_status == [e[0] for e in host_items]
    # an arena one arc short: the items that do not fit say so, the cursor says what is needed
    short = run_device_sp(cs, num, need - 1)
    st = short.status.cpu().numpy()[:num].tolist()
    assert short.cursor() == need and FULL in st
    for i, e in enumerate(short.items()):
        assert e == host_items[i] or e == (FULL,), i
    exact = run_device_sp(cs, num, short.cursor())
    assert exact.items() == host_items
    # n is the single call's
    assert all(e == (EMPTY,) for e in run_device_sp(cs, num, ns, n=0).items())
    assert all(e == (ERROR_N,) for e in run_device_sp(cs, num, ns, n=2).items())


def test_device_entry_validates_per_item(graphs):
    fsts = graphs[0][:40]
    exp = graphs[1][:40]
    lhs = batch_of(fsts)
    victim = next(i for i, f in enumerate(fsts) if any(f.arcs) and exp[i][0] == OK)
    bad = F.LhsBatch(lhs.state_offsets, lhs.start, lhs.final_weights, lhs.arc_offsets, lhs.ilabels,
                     lhs.olabels, lhs.weights, lhs.nextstates.copy())
    s0 = int(lhs.state_offsets[victim])
    a0 = int(lhs.arc_offsets[s0])
    bad.nextstates[a0] = fsts[victim].num_states              # one past the item's last state
    d = DeviceLhs(bad)
    out = run_device_sp(d.cs, len(fsts), int(lhs.state_offsets[-1]))
    for i, e in enumerate(out.items()):
        assert e == ((UNSUPPORTED,) if i == victim else exp[i]), i
    # state offsets that decrease anywhere: no item is run
    worse = F.LhsBatch(lhs.state_offsets.copy(), lhs.start, lhs.final_weights, lhs.arc_offsets,
                       lhs.ilabels, lhs.olabels, lhs.weights, lhs.nextstates)
    assert int(worse.state_offsets[2]) > 0
    worse.state_offsets[3] = worse.state_offsets[2] - 1
    d = DeviceLhs(worse)
    out = run_device_sp(d.cs, len(fsts), int(lhs.state_offsets[-1]))
    assert out.items() == [(UNSUPPORTED,)] * len(fsts)
