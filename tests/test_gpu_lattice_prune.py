"""GPU: fst_prune_lhs_batch / fst_device_prune_lhs against model (a) of tests/prune_model.py, bit
for bit on start, state_offsets, arc_offsets, finals, labels, weight bits and next states.

The tests sit on what the prune adds: the statuses and their order, both sweeps of the wave tier
at the edges of its 64-state chunks and of its LDS bound, the frontier tier behind it, the cut on
f64 values, and the chain into the other lhs entries."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import libfst_amd as F
import libfst_amd.fst as FF
import prune_model as PM
from libfst_amd import synthetic as SY
from test_gpu_lattice_batch import ARRAYS, DeviceLattices, assert_layout, same_bytes
from test_gpu_lattice_sp import emit_text, tagger_blob
from test_gpu_lhs_batch import bits, got_item
from test_gpu_lhs_device import DeviceLhs, DeviceOut
from test_gpu_parity import load_blob

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
OK, UNSUPPORTED, NO_STATE = F.FST_PATH_OK, F.FST_PATH_UNSUPPORTED, F.FST_NO_STATE
BEAMS = (0.0, 0.5, 1.5, INF)
LDS = 256   # the wave tier keeps its keys in LDS up to this many states (kPruneLdsStates)


def check(fsts, beam, exp=None, cache=None, **kw):
    got = F.prune_lhs_batch(F.LhsBatch.from_fsts(fsts), beam, **kw)
    assert len(got) == len(fsts)
    assert_layout(got)
    exp = exp if exp is not None else PM.prune_batch(fsts, beam, cache)
    PM.assert_batch_equal(got, exp, beam)
    return got


def prune_line(capfd):
    """The last `lattice prune:` route line: (items, wave, frontier, states in, out, arcs in, out)."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lattice prune:" in ln]
    assert lines, err
    m = re.search(r"lattice prune: items (\d+) \| wave (\d+) frontier (\d+) \| states (\d+) -> "
                  r"(\d+) arcs (\d+) -> (\d+) \| [0-9.]+ ms", lines[-1])
    assert m, lines[-1]
    return tuple(int(x) for x in m.groups())


# ---- 1. known answers --------------------------------------------------------------------------

def diamond():
    # 0 -1-> 1 -0-> 3 (total 1), 0 -3-> 2 -0-> 3 (total 3); final(3) = 0
    return (0, [INF, INF, INF, 0.0],
            [[(1, 1, 1.0, 1), (2, 2, 3.0, 2)], [(3, 3, 0.0, 3)], [(4, 4, 0.0, 3)], []])


def known():
    return [
        diamond(),
        (0, [0.0, 0.0], [[(1, 1, 1.0, 1)], []]),                      # a start that is final
        (0, [5.0, 0.0], [[(1, 1, 1.0, 1)], []]),                      # a final weight that is cut
        (0, [INF, INF], [[(1, 1, 0.0, 1)], []]),                      # no final
        (None, [], []),                                               # zero states
        (0, [INF, 0.0], [[(1, 1, INF, 1), (2, 2, 1.0, 1)], []]),      # a +inf arc
        (0, [INF, 0.0], [[(1, 1, -1.0, 1)], []]),                     # a negative arc
        (0, [INF, NAN], [[(1, 1, 0.0, 1)], []]),                      # a NaN
        (0, [INF, -2.0, 0.0], [[(1, 1, 1.0, 1), (2, 2, 0.0, 2)], [], []]),   # a negative final
        (0, [INF, -0.0, 0.0], [[(1, 1, -0.0, 1), (2, 2, 0.0, 2)], [(3, 3, -0.0, 2)], []]),
        (0, [INF, 0.0], [[(1, 1, 0.0, 0), (2, 2, 1.0, 1)], []]),      # a self-loop of weight 0
        (0, [INF, 0.0], [[(1, 1, 1.0, 0), (2, 2, 1.0, 1)], []]),      # ... of weight 1
        (0, [INF, INF, 0.0], [[(1, 1, 0.0, 1)], [(2, 2, 0.0, 0), (3, 3, 1.0, 2)], []]),  # 2-cycle, 0
        (0, [INF, INF, 0.0], [[(1, 1, 1.0, 1)], [(2, 2, 1.0, 0), (3, 3, 1.0, 2)], []]),  # 2-cycle, 1
        (None, [NAN], [[(1, 1, NAN, 0)]]),                            # no start wins over a NaN
        (0, [INF, 0.0], [[(1, 1, -INF, 1)], []]),                     # -inf is < 0.0
    ]


def test_known_answers():
    fsts = known()
    got = check(fsts, 1.0)
    assert F.last_launch_stats().engine == 15
    st = got.status.tolist()
    assert [i for i, s in enumerate(st) if s != OK] == [6, 7, 15] and st[6] == UNSUPPORTED
    ns = np.diff(got.state_offsets.astype(np.int64)).tolist()
    assert ns[0] == 3 and got.item(0) == (0, [INF, INF, 0.0], [[(1, 1, 1.0, 1)], [(3, 3, 0.0, 2)], []])
    assert got.item(2) == (0, [INF, 0.0], [[(1, 1, 1.0, 1)], []])     # the state stays
    assert ns[3] == ns[4] == ns[6] == ns[7] == ns[14] == 0
    assert got.start[3] == got.start[4] == got.start[6] == NO_STATE
    assert got.item(5) == (0, [INF, 0.0], [[(2, 2, 1.0, 1)], []])
    assert ns[8] == 3                                                 # best = -1, limit = 0
    for beam in (0.0, -0.0, INF):
        check(fsts, beam)
    assert check([fsts[8]], 0.5).item(0) == (0, [INF, -2.0], [[(1, 1, 1.0, 1)], []])
    # the zeros of either sign: beam -0.0 keeps every arc and both finals, bits copied
    z = check([fsts[9]], -0.0)
    assert bits(z.final_weights).tolist() == bits([INF, -0.0, 0.0]).tolist()
    assert bits(z.weights).tolist() == bits([-0.0, 0.0, -0.0]).tolist()
    # the loops: free ones stay at beam 0, the others need their weight as slack
    assert check([fsts[10], fsts[11]], 0.0).ilabels.tolist() == [1, 2, 2]
    assert check([fsts[10], fsts[11]], 1.0).ilabels.tolist() == [1, 2, 1, 2]
    assert check([fsts[12], fsts[13]], 0.0).ilabels.tolist() == [1, 2, 3, 1, 3]
    assert check([fsts[12], fsts[13]], 2.0).ilabels.tolist() == [1, 2, 3, 1, 2, 3]


def test_rounding_can_cut_the_start():
    big = 2.0 ** 53
    fst = (0, [INF, INF, INF, 0.0], [[(1, 1, big, 1)], [(2, 2, 1.0, 2)], [(3, 3, 1.0, 3)], []])
    got = check([fst, diamond()], 0.0)
    assert got.state_offsets.tolist() == [0, 0, 3] and got.start.tolist() == [NO_STATE, 0]
    assert check([fst], 2.0).ilabels.tolist() == [1, 2, 3]


# ---- 2. chunk edges ----------------------------------------------------------------------------

def path_with_branches(n, reverse=False):
    """A chain of n states, 0.5 per arc, the last state final; every third state has a skip arc
    that costs 1.0 more than the two arcs it skips, every fifth a parallel arc that costs 1.0
    more, every seventh an arc back (a cycle), every eleventh a dead-end state's worth of
    final weight that is 0.75 off the best.  reverse: the same with the ids reversed."""
    finals = [INF] * n
    finals[n - 1] = 0.0
    arcs = [[] for _ in range(n)]
    for s in range(n - 1):
        arcs[s].append((s % 250 + 1, 1, 0.5, s + 1))
        if s % 3 == 0 and s + 2 < n:
            arcs[s].append((300, 2, 2.0, s + 2))
        if s % 5 == 0:
            arcs[s].append((301, 3, 1.5, s + 1))
        if s % 7 == 3:
            arcs[s].append((302, 4, 0.25, s - 1))
        if s % 11 == 0:
            finals[s] = 0.5 * (n - 1 - s) + 0.75
    if not reverse:
        return 0, finals, arcs
    r = lambda s: n - 1 - s
    return (r(0), finals[::-1],
            [[(il, ol, w, r(t)) for il, ol, w, t in arcs[r(s)]] for s in range(n)])


EDGE_SIZES = (1, 63, 64, 65, 128, 129, 130, LDS - 1, LDS, LDS + 1)


@pytest.fixture(scope="module")
def edges():
    fsts = [path_with_branches(n) for n in EDGE_SIZES] + \
           [path_with_branches(n, True) for n in (65, 130, LDS + 1)]
    cache = [{} for _ in fsts]
    return fsts, {b: PM.prune_batch(fsts, b, cache) for b in BEAMS}


def test_chunk_edges(edges, monkeypatch, capfd):
    fsts, exp = edges
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    for beam in BEAMS:
        got = check(fsts, beam, exp[beam])
        items, wave, frontier, s_in, s_out, a_in, a_out = prune_line(capfd)
        assert (items, wave + frontier) == (len(fsts), len(fsts))
        assert s_in == sum(len(f[1]) for f in fsts) and s_out == int(got.state_offsets[-1])
        assert a_in == sum(len(a) for f in fsts for a in f[2]) and a_out == len(got.ilabels)
    # the beams cut differently: 0 leaves the chains, 0.5 nothing more, 1.5 everything alive
    n0, n1 = len(exp[0.0]["il"]), len(exp[1.5]["il"])
    assert sum(n - 1 for n in EDGE_SIZES) + 64 + 129 + LDS == n0 < n1 == len(exp[INF]["il"])
    monkeypatch.setenv("FSTAMD_PRUNE_SWEEPS", "1")      # the arcs back: the frontier tier
    check(fsts, 0.5, exp[0.5])
    assert prune_line(capfd)[2] >= 3
    monkeypatch.setenv("FSTAMD_PRUNE_SWEEPS", "0")      # every item with a start
    check(fsts, 1.5, exp[1.5])
    assert prune_line(capfd)[1:3] == (0, len(fsts))


# ---- 3. numbering against the sweep direction ------------------------------------------------------

def plain_chain(n, reverse):
    finals = [INF] * n
    arcs = [[] for _ in range(n)]
    if reverse:
        finals[0] = 0.0
        for s in range(1, n):
            arcs[s].append((1, 1, 1.0, s - 1))
            if s % 9 == 0 and s >= 2:
                arcs[s].append((2, 2, 3.0, s - 2))
        return n - 1, finals, arcs
    finals[n - 1] = 0.0
    for s in range(n - 1):
        arcs[s].append((1, 1, 1.0, s + 1))
        if s % 9 == 0 and s + 2 < n:
            arcs[s].append((2, 2, 3.0, s + 2))
    return 0, finals, arcs


def test_numbering_against_the_sweeps(monkeypatch, capfd):
    fwd, bwd = plain_chain(130, False), plain_chain(130, True)
    exp = {b: PM.prune_batch([fwd, bwd], b) for b in (0.0, 1.0)}
    assert len(exp[0.0]["il"]) == 2 * 129 < len(exp[1.0]["il"])
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    monkeypatch.setenv("FSTAMD_PRUNE_SWEEPS", "1")
    for beam in (0.0, 1.0):
        check([fwd, bwd], beam, exp[beam])
        # ids that rise along the arcs settle in one sweep each way; ids that fall do not
        assert prune_line(capfd)[:3] == (2, 1, 1)
    monkeypatch.delenv("FSTAMD_PRUNE_SWEEPS")
    for beam in (0.0, 1.0):
        check([fwd, bwd], beam, exp[beam])
        assert prune_line(capfd)[:3] == (2, 2, 0)       # three chunks: three sweeps suffice


# ---- 4. random sweep ---------------------------------------------------------------------------

def random_graph(rng, acyclic):
    n = int(rng.integers(1, 41))
    weights = (0.0, 0.5, 1.0, 2.0, 0.1, 0.3, INF)
    pw = (0.2, 0.2, 0.2, 0.15, 0.1, 0.1, 0.05)
    finals = [float(rng.choice((0.0, 0.5, 1.0, 0.1, -1.0))) if rng.random() < 0.25 else INF
              for _ in range(n)]
    arcs = []
    for s in range(n):
        al = []
        for _ in range(int(rng.integers(0, 5))):
            if acyclic:
                if s + 1 >= n:
                    break
                t = int(rng.integers(s + 1, min(n, s + 6)))
            else:
                t = int(rng.integers(0, n))
            al.append((int(rng.integers(1, 9)), int(rng.integers(0, 9)),
                       float(rng.choice(weights, p=pw)), t))
        arcs.append(al)
    start = None if rng.random() < 0.03 else int(rng.integers(0, n)) if not acyclic else 0
    return start, finals, arcs


@pytest.fixture(scope="module")
def graphs():
    rng = np.random.default_rng(150)
    fsts = [random_graph(rng, k % 2 == 0) for k in range(200)]
    cache = [{} for _ in fsts]
    return fsts, {b: PM.prune_batch(fsts, b, cache) for b in BEAMS}


def test_random_sweep(graphs, monkeypatch):
    fsts, exp = graphs
    kept = [int(exp[b]["state_offsets"][-1]) for b in BEAMS]
    assert 0 < kept[0] < kept[2] <= kept[3] < sum(len(f[1]) for f in fsts)
    for beam in BEAMS:
        check(fsts, beam, exp[beam])
    monkeypatch.setenv("FSTAMD_PRUNE_SWEEPS", "0")      # the same through the frontier tier
    for beam in (0.0, 1.5):
        check(fsts, beam, exp[beam])


# ---- 5. properties on real lattices ------------------------------------------------------------

def total(e):
    """The serial fold of a path's arc weights and its final weight (a got_item tuple)."""
    t = 0.0
    for x in np.array(e[3], np.uint64).view(np.float64).tolist():
        t += x
    return t + float(np.array([e[4]], np.uint64).view(np.float64)[0])


@pytest.fixture(scope="module")
def lattices():
    texts = SY.utterances(np.random.default_rng(15), 300, 4, 24)
    lat = F.compose_frozen_batch(load_blob(tagger_blob()), *SY.to_labels(texts))
    assert np.all(lat.status == OK)
    return lat


def test_best_path_survives_beam_zero(lattices):
    num = len(lattices)
    pruned = F.prune_lhs_batch(lattices.as_lhs(), 0.0)
    assert np.all(pruned.status == OK)
    assert 0 < int(pruned.state_offsets[-1]) < int(lattices.state_offsets[-1])
    a = F.shortest_path_lhs_batch(lattices.as_lhs())
    b = F.shortest_path_lhs_batch(pruned.as_lhs())
    assert a.status.tolist() == b.status.tolist() and np.all(a.status == OK)
    for i in range(num):
        assert bits([total(got_item(a, i))])[0] == bits([total(got_item(b, i))])[0], i


def test_nbest_of_the_pruned_batch(lattices):
    num, n, beam = len(lattices), 8, 0.5
    pruned = F.prune_lhs_batch(lattices.as_lhs(), beam)
    full = F.nbest_lhs_batch(lattices.as_lhs(), n)
    cut = F.nbest_lhs_batch(pruned.as_lhs(), n)
    some_cut = 0
    for i in range(num):
        a = [got_item(full, i * n + k) for k in range(n)]
        b = [got_item(cut, i * n + k) for k in range(n)]
        assert a[0][0] == OK
        limit = total(a[0]) + beam
        lead = [e for e in a if e[0] == OK and total(e) <= limit]
        assert b[:len(lead)] == lead, i
        some_cut += len(lead) < n
    assert some_cut > 0


def test_infinite_beam_is_connect(lattices, graphs):
    same_bytes(F.prune_lhs_batch(lattices.as_lhs(), INF), F.connect_lhs_batch(lattices.as_lhs()))
    # ... and on the random graphs without +inf arcs, negative or NaN weights
    fsts = [f for f in graphs[0]
            if all(0.0 <= a[2] < INF for al in f[2] for a in al)][:80]
    lhs = F.LhsBatch.from_fsts(fsts)
    same_bytes(F.prune_lhs_batch(lhs, INF), F.connect_lhs_batch(lhs))


# ---- 6. order independence ---------------------------------------------------------------------

def test_grid_and_shards_do_not_show(edges, graphs, monkeypatch):
    for fsts, exp in (edges, graphs):
        assert len(fsts) % 3
        lhs = F.LhsBatch.from_fsts(fsts)
        one = F.prune_lhs_batch(lhs, 0.5)
        PM.assert_batch_equal(one, exp[0.5])
        same_bytes(F.prune_lhs_batch(lhs, 0.5, devices=[0], shards=3), one)
        monkeypatch.setenv("FSTAMD_GRAPH_GRID", "1")               # every item in one workgroup
        same_bytes(F.prune_lhs_batch(lhs, 0.5), one)
        monkeypatch.setenv("FSTAMD_PRUNE_SWEEPS", "0")             # ... of the frontier tier too
        same_bytes(F.prune_lhs_batch(lhs, 0.5), one)
        monkeypatch.delenv("FSTAMD_PRUNE_SWEEPS")
        monkeypatch.delenv("FSTAMD_GRAPH_GRID")


# ---- 7. device entry ---------------------------------------------------------------------------

def run_device(d: DeviceLhs, beam, out: DeviceLattices):
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    needed = (C.c_uint64 * 2)(0, 0)
    rc = F.lib().fst_device_prune_lhs(C.byref(d.cs), beam, C.byref(opts), C.byref(out.desc),
                                      needed, None)
    assert rc == FF.FST_OK
    return int(needed[0]), int(needed[1])


def test_device_entry(graphs):
    fsts, exp = graphs
    lhs = F.LhsBatch.from_fsts(fsts)
    num, beam = len(fsts), 1.5
    host = F.prune_lhs_batch(lhs, beam)
    ns, na = int(host.state_offsets[-1]), int(host.arc_offsets[-1])
    d = DeviceLhs(lhs)

    def equal_host(out):
        got = out.arrays(ns, na)
        for name in ARRAYS:
            assert got[name].tobytes() == getattr(host, name).tobytes(), name

    ample = DeviceLattices(num, ns + 100, na + 100)
    assert run_device(d, beam, ample) == (ns, na)
    st = F.last_launch_stats()
    assert st.engine == 15 and st.launches >= 2 + 1 + 3      # prepare, prune, trim
    equal_host(ample)
    assert int(ample.fin.cpu()[ns]) == 77 and int(ample.il.cpu()[na]) == 77
    # one short in states, then in arcs: the pruned totals come back, nothing is written past a
    # capacity, and the second call with them succeeds
    for scap, acap in ((ns - 1, na), (ns, na - 1)):
        short = DeviceLattices(num, scap, acap)
        assert run_device(d, beam, short) == (ns, na)
        assert np.array_equal(short.status.cpu().numpy()[:num], host.status)
        assert int(short.fin.cpu()[scap - 1]) == 77 and int(short.il.cpu()[acap - 1]) == 77
        assert int(short.fin.cpu()[0]) == 77 and int(short.nx.cpu()[0]) == 77
    exact = DeviceLattices(num, ns, na)
    assert run_device(d, beam, exact) == (ns, na)
    equal_host(exact)


def test_device_entry_empty_batch():
    out = DeviceLattices(0, 4, 4)
    none = FF.FstLhsBatch(0, None, None, None, None, None, None, None, None)
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    needed = (C.c_uint64 * 2)(7, 7)
    assert F.lib().fst_device_prune_lhs(C.byref(none), 1.0, C.byref(opts), C.byref(out.desc),
                                        needed, None) == FF.FST_OK
    assert list(needed) == [0, 0] and F.last_launch_stats().engine == 15
    assert int(out.soff.cpu()[0]) == 0 and int(out.aoff.cpu()[0]) == 0
    assert int(out.aoff.cpu()[1]) == 77 and int(out.fin.cpu()[0]) == 77


def test_device_entry_validates_per_item(graphs):
    fsts = graphs[0][:60]
    lhs = F.LhsBatch.from_fsts(fsts)
    host = F.prune_lhs_batch(lhs, 1.5)
    ns = np.diff(host.state_offsets.astype(np.int64))
    victim = next(i for i in range(5, 60) if ns[i] > 1)
    bad = F.LhsBatch(lhs.state_offsets, lhs.start, lhs.final_weights, lhs.arc_offsets, lhs.ilabels,
                     lhs.olabels, lhs.weights, lhs.nextstates.copy())
    a0 = int(lhs.arc_offsets[int(lhs.state_offsets[victim])])
    bad.nextstates[a0] = len(fsts[victim][1])                 # one past the item's last state
    clean = [f for i, f in enumerate(fsts) if i != victim]
    exp = F.prune_lhs_batch(F.LhsBatch.from_fsts(clean), 1.5)
    out = DeviceLattices(60, int(host.state_offsets[-1]), int(host.arc_offsets[-1]))
    need = run_device(DeviceLhs(bad), 1.5, out)
    assert need == (int(exp.state_offsets[-1]), int(exp.arc_offsets[-1]))
    got = out.arrays(*need)
    assert got["status"].tolist() == (host.status[:victim].tolist() + [UNSUPPORTED] +
                                      host.status[victim + 1:].tolist())
    assert int(got["start"][victim]) == NO_STATE
    assert got["state_offsets"][victim] == got["state_offsets"][victim + 1]
    for name in ("final_weights", "arc_offsets", "ilabels", "olabels", "weights", "nextstates"):
        assert got[name].tobytes() == getattr(exp, name).tobytes(), name


def test_device_chain_into_unique_nbest_and_text(lattices):
    """lattices -> prune -> unique n-best -> text with nothing but the extents read by the host:
    the texts are those of the host entries on the host's pruned batch."""
    num, n, beam = 96, 4, 0.5
    sub = F.LhsBatch(lattices.state_offsets[:num + 1], lattices.start[:num],
                     lattices.final_weights, lattices.arc_offsets, lattices.ilabels,
                     lattices.olabels, lattices.weights, lattices.nextstates)
    host = F.prune_lhs_batch(sub, beam)
    ns, na = int(host.state_offsets[-1]), int(host.arc_offsets[-1])
    want = F.batch_result_to_text(F.nbest_unique_lhs_batch(host.as_lhs(), n))
    d = DeviceLhs(sub)
    out = DeviceLattices(num, ns, na)
    assert run_device(d, beam, out) == (ns, na)
    cs = out.as_device_lhs()
    paths = DeviceOut(num * n, n * ns)
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    assert F.lib().fst_device_nbest_unique_lhs(C.byref(cs), n, C.byref(opts), C.byref(paths.desc),
                                               None) == FF.FST_OK
    texts, status = emit_text(paths, num * n, 8 * n * max(na, 1) + 64)
    assert status == want.status.tolist()
    assert texts == want.texts()
    assert sum(s == OK for s in status) > num
    torch.cuda.synchronize()
