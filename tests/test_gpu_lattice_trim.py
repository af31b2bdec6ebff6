"""GPU: connect on the device -- FST_LATTICE_CONNECT on the three lattice entries and
fst_connect_lhs_batch -- against tests/connect_model.py, item by item, bit for bit.

The expected value of an item is connect_model applied to O.compose_csr(lhs, blob) (the compose
entries) or to the input itself (the stand-alone entry).  Every item of every batch is compared:
start, state count, final-weight bits, per-state arc ranges and the four arc arrays; the layout
as test_gpu_lattice_batch.assert_layout checks it.  The tests sit on what the trim adds: the
64-state chunks of its waves, the two tiers and their hand-over, the filtering gather, and that
nothing of it shows without the flag.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

import connect_model as CM
import libfst_amd as F
import libfst_amd.fst as FF
import oracle_ffi as O
from libfst_amd import synthetic as SY
from test_gpu_lattice_batch import (ARRAYS, DeviceLattices, assert_layout, chain_fst, check_chain,
                                    check_lhs, csr_of, dev_tensor, heap_tree, loop_rhs, oracle,
                                    projected, route_cols, same_bytes)
from test_gpu_lhs_batch import (assert_shards_do_not_show, batch_of, bits, expect, got_item,
                                item)
from test_gpu_parity import load_blob, random_rhs

pytestmark = pytest.mark.gpu

EAGER, LAZY = F.FST_SEM_EAGER, F.FST_SEM_LAZY
INF, NAN = math.inf, math.nan
OK, NO_STATE = F.FST_PATH_OK, F.FST_NO_STATE
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)


def assert_trimmed(got: F.LatticeBatch, i, t: CM.Trimmed, project=False):
    """Item i of the batch equals the model's connect, bit for bit."""
    assert int(got.status[i]) == OK, (i, int(got.status[i]))
    s0, s1 = int(got.state_offsets[i]), int(got.state_offsets[i + 1])
    assert s1 - s0 == len(t.finals), (i, s1 - s0, len(t.finals))
    assert int(got.start[i]) == t.start, (i, int(got.start[i]), t.start)
    assert np.array_equal(bits(got.final_weights[s0:s1]), bits(t.finals)), i
    ao = got.arc_offsets[s0:s1 + 1]
    a0, a1 = int(ao[0]), int(ao[-1])
    assert np.array_equal(ao - ao[0], t.off), i
    assert a1 - a0 == len(t.next), i
    assert np.array_equal(got.ilabels[a0:a1], t.ol if project else t.il), i
    assert np.array_equal(got.olabels[a0:a1], t.ol), i
    assert np.array_equal(bits(got.weights[a0:a1]), bits(t.w)), i
    assert np.array_equal(got.nextstates[a0:a1], t.next), i


def check_all(got, exp, project=False):
    assert len(got) == len(exp)
    assert_layout(got)
    for i, t in enumerate(exp):
        assert_trimmed(got, i, t, project)
    return got


def model_of(f: O.Fst) -> CM.Trimmed:
    return CM.connect_lists(*item(f))


def check_connect(fsts, exp=None, **kw):
    exp = exp if exp is not None else [model_of(f) for f in fsts]
    return check_all(F.connect_lhs_batch(batch_of(fsts), **kw), exp), exp


def check_lhs_connect(rhs, fsts, exp, project=False, **kw):
    return check_all(F.compose_frozen_lhs_batch(rhs, batch_of(fsts), project_output=project,
                                                connect=True, **kw), exp, project)


def check_chain_connect(rhs, seqs, exp, project=False, **kw):
    return check_all(F.compose_frozen_batch(rhs, *csr_of(seqs), project_output=project,
                                            connect=True, **kw), exp, project)


def trim_line(capfd):
    """The last `lattice trim:` route line: (items, sweep, linear, states in/out, arcs in/out)."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lattice trim:" in ln]
    assert lines, err
    m = re.search(r"lattice trim: items (\d+) \| sweep (\d+) linear (\d+) \| states (\d+) -> (\d+) "
                  r"arcs (\d+) -> (\d+)", lines[-1])
    assert m, lines[-1]
    return tuple(int(x) for x in m.groups())


# ---- 1. known answers --------------------------------------------------------------------------

def known_fsts():
    dead_end = O.Fst(start=0, finals=[INF, INF, 0.0, INF],          # connect.zig:133-142
                     arcs=[[(1, 1, 0.0, 1), (3, 3, 0.0, 3)], [(2, 2, 0.0, 2)], [], []])
    connected = O.Fst(start=0, finals=[INF, 0.0], arcs=[[(1, 1, 0.0, 1)], []])
    return [dead_end, connected, O.Fst()]


def test_known_answers_stand_alone():
    got, exp = check_connect(known_fsts())
    assert F.last_launch_stats().engine == 11
    assert got.state_offsets.tolist() == [0, 3, 5, 5]                # 4 -> 3, 2 -> 2, empty
    assert got.start.tolist() == [0, 0, NO_STATE]
    assert got.item(0) == (0, [INF, INF, 0.0], [[(1, 1, 0.0, 1)], [(2, 2, 0.0, 2)], []])
    assert got.item(1) == (0, [INF, 0.0], [[(1, 1, 0.0, 1)], []])


def test_known_answers_through_both_compose_entries():
    ident = O.Fst(start=0, finals=[0.0], arcs=[[(l, l, 0.0, 0) for l in (1, 2, 3)]])
    blob = O.freeze(ident)
    rhs = load_blob(blob)
    fsts = known_fsts()
    exp = [CM.connect_csr(oracle(f, blob)) for f in fsts]
    got = check_lhs_connect(rhs, fsts, exp)
    assert F.last_launch_stats().engine == 10
    assert got.state_offsets.tolist() == [0, 3, 5, 5] and got.start.tolist() == [0, 0, NO_STATE]
    # compose numbers the dead end 2 (BFS order); connect drops it and closes the gap
    assert got.item(0) == (0, [INF, INF, 0.0], [[(1, 1, 0.0, 1)], [(2, 2, 0.0, 2)], []])
    # the chain entry: a connected chain, the one-state acceptor, a chain the rhs rejects
    seqs = [[1, 2], [], [9], [1, 9]]
    exp = [CM.connect_csr(oracle(chain_fst(s), blob)) for s in seqs]
    got = check_chain_connect(rhs, seqs, exp)
    assert got.state_offsets.tolist() == [0, 3, 4, 4, 4]
    assert got.start.tolist() == [0, 0, NO_STATE, NO_STATE] and np.all(got.status == OK)


# ---- 2. chunk edges ----------------------------------------------------------------------------

def path_with_dead(n, dead):
    """States 0 .. n-1: the live ones form a chain in increasing id (the last is final, the
    first the start); each dead one hangs off the live state before it and loops on itself."""
    live = [s for s in range(n) if s not in dead]
    f = O.Fst(finals=[INF] * n, arcs=[[] for _ in range(n)])
    if not live:
        f.start = 0
        return f
    f.start = live[0]
    f.finals[live[-1]] = 0.5
    for a, b in zip(live, live[1:]):
        f.add_arc(a, 1 + a % 5, 1 + b % 7, float(a % 3), b)
    for d in sorted(dead):
        before = [s for s in live if s < d]
        f.add_arc(before[-1] if before else live[0], 9, 9, 1.25, d)
        f.add_arc(d, 8, 8, 0.75, d)
    return f


def edge_items(n):
    chunk_edges = {s for s in range(n) if s % 64 in (0, 63)}
    one_path = O.Fst(start=0, finals=[INF] * n, arcs=[[] for _ in range(n)])
    one_path.finals[n - 1] = -0.0
    for s in range(1, n):                                  # the start fans out to every state
        one_path.add_arc(0, 2, 3, 0.5, s)
    if n // 2 not in (0, n - 1):
        one_path.add_arc(n // 2, 4, 5, 1.5, n - 1)
    none_dead = path_with_dead(n, set())
    for s in range(0, n - 3, 3):
        none_dead.add_arc(s, 6, 6, 2.0, s + 3)
    start_dead = O.Fst(start=n - 1, finals=[INF] * n, arcs=[[] for _ in range(n)])
    if n > 1:
        start_dead.finals[0] = 0.0                          # final, but the start cannot reach it
    for s in range(n - 1):
        start_dead.add_arc(s, 1, 1, 0.0, s + 1)
    return [path_with_dead(n, chunk_edges), one_path, none_dead, start_dead]


@pytest.fixture(scope="module")
def edges():
    fsts = [f for n in SIZES for f in edge_items(n)]
    return fsts, [model_of(f) for f in fsts]


def test_chunk_edges(edges, monkeypatch, capfd):
    fsts, exp = edges
    kept = [len(t.finals) for t in exp]
    for k, n in enumerate(SIZES):
        dead = len([s for s in range(n) if s % 64 in (0, 63)])
        # dead states at chunk edges, one path, nothing dead, the start dead
        assert kept[4 * k:4 * k + 4] == [n - dead, len({0, n // 2, n - 1}) if n > 2 else n, n, 0]
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    got, _ = check_connect(fsts, exp=exp)
    items, sweep, linear, s_in, s_out, a_in, a_out = trim_line(capfd)
    assert (items, sweep, linear) == (len(fsts), len(fsts), 0)
    assert (s_in, s_out) == (sum(t.states_in for t in exp), sum(kept))
    assert (a_in, a_out) == (sum(t.arcs_in for t in exp), sum(len(t.next) for t in exp))
    monkeypatch.setenv("FSTAMD_TRIM_SWEEPS", "0")            # the same through the linear tier
    lin, _ = check_connect(fsts, exp=exp)
    items, sweep, linear = trim_line(capfd)[:3]
    assert (items, sweep, linear) == (len(fsts), 0, len(fsts))
    same_bytes(got, lin)
    monkeypatch.delenv("FSTAMD_TRIM_SWEEPS")
    back, _ = check_connect(fsts[::-1], exp=exp[::-1])       # another place in the batch
    assert back.item(1) == got.item(len(fsts) - 2)


# ---- 3. random sweep ---------------------------------------------------------------------------

def random_graph(rng):
    n = int(rng.integers(1, 201))
    f = O.Fst(finals=[INF] * n, arcs=[[] for _ in range(n)])
    odd_fin = [NAN, -0.0, -INF, 0.5, 0.0, 2.0]
    odd_w = [NAN, -0.0, INF, -INF, 1.5, 0.0, -2.0]
    for s in range(n):
        if rng.random() < 0.08:
            f.finals[s] = odd_fin[int(rng.integers(len(odd_fin)))]
    m = int(n * rng.choice([0.5, 1.0, 1.5, 3.0]))
    for _ in range(m):
        f.add_arc(int(rng.integers(n)), int(rng.integers(0, 5)), int(rng.integers(0, 5)),
                  odd_w[int(rng.integers(len(odd_w)))], int(rng.integers(n)))
    f.start = O.NO_STATE if rng.random() < 0.03 else int(rng.integers(n))
    return f


@pytest.fixture(scope="module")
def graphs():
    rng = np.random.default_rng(4242)
    calls = [[random_graph(rng) for _ in range(50)] for _ in range(4)]
    return calls, [[model_of(f) for f in fsts] for fsts in calls]


def test_random_sweep(graphs, monkeypatch):
    calls, exps = graphs
    assert sum(len(c) for c in calls) == 200
    trimmed = empty = whole = multi_final = cyc = 0
    for fsts, exp in zip(calls, exps):
        monkeypatch.delenv("FSTAMD_TRIM_SWEEPS", raising=False)
        base, _ = check_connect(fsts, exp=exp)
        for budget in ("1", "0"):
            monkeypatch.setenv("FSTAMD_TRIM_SWEEPS", budget)
            other, _ = check_connect(fsts, exp=exp)
            same_bytes(base, other)
        for f, t in zip(fsts, exp):
            trimmed += 0 < len(t.finals) < f.num_states
            empty += t.start == NO_STATE
            whole += len(t.finals) == f.num_states
            multi_final += int(np.sum(~np.isinf(t.finals))) > 1
            cyc += any(a[3] <= s for s, al in enumerate(f.arcs) for a in al)
    # what the sweep is meant to hold
    assert trimmed > 40 and empty > 20 and multi_final > 20 and cyc > 150 and whole >= 1


# ---- 4. the backwards-numbered chain -----------------------------------------------------------

def test_backwards_chain_goes_to_the_linear_tier(monkeypatch, capfd):
    n = 4096
    back = O.Fst(start=n - 1, finals=[INF] * n, arcs=[[] for _ in range(n)])
    back.finals[0] = 0.25
    for s in range(1, n):
        back.add_arc(s, 1 + s % 3, 2, float(s % 2), s - 1)
    back.add_arc(5, 7, 7, 1.0, 5)
    fwd = path_with_dead(n, {100, 4000})
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    got, exp = check_connect([back, fwd])
    assert [len(t.finals) for t in exp] == [n, n - 2]
    # each sweep settles one more 64-state chunk of the backwards chain: 64 sweeps, beyond
    # the budget; the forwards one settles in the first
    assert trim_line(capfd)[:3] == (2, 1, 1)
    assert int(got.start[0]) == n - 1 and int(got.start[1]) == 0


# ---- 5. compose + connect ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def verbalizer_case():
    ns, start, finals, arcs = SY.verbalizer()
    blob = O.freeze(O.Fst(start=start, finals=finals, arcs=arcs))
    texts = [t.replace("1", "#b").replace("2", "#z")
             for t in SY.utterances(np.random.default_rng(1), 300)][:64]
    seqs = [[ord(ch) + 1 for ch in t] for t in texts]
    full = [oracle(chain_fst(s), blob) for s in seqs]
    return blob, seqs, full, [CM.connect_csr(c) for c in full]


def test_verbalizer_dead_ends(verbalizer_case, monkeypatch, capfd):
    blob, seqs, full, exp = verbalizer_case
    # not vacuous, by the model alone: about half the states go, and whole items do
    states_in, states_out = sum(len(c.finals) for c in full), sum(len(t.finals) for t in exp)
    assert states_in == 995 and states_out == 524
    assert sum(t.start == NO_STATE for t in exp) == 38
    rhs = load_blob(blob)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    off_before, _ = check_chain(rhs, blob, seqs, exp=full)
    got = check_chain_connect(rhs, seqs, exp)
    items, sweep, linear, s_in, s_out, a_in, a_out = trim_line(capfd)
    assert (items, s_in, s_out) == (64, 995, 524) and sweep + linear == 64
    assert a_out == sum(len(t.next) for t in exp) == int(got.arc_offsets[-1])
    check_chain_connect(rhs, seqs, exp, project=True)
    fsts = [chain_fst(s) for s in seqs]
    check_lhs_connect(rhs, fsts, exp)
    check_lhs_connect(rhs, fsts, exp, project=True)
    # flag off after flag on: the untouched path, byte for byte
    off_after, _ = check_chain(rhs, blob, seqs, exp=full)
    same_bytes(off_before, off_after)


@pytest.fixture(scope="module")
def forty():
    """An rhs with cycles and input epsilons; lhs with cycles and dead parts."""
    rng = np.random.default_rng(23)
    rhs_fst = random_rhs(rng, 9, 50, 3, eps=True)
    assert any(a[0] == 0 for al in rhs_fst.arcs for a in al)
    assert any(a[3] <= s for s, al in enumerate(rhs_fst.arcs) for a in al)
    blob = O.freeze(rhs_fst)
    fsts = [random_rhs(rng, int(rng.integers(1, 9)), int(rng.integers(1, 25)), 3, eps=True)
            for _ in range(40)]
    seqs = [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, 14)))] for _ in range(40)]
    full = [oracle(f, blob) for f in fsts]
    full_chain = [oracle(chain_fst(s), blob) for s in seqs]
    return (blob, fsts, seqs, full, full_chain, [CM.connect_csr(c) for c in full],
            [CM.connect_csr(c) for c in full_chain])


def test_cyclic_rhs_with_input_epsilon(forty):
    blob, fsts, seqs, full, full_chain, exp, exp_chain = forty
    rhs = load_blob(blob)
    assert sum(0 < len(t.finals) < t.states_in for t in exp + exp_chain) > 10
    before, _ = check_lhs(rhs, blob, fsts, exp=full)
    before_chain, _ = check_chain(rhs, blob, seqs, exp=full_chain)
    for project in (False, True):
        check_lhs_connect(rhs, fsts, exp, project=project)
        check_chain_connect(rhs, seqs, exp_chain, project=project)
    after, _ = check_lhs(rhs, blob, fsts, exp=full)
    after_chain, _ = check_chain(rhs, blob, seqs, exp=full_chain)
    same_bytes(before, after)
    same_bytes(before_chain, after_chain)


@pytest.fixture(scope="module")
def tier_case():
    rng = np.random.default_rng(5)
    blob = O.freeze(loop_rhs())
    sizes = (128, 129, 256, 257, 16384, 16385)
    fsts = [heap_tree(N, rng) for N in sizes]
    full = [oracle(f, blob) for f in fsts]
    return blob, fsts, sizes, full, [CM.connect_csr(c) for c in full]


def test_items_of_every_bfs_tier(tier_case, monkeypatch, capfd):
    blob, fsts, sizes, full, exp = tier_case
    # a heap-ordered 8-ary tree whose last state alone is final: one root-to-leaf path stays
    assert [t.states_in for t in exp] == list(sizes)
    assert [len(t.finals) for t in exp] == [4, 4, 4, 4, 6, 6]
    rhs = load_blob(blob)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    for project in (False, True):
        check_lhs_connect(rhs, fsts, exp, project=project)
        items, cols, _ = route_cols(capfd)
        assert items == 6 and cols == [6, 5, 3, 1]                # LDS 128, LDS 256, tier 0, 1+
    st = F.last_launch_stats()
    assert st.engine == 10 and st.launches == 2 * 4 + 2            # + the sweep and the map
    monkeypatch.setenv("FSTAMD_TRIM_SWEEPS", "0")
    check_lhs_connect(rhs, fsts, exp)
    assert F.last_launch_stats().launches == 2 * 4 + 3             # + the linear tier
    monkeypatch.delenv("FSTAMD_TRIM_SWEEPS")
    check_lhs(rhs, blob, fsts, exp=full)                           # flag off: untrimmed
    assert F.last_launch_stats().launches == 2 * 4


# ---- 6. order independence and growth ----------------------------------------------------------

def test_grid_arena_and_shards_do_not_show(forty, graphs, monkeypatch):
    blob, fsts, seqs, _, _, exp, exp_chain = forty
    rhs = load_blob(blob)
    alone_fsts, alone_exp = graphs[0][0], graphs[1][0]
    plain = check_lhs_connect(rhs, fsts, exp)
    plain_chain = check_chain_connect(rhs, seqs, exp_chain)
    plain_alone, _ = check_connect(alone_fsts, exp=alone_exp)
    monkeypatch.setenv("FSTAMD_GRAPH_GRID", "2")                   # many items per workgroup
    same_bytes(plain, check_lhs_connect(rhs, fsts, exp))
    same_bytes(plain_chain, check_chain_connect(rhs, seqs, exp_chain))
    same_bytes(plain_alone, check_connect(alone_fsts, exp=alone_exp)[0])
    monkeypatch.setenv("FSTAMD_TRIM_SWEEPS", "0")                  # ... of the linear tier too
    same_bytes(plain, check_lhs_connect(rhs, fsts, exp))
    same_bytes(plain_alone, check_connect(alone_fsts, exp=alone_exp)[0])
    monkeypatch.delenv("FSTAMD_TRIM_SWEEPS")
    monkeypatch.delenv("FSTAMD_GRAPH_GRID")
    monkeypatch.setenv("FSTAMD_LATTICE_ARENA", "8,8")              # forced reruns
    same_bytes(plain, check_lhs_connect(rhs, fsts, exp))
    same_bytes(plain_chain, check_chain_connect(rhs, seqs, exp_chain))
    monkeypatch.delenv("FSTAMD_LATTICE_ARENA")
    same_bytes(plain, check_lhs_connect(rhs, fsts, exp, devices=[0], shards=3))
    same_bytes(plain_chain, check_chain_connect(rhs, seqs, exp_chain, devices=[0], shards=3))
    same_bytes(plain_alone, check_connect(alone_fsts, exp=alone_exp, devices=[0], shards=3)[0])


def test_shards_do_not_show_on_the_edge_batch():
    fsts = SY.edge_networks()
    lhs = F.LhsBatch.from_fsts(fsts)
    one = assert_shards_do_not_show(lambda **kw: F.connect_lhs_batch(lhs, **kw))
    assert one.status.tolist() == [F.FST_PATH_OK] * 48
    ns = np.diff(one.state_offsets.astype(np.int64)).tolist()
    assert ns[13] == 0 and ns[21] == 1 and ns[29] == len(fsts[29][1]) - 1   # (29: the dead end)
    assert ns[:5] == [len(f[1]) for f in fsts[:5]]


# ---- 7. device entry ---------------------------------------------------------------------------

def run_device(rhs, d_lab, d_off, num, max_len, out: DeviceLattices, flags):
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    needed = (C.c_uint64 * 2)(0, 0)
    rc = F.lib().fst_device_compose_frozen(rhs.h, d_lab.data_ptr(), d_off.data_ptr(), num,
                                           max_len, flags, C.byref(opts), C.byref(out.desc),
                                           needed, None)
    assert rc == FF.FST_OK
    return int(needed[0]), int(needed[1])


def test_device_entry_reports_trimmed_totals(verbalizer_case):
    blob, seqs, full, exp = verbalizer_case
    rhs = load_blob(blob)
    num = len(seqs)
    labels, offsets = csr_of(seqs)
    flags = FF.FST_LATTICE_CONNECT | FF.FST_LATTICE_PROJECT_OUTPUT
    host = check_chain_connect(rhs, seqs, exp, project=True)
    ns, na = sum(len(t.finals) for t in exp), sum(len(t.next) for t in exp)
    assert (ns, na) == (int(host.state_offsets[-1]), int(host.arc_offsets[-1]))
    d_lab, d_off = dev_tensor(labels), dev_tensor(offsets)
    max_len = max(len(s) for s in seqs)

    def equal_host(out):
        got = out.arrays(ns, na)
        for name in ARRAYS:
            assert got[name].tobytes() == getattr(host, name).tobytes(), name

    ample = DeviceLattices(num, ns + 100, na + 100)
    assert run_device(rhs, d_lab, d_off, num, max_len, ample, flags) == (ns, na)
    assert F.last_launch_stats().engine == 10
    equal_host(ample)
    assert int(ample.fin.cpu()[ns]) == 77 and int(ample.il.cpu()[na]) == 77
    # one short in states, then in arcs: the trimmed totals come back, nothing is written past a
    # capacity, and the second call with them succeeds
    for scap, acap in ((ns - 1, na), (ns, na - 1)):
        short = DeviceLattices(num, scap, acap)
        assert run_device(rhs, d_lab, d_off, num, max_len, short, flags) == (ns, na)
        assert np.array_equal(short.status.cpu().numpy()[:num], host.status)
        assert int(short.fin.cpu()[scap - 1]) == 77 and int(short.il.cpu()[acap - 1]) == 77
        assert int(short.fin.cpu()[0]) == 77 and int(short.nx.cpu()[0]) == 77
    exact = DeviceLattices(num, ns, na)
    assert run_device(rhs, d_lab, d_off, num, max_len, exact, flags) == (ns, na)
    equal_host(exact)
    # without the flag the same call needs the untrimmed totals
    loose = DeviceLattices(num, 995, sum(len(c.arcs) for c in full))
    assert run_device(rhs, d_lab, d_off, num, max_len, loose, 0) == (995, loose.acap)


# ---- 8. cascade --------------------------------------------------------------------------------

def cascade_stages():
    """test_gpu_lattice_batch.cascade_stages with dead ends in stage 1: label 5 may also go to
    state 2 (no way out), 7 and 8 to state 3 (a loop that is never final).  Weights are
    positive or +0.0, so no signed zero reaches a sum."""
    r1 = O.Fst(start=0, finals=[0.0, INF, INF, INF],
               arcs=[[(5, 10, 1.0, 0), (5, 11, 2.0, 0), (6, 0, 0.5, 1), (7, 13, 0.5, 0),
                      (5, 14, 0.75, 2), (7, 15, 1.5, 3), (8, 16, 1.0, 3)],
                     [(0, 12, 0.25, 0)], [], [(5, 16, 0.5, 3), (8, 16, 0.25, 3)]])
    r2 = O.Fst(start=0, finals=[0.125],
               arcs=[[(10, 20, 5.0, 0), (11, 21, 0.0, 0), (12, 22, 1.0, 0), (13, 0, 0.5, 0),
                      (13, 23, 2.0, 0), (14, 24, 0.25, 0), (16, 26, 0.5, 0)]])
    return r1, r2


def fst_of(t: CM.Trimmed, project) -> O.Fst:
    f = O.Fst(start=t.start if len(t.finals) else O.NO_STATE, finals=t.finals.tolist(),
              arcs=[[] for _ in range(len(t.finals))])
    for s in range(len(t.finals)):
        for k in range(int(t.off[s]), int(t.off[s + 1])):
            ol = int(t.ol[k])
            f.arcs[s].append((ol if project else int(t.il[k]), ol, float(t.w[k]), int(t.next[k])))
    return f


def total(e):
    """The serial fold of a path's arc weights and its final weight (a got_item tuple)."""
    t = 0.0
    for x in np.array(e[3], np.uint64).view(np.float64).tolist():
        t += x
    return t + float(np.array([e[4]], np.uint64).view(np.float64)[0])


def test_cascade_on_trimmed_lattices():
    rng = np.random.default_rng(31)
    r1, r2 = cascade_stages()
    b1, b2 = O.freeze(r1), O.freeze(r2)
    rhs1, rhs2 = load_blob(b1), load_blob(b2)
    seqs = [[5], [8], [7, 8]] + [[int(x) for x in rng.integers(5, 9, int(rng.integers(1, 9)))]
                                 for _ in range(21)]
    full = [oracle(chain_fst(s), b1) for s in seqs]
    trim = [CM.connect_csr(c) for c in full]
    assert sum(len(t.finals) for t in trim) < sum(len(c.finals) for c in full)
    assert trim[1].start == NO_STATE and any(0 < len(t.finals) < t.states_in for t in trim)
    lat_full = F.compose_frozen_batch(rhs1, *csr_of(seqs), project_output=True)
    lat_trim = check_chain_connect(rhs1, seqs, trim, project=True)
    mids_full = []
    for s in seqs:
        rc, lat = O.compose(chain_fst(s), b1)
        assert rc == O.OR_OK
        mids_full.append(projected(lat))
    mids_trim = [fst_of(t, True) for t in trim]
    ok = 0
    for sem in (LAZY, EAGER):
        got_full = F.compose_frozen_shortest_path_lhs_batch(rhs2, lat_full.as_lhs(), 1, sem)
        got_trim = F.compose_frozen_shortest_path_lhs_batch(rhs2, lat_trim.as_lhs(), 1, sem)
        for i in range(len(seqs)):
            a, b = got_item(got_full, i), got_item(got_trim, i)
            assert a == expect(mids_full[i], b2, sem), (i, sem)    # each run against the oracle
            assert b == expect(mids_trim[i], b2, sem), (i, sem)    # on the item it was given
            assert a[0] == b[0], (i, sem)                          # the same status ...
            if a[0] == OK:                                         # ... and total weight
                assert bits([total(a)])[0] == bits([total(b)])[0], (i, sem)
                ok += 1
    assert ok >= 20
