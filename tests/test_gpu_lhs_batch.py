"""GPU: the batch entry for general lhs FSTs (lattices, confusion networks, n-best unions)
against the CPU oracle, item by item, bit for bit.

Expected values: lazy = O.compose_shortest_path(lhs, blob, n); eager =
O.shortest_path(O.compose(lhs, blob), n).  Statuses, labels and weight bit patterns are
compared as tests/test_gpu_parity.py::check does.  The tests sit on what the batch adds to
the single-lhs kernels: the per-item descriptor, table reuse across a wave's consecutive
items, the shared arena cursor and the tier hand-over lists.
"""
import math
import re

import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
from libfst_amd import synthetic as SY
from test_gpu_parity import load_blob, random_rhs, to_product

pytestmark = pytest.mark.gpu

EAGER, LAZY = F.FST_SEM_EAGER, F.FST_SEM_LAZY
SEMS = [LAZY, EAGER]
INF = math.inf


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def item(f: O.Fst):
    return (None if f.start == O.NO_STATE else f.start, f.finals, f.arcs)


def batch_of(fsts) -> F.LhsBatch:
    return F.LhsBatch.from_fsts([item(f) for f in fsts])


def expect(lhs: O.Fst, blob: bytes, sem, n=1):
    """(status, ilabels, olabels, weight bits, final bits) of one item, from the oracle."""
    if sem == LAZY:
        rc, ref = O.compose_shortest_path(lhs, blob, n)
    else:
        rc, lat = O.compose(lhs, blob)
        assert rc == O.OR_OK
        rc, ref = O.shortest_path(lat, n)
    if rc == O.OR_ERR_UNSUPPORTED_N:
        return (F.FST_PATH_ERROR_N,)
    if rc == O.OR_ERR_CYCLE:
        return (F.FST_PATH_CYCLE,)
    assert rc == O.OR_OK, rc
    ch = O.chain(ref)
    if ch is None:
        return (F.FST_PATH_EMPTY,)
    il, ol, w, fin = ch
    return (F.FST_PATH_OK, il, ol, bits(w).tolist(), int(bits([fin])[0]))


def got_item(got, i):
    st = int(got.status[i])
    a0, a1 = int(got.offsets[i]), int(got.offsets[i + 1])
    if st != F.FST_PATH_OK:
        assert a0 == a1, i
        return (st,)
    return (st, got.ilabels[a0:a1].tolist(), got.olabels[a0:a1].tolist(),
            bits(got.weights[a0:a1]).tolist(), int(bits(got.finals[i:i + 1])[0]))


def check(rhs, blob, fsts, sem, n=1, exp=None, skip=(), **kw):
    got = F.compose_frozen_shortest_path_lhs_batch(rhs, batch_of(fsts), n, sem, **kw)
    assert len(got.status) == len(fsts) and int(got.offsets[0]) == 0
    exp = exp if exp is not None else [None if i in skip else expect(f, blob, sem, n)
                                       for i, f in enumerate(fsts)]
    for i, e in enumerate(exp):
        if e is not None:
            assert got_item(got, i) == e, (i, sem, n)
    return got, exp


def same_result(a, b):
    return all(np.array_equal(x, y) for x, y in (
        (a.status, b.status), (a.offsets, b.offsets), (a.ilabels, b.ilabels),
        (a.olabels, b.olabels), (bits(a.weights), bits(b.weights)),
        (bits(a.finals), bits(b.finals))))


def route_line(capfd):
    """The last `lhs batch:` route line of the captured stderr as (sem, items, columns)."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lhs batch:" in ln]
    assert lines, err
    m = re.search(r"lhs batch: (\w+) items (\d+) \| (.*) \| replay (\d+)", lines[-1])
    cols = m.group(3).split()
    return (m.group(1), int(m.group(2)),
            {cols[i]: int(cols[i + 1]) for i in range(0, len(cols), 2)}, int(m.group(4)), lines)


# ---- 1. known answers --------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_known_answers_through_both_entries(sem):
    a1 = O.compile_string(b"123")                              # compose-shortest-path.zig:447-471
    a2 = O.compile_string_transducer(b"abcde", b"xy")          # epsilon outputs
    for rhs_fst, answers in ((O.compile_string_transducer(b"123", b"abc"), (b"abc", None)),
                             (O.compile_string_transducer(b"xy", b"uvw"), (None, b"uvw"))):
        blob = O.freeze(rhs_fst)
        rhs = load_blob(blob)
        got, exp = check(rhs, blob, [a1, a2], sem)
        via_handles = F.compose_frozen_shortest_path_handles_batch(
            rhs, [to_product(a1), to_product(a2)], 1, sem)
        assert same_result(got, via_handles)
        texts = F.batch_result_to_text(got).texts()
        for i, ans in enumerate(answers):
            if ans is None:
                assert exp[i] == (F.FST_PATH_EMPTY,)
            else:
                assert exp[i][0] == F.FST_PATH_OK and texts[i] == ans


# ---- 2. degenerate items -------------------------------------------------------------------

def degenerate_items():
    no_states = O.Fst()
    no_start = O.Fst(finals=[0.0, INF], arcs=[[(1, 1, 0.0, 1)], []])
    lone_final = O.Fst(start=0, finals=[0.5], arcs=[[]])
    never_final = O.Fst(start=0, finals=[INF, INF], arcs=[[(1, 1, 0.0, 1)], [(1, 1, 1.0, 0)]])
    plain = O.Fst(start=0, finals=[INF, 0.25], arcs=[[(1, 2, 0.5, 1)], []])
    return [no_states, no_start, lone_final, never_final, plain]


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("rhs_start_final", [True, False])
def test_degenerate_items(sem, rhs_start_final):
    r = O.Fst(start=0, finals=[1.5 if rhs_start_final else INF, 0.0],
              arcs=[[(1, 1, 0.25, 1), (2, 3, 0.0, 1)], [(1, 1, 0.0, 1)]])
    blob = O.freeze(r)
    rhs = load_blob(blob)
    fsts = degenerate_items()
    for n in (0, 1, 2):
        got, exp = check(rhs, blob, fsts, sem, n=n)
        # EMPTY wins over ERROR_N: no start (or no state at all) is EMPTY for every n
        assert exp[0] == exp[1] == (F.FST_PATH_EMPTY,)
        if n == 0:
            assert all(e == (F.FST_PATH_EMPTY,) for e in exp)
        if n == 2:
            assert [e[0] for e in exp[2:]] == [F.FST_PATH_ERROR_N] * 3
        if n == 1:
            assert exp[2][0] == (F.FST_PATH_OK if rhs_start_final else F.FST_PATH_EMPTY)
            assert exp[3] == (F.FST_PATH_EMPTY,)
    # an rhs without a start: EMPTY whatever n
    empty_blob = O.freeze(O.Fst())
    for n in (1, 2):
        check(load_blob(empty_blob), empty_blob, fsts, sem, n=n,
              exp=[(F.FST_PATH_EMPTY,)] * len(fsts))


# ---- 3. random graphs ------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(10))
def test_random_graphs(seed):
    rng = np.random.default_rng(7000 + seed)
    frac = seed % 2 == 1
    rhs_fst = random_rhs(rng, int(rng.integers(1, 20)), int(rng.integers(1, 80)), 3, eps=True,
                         frac=frac)
    blob = O.freeze(rhs_fst)
    rhs = load_blob(blob)
    fsts = [random_rhs(rng, int(rng.integers(1, 11)), int(rng.integers(1, 31)), 3, eps=True,
                       frac=frac) for _ in range(64)]
    for sem in SEMS:
        check(rhs, blob, fsts, sem)


# ---- 4. out-degree boundaries ------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_out_degree_boundaries(sem):
    rng = np.random.default_rng(41)
    rhs_fst = random_rhs(rng, 6, 40, 4, eps=True)
    blob = O.freeze(rhs_fst)
    rhs = load_blob(blob)
    fsts = []
    for deg in (1, 63, 64, 65, 130):
        f = O.Fst(start=0, finals=[INF, 0.0, 1.0, INF], arcs=[[], [], [], []])
        for k in range(deg):  # a third of the arcs output epsilon
            ol = 0 if k % 3 == 1 else int(rng.integers(1, 5))
            f.add_arc(0, int(rng.integers(0, 5)), ol, float(rng.integers(0, 4)),
                      int(rng.integers(1, 4)))
        f.add_arc(3, 1, 2, 1.0, 1)
        f.add_arc(2, 0, 0, 0.0, 3)
        fsts.append(f)
        fsts.append(O.Fst(start=0, finals=[INF, 0.0], arcs=[[(1, int(rng.integers(1, 5)), 0.5, 1)], []]))
    check(rhs, blob, fsts, sem)


# ---- 5. tier boundaries --------------------------------------------------------------------------

def ladder_rhs():
    return O.Fst(start=0, finals=[0.125], arcs=[[(1, 1, 0.5, 0), (2, 3, 0.25, 0)]])


def ladder(K, rng):
    """A K-position lhs with two arcs per position: K + 1 product tuples, 2 K arcs and
    K + 1 BFS levels against ladder_rhs()."""
    f = O.Fst(start=0, finals=[INF] * K + [0.75], arcs=[[] for _ in range(K + 1)])
    w = rng.integers(0, 4, size=(K, 2))
    for k in range(K):
        f.arcs[k] = [(1, 1, float(w[k, 0]), k + 1), (2, 2, float(w[k, 1]), k + 1)]
    return f


@pytest.fixture(scope="module")
def tier_case():
    rng = np.random.default_rng(5)
    blob = O.freeze(ladder_rhs())
    # 81 tuples / 160 arcs (the 128-tuple LDS size holds 176 arcs), 151 (the 256-tuple size),
    # 1,001 (tier 0: 16 K tuples), 20,001 (tier 1)
    fsts = [ladder(K, rng) for K in (80, 150, 1000, 20000, 3, 80)]
    return blob, load_blob(blob), fsts, {}


def test_eager_tier_boundaries(tier_case, monkeypatch, capfd):
    blob, rhs, fsts, _ = tier_case
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    check(rhs, blob, fsts, EAGER)
    sem, items, cols, replay, _ = route_line(capfd)
    assert (sem, items, replay) == ("eager", 6, 0)
    assert cols == {"tiny128": 6, "tiny256": 3, "tier0": 2, "tier1+": 1}


def test_lazy_tier_boundaries(tier_case, monkeypatch, capfd):
    blob, rhs, fsts, _ = tier_case
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    rng = np.random.default_rng(6)
    fsts = fsts[:3] + [ladder(1023, rng), ladder(1024, rng), ladder(2000, rng)]
    check(rhs, blob, fsts, LAZY)   # 1,024 tuples fill the first tier's tables, 1,025 do not
    sem, items, cols, _, _ = route_line(capfd)
    assert (sem, items) == ("lazy", 6)
    assert cols["t1k"] == 6 and cols["t16k"] == 2 and cols["t256k"] == 0


# ---- 6. many items per wave ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def many_small():
    rng = np.random.default_rng(77)
    rhs_fst = random_rhs(rng, 8, 30, 3, eps=True)
    blob = O.freeze(rhs_fst)
    fsts = [random_rhs(rng, int(rng.integers(1, 6)), int(rng.integers(1, 9)), 3, eps=True)
            for _ in range(3000)]
    return blob, load_blob(blob), fsts, {}


@pytest.mark.parametrize("sem", SEMS)
def test_many_items_per_wave(many_small, sem, monkeypatch):
    blob, rhs, fsts, cache = many_small
    free, exp = check(rhs, blob, fsts, sem)
    cache[sem] = exp
    monkeypatch.setenv("FSTAMD_GRAPH_GRID", "2")
    capped, _ = check(rhs, blob, fsts, sem, exp=exp)
    assert F.last_launch_stats().grid <= 2
    # path order in the arena differs with the grid; the CSR result does not
    assert same_result(free, capped)


# ---- 7. weights ------------------------------------------------------------------------------------

def weighted_dag(rng, weights, finals):
    """A small acyclic lhs (arcs go forward) over labels 0..3 with the given weights."""
    ns = 6
    f = O.Fst(start=0, finals=[INF] * ns, arcs=[[] for _ in range(ns)])
    for s in range(ns - 1):
        for _ in range(int(rng.integers(1, 4))):
            f.add_arc(s, int(rng.integers(0, 4)), int(rng.integers(0, 4)),
                      weights[int(rng.integers(len(weights)))], int(rng.integers(s + 1, ns)))
    f.finals[ns - 1] = finals[0]
    f.finals[ns - 2] = finals[1]
    return f


@pytest.mark.parametrize("sem", SEMS)
def test_non_dyadic_weights_and_finals(sem):
    rng = np.random.default_rng(91)
    blob = O.freeze(random_rhs(rng, 7, 45, 3, eps=True, frac=True))
    fsts = [weighted_dag(rng, [0.1, 1.0 / 3.0, math.log(3.0)], [0.7, math.log(2.0)])
            for _ in range(48)]
    _, exp = check(load_blob(blob), blob, fsts, sem)
    assert sum(e[0] == F.FST_PATH_OK for e in exp) >= 8


@pytest.mark.parametrize("sem", SEMS)
def test_mixed_weight_routes(sem, monkeypatch, capfd):
    rng = np.random.default_rng(92)
    blob = O.freeze(random_rhs(rng, 7, 45, 3, eps=True))
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    fsts, nan_items, replay_items = [], [], 0
    for i in range(40):
        kind = i % 4
        if kind == 0:
            f = weighted_dag(rng, [0.0, 1.0, 2.5], [0.0, 1.0])
        elif kind == 1:
            f = weighted_dag(rng, [-1.0, 0.5, 2.0, -0.0], [-0.5, 0.0])
            replay_items += 1
        elif kind == 2:
            f = weighted_dag(rng, [INF, 0.0, 1.0], [0.0, 0.5])
            replay_items += int(any(a[2] == INF for al in f.arcs for a in al))
        else:
            f = weighted_dag(rng, [math.nan, 1.0], [0.0, 0.0])
            if any(math.isnan(a[2]) for al in f.arcs for a in al):
                nan_items.append(i)
            else:
                f.finals[5] = math.nan
                nan_items.append(i)
            # NaN has no place in the reference's order: the entry reports UNSUPPORTED
        fsts.append(f)
    got, _ = check(load_blob(blob), blob, fsts, sem, skip=set(nan_items))
    assert [int(got.status[i]) for i in nan_items] == [F.FST_PATH_UNSUPPORTED] * len(nan_items)
    _, _, _, replay, _ = route_line(capfd)
    if sem == EAGER:  # the heap-replay list: every item with a negative, -0.0 or +inf weight
        nan_replay = sum(1 for i in nan_items
                         if any(a[2] < 0 or a[2] == INF for al in fsts[i].arcs for a in al))
        assert replay == replay_items + nan_replay


# ---- 8. chain-shaped items -----------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_chain_items_equal_the_chain_batch(sem):
    rng = np.random.default_rng(17)
    spec = SY.tagger()
    r = O.Fst(start=spec[1], finals=spec[2], arcs=spec[3])
    blob = O.freeze(r)
    rhs = load_blob(blob)
    texts = [t.encode() for t in SY.utterances(rng, 12, 0, 20)] + [b""]
    fsts, chains = [], {}
    for i, t in enumerate(texts):
        chains[len(fsts)] = i
        fsts.append(O.compile_string(t))
        cn = SY.confusion_network(rng, t.decode(), 3, 0.2)
        fsts.append(O.Fst(start=cn[0], finals=cn[1], arcs=cn[2]))
    got, _ = check(rhs, blob, fsts, sem)
    labels, offsets = SY.to_labels([t.decode() for t in texts])
    ref = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem)
    for j, i in chains.items():
        assert int(got.status[j]) == int(ref.status[i])
        a0, a1 = int(got.offsets[j]), int(got.offsets[j + 1])
        b0, b1 = int(ref.offsets[i]), int(ref.offsets[i + 1])
        assert np.array_equal(got.ilabels[a0:a1], ref.ilabels[b0:b1])
        assert np.array_equal(got.olabels[a0:a1], ref.olabels[b0:b1])
        assert np.array_equal(bits(got.weights[a0:a1]), bits(ref.weights[b0:b1]))
        if int(ref.status[i]) == F.FST_PATH_OK:
            assert bits(got.finals[j:j + 1])[0] == bits(ref.finals[i:i + 1])[0]


# ---- 9 / 10. arena growth, shards ------------------------------------------------------------------

@pytest.fixture(scope="module")
def forty():
    rng = np.random.default_rng(23)
    spec = SY.tagger()
    blob = O.freeze(O.Fst(start=spec[1], finals=spec[2], arcs=spec[3]))
    fsts = []
    for t in SY.utterances(rng, 40, 1, 24):
        cn = SY.confusion_network(rng, t, 3, 0.15)
        fsts.append(O.Fst(start=cn[0], finals=cn[1], arcs=cn[2]))
    return blob, load_blob(blob), fsts, {}


@pytest.mark.parametrize("sem", SEMS)
def test_arena_growth(forty, sem, monkeypatch):
    blob, rhs, fsts, cache = forty
    plain, exp = check(rhs, blob, fsts, sem)
    cache[sem] = exp
    assert int(plain.offsets[-1]) > 8 * 4      # the first arena (8 arcs) and its x4 are too small
    monkeypatch.setenv("FSTAMD_ARENA_ARCS", "8")
    grown, _ = check(rhs, blob, fsts, sem, exp=exp)
    assert same_result(plain, grown)


@pytest.mark.parametrize("sem", SEMS)
def test_three_shards_equal_one(forty, sem):
    blob, rhs, fsts, cache = forty
    one, exp = check(rhs, blob, fsts, sem, exp=cache.get(sem))
    three, _ = check(rhs, blob, fsts, sem, exp=exp, devices=[0], shards=3)
    assert same_result(one, three)
    for name in ("status", "offsets", "ilabels", "olabels", "weights", "finals"):
        assert getattr(one, name).tobytes() == getattr(three, name).tobytes(), name


def assert_shards_do_not_show(call):
    """`call(**kw)` is one entry on SY.edge_networks(): 2 and 3 shards on one GPU return the
    one-shard call's arrays, byte for byte.  Returns the one-shard result."""
    one = call()
    arrays = {k: v for k, v in vars(one).items() if isinstance(v, np.ndarray)}
    assert len(arrays) >= 4 and len(one.status) == 48
    for shards in (2, 3):
        got = call(devices=[0], shards=shards)
        for name, a in arrays.items():
            assert getattr(got, name).tobytes() == a.tobytes(), (name, shards)
    return one


def tagger_rhs():
    return SY.to_mutable(SY.tagger()).freeze()


@pytest.mark.parametrize("sem", SEMS)
def test_shards_do_not_show_on_the_edge_batch(sem):
    rhs, fsts = tagger_rhs(), SY.edge_networks()
    lhs = F.LhsBatch.from_fsts(fsts)
    one = assert_shards_do_not_show(
        lambda **kw: F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, 1, sem, **kw))
    st = one.status.tolist()
    assert st[9] == F.FST_PATH_UNSUPPORTED and st[13] == F.FST_PATH_EMPTY   # the NaN, no states
    assert st.count(F.FST_PATH_OK) >= 44
    handles = []
    for start, finals, arcs in fsts:
        m = F.MutableFst()
        for _ in finals:
            m.add_state()
        if start is not None:
            m.set_start(start)
        for s, fw in enumerate(finals):
            if fw != INF:
                m.set_final(s, fw)
        for s, state_arcs in enumerate(arcs):
            for a in state_arcs:
                m.add_arc(s, *a)
        handles.append(m)
    via_handles = assert_shards_do_not_show(
        lambda **kw: F.compose_frozen_shortest_path_handles_batch(rhs, handles, 1, sem, **kw))
    assert same_result(one, via_handles)


# ---- 11. route --------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_route_of_a_large_batch(many_small, sem, monkeypatch, capfd):
    blob, rhs, fsts, cache = many_small
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    exp = cache.get(sem)
    check(rhs, blob, fsts[:2000], sem, exp=exp[:2000] if exp else None)
    st = F.last_launch_stats()
    name, items, cols, replay, lines = route_line(capfd)
    assert len(lines) == 1                       # one line per call
    assert (name, items) == ("lazy" if sem == LAZY else "eager", 2000)
    assert st.engine == (8 if sem == LAZY else 9)
    assert st.grid > 1                           # the items run side by side
    first = "t1k" if sem == LAZY else "tiny128"
    assert cols[first] == 2000
    # launches: one kernel per tier an item list entered, plus one hand-over list kernel
    # (the fixed helper) per tier -- read from the route line, whatever the tiers were
    tiers_used = sum(1 for v in cols.values() if v > 0)
    assert 1 <= st.launches <= 2 * tiers_used
