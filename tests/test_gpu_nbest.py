"""fst_nbest_lhs_batch / fst_device_nbest_lhs on the GPU against tests/nbest_model.py, string by
string: status, length, ilabels, olabels and the bits of every arc weight and final weight.
The model is the definition (include/fst_batch.h); tests/test_nbest_model.py checks it against
the declarative form on the CPU.  Both tiers run everything: the LDS tier by default, the HBM
tier with FSTAMD_NBEST_LDS=0 (no item fits a budget of no bytes)."""
import ctypes as C
import math
import random
import re

import numpy as np
import pytest
import torch

import libfst_amd as F
import libfst_amd.fst as FF
import nbest_model as M
from libfst_amd import synthetic as SY
from test_gpu_lattice_batch import DeviceLattices, dev_tensor
from test_gpu_lattice_sp import emit_text, tagger_blob
from test_gpu_lhs_batch import bits, got_item
from test_gpu_lhs_device import DeviceLhs, DeviceOut
from test_gpu_parity import load_blob

pytestmark = pytest.mark.gpu

OK, EMPTY, UNSUPPORTED, FULL = (F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED,
                                F.FST_PATH_OUTPUT_FULL)
I = math.inf
TIERS = ("lds", "hbm")


def set_tier(monkeypatch, tier):
    if tier == "hbm":
        monkeypatch.setenv("FSTAMD_NBEST_LDS", "0")
    else:
        monkeypatch.delenv("FSTAMD_NBEST_LDS", raising=False)


def expect(item, n):
    """The n strings of one item as got_item gives them, from the model."""
    start, finals, arcs = item
    res = M.nbest(start, finals, arcs, n)
    if not isinstance(res, list):
        return [(res,)] * n
    flat = [a for lst in arcs for a in lst]
    out = []
    for seq, t in res:
        out.append((OK, [flat[a][0] for a in seq], [flat[a][1] for a in seq],
                    bits([flat[a][2] for a in seq]).tolist(), int(bits([finals[t]])[0])))
    return out + [(EMPTY,)] * (n - len(res))


def strings_of(got, count):
    return [got_item(got, i) for i in range(count)]


def check(items, n, exp=None, **kw):
    got = F.nbest_lhs_batch(F.LhsBatch.from_fsts(items), n, **kw)
    assert len(got.status) == len(items) * n and int(got.offsets[0]) == 0
    exp = exp if exp is not None else [expect(it, n) for it in items]
    have = strings_of(got, len(items) * n)
    for i, e in enumerate(exp):
        assert have[i * n:(i + 1) * n] == e, (i, n, items[i] if len(items[i][1]) < 12 else "...")
    return got


def nb_line(capfd):
    """(items, lds, hbm) of the last route line."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lattice nbest:" in ln]
    assert lines, err
    m = re.search(r"lattice nbest: items (\d+) \| lds (\d+) hbm (\d+) \| [\d.]+ ms", lines[-1])
    return tuple(int(x) for x in m.groups())


# ---- 1. known answers ----------------------------------------------------------------------------

@pytest.mark.parametrize("tier", TIERS)
def test_known_answers(tier, monkeypatch):
    set_tier(monkeypatch, tier)
    items = [k[1] for k in M.KNOWN]
    for n in (1, 2, 3, 16):
        got = check(items, n)
        have = strings_of(got, len(items) * n)
        for i, (name, item, answers) in enumerate(M.KNOWN):   # the answers written by hand
            if n not in answers:
                continue
            want = answers[n]
            mine = have[i * n:(i + 1) * n]
            if not isinstance(want, list):
                assert mine == [(want,)] * n, name
                continue
            flat = [a for lst in item[2] for a in lst]
            assert [s[0] for s in mine] == [OK] * len(want) + [EMPTY] * (n - len(want)), name
            for s, (seq, t) in zip(mine, want):
                assert s[1] == [flat[a][0] for a in seq], name
                assert s[4] == int(bits([item[1][t]])[0]), name
    assert F.last_launch_stats().engine == 13


def test_status_order():
    """No start before a NaN before a cycle; the neighbours are not touched."""
    plain = M.KNOWN[0][1]
    nan = math.nan
    items = [plain,
             (None, [nan, 0.0], [[(1, 1, nan, 0)], []]),        # no start, NaN, self-loop: EMPTY
             plain,
             (0, [I, nan], [[(1, 1, 1.0, 0)], []]),             # NaN and a self-loop
             (0, [I, 0.0], [[(1, 1, 1.0, 1)], [(1, 1, I, 0)]]),  # a cycle through an arc of +inf
             (None, [], []),                                     # zero states
             plain]
    got = check(items, 3)
    st = got.status.reshape(-1, 3).tolist()
    assert st[1] == [EMPTY] * 3 and st[3] == [UNSUPPORTED] * 3 and st[4] == [UNSUPPORTED] * 3
    assert st[5] == [EMPTY] * 3 and st[0] == st[2] == st[6] == [OK, OK, EMPTY]


# ---- 2. shapes where the kernel can go wrong -----------------------------------------------------

SIZES = (1, 2, 63, 64, 65, 128, 129, 257)


def chain(S, falling):
    """S states, S - 1 arcs, depth S - 1, one path."""
    sid = (lambda s: S - 1 - s) if falling else (lambda s: s)
    arcs = [[] for _ in range(S)]
    finals = [I] * S
    for s in range(S - 1):
        arcs[sid(s)].append((1 + s % 7, 2 + s % 5, 0.1 * (s % 9), sid(s + 1)))
    finals[sid(S - 1)] = 0.25
    return sid(0), finals, arcs


def ladder(S):
    """Falling ids, arcs to the next and the next but one: many paths, ties among them."""
    sid = lambda s: S - 1 - s
    arcs = [[] for _ in range(S)]
    finals = [I] * S
    for s in range(S - 1):
        arcs[sid(s)].append((1, 1 + s % 3, 1.0, sid(s + 1)))
        if s + 2 < S:
            arcs[sid(s)].append((2, 2, 2.0 if s % 4 else 1.5, sid(s + 2)))
    finals[sid(S - 1)] = 0.0
    if S > 2:
        finals[sid(S - 2)] = 0.5
    return sid(0), finals, arcs


def sausage(slots, alts):
    """`slots` slots of `alts` parallel arcs: alts ** slots paths, the cap n binds everywhere."""
    S = slots + 1
    arcs = [[(1 + k, 1 + k, [0.5, 0.25, 0.5][k % 3] + 0.125 * (s % 2), s + 1) for k in range(alts)]
            for s in range(slots)] + [[]]
    return 0, [I] * slots + [0.0], arcs


def fan(deg):
    """A state of out-degree `deg`, then one of in-degree `deg` (ids fall into it)."""
    S = deg + 2
    hub, sink = S - 1, 0
    arcs = [[] for _ in range(S)]
    for k in range(deg):
        mid = 1 + k
        arcs[hub].append((1 + k % 5, 1, 0.25 * (k % 7), mid))
        arcs[mid].append((2, 1 + k % 3, 0.5 * (k % 3), sink))
    return hub, [0.0] + [I] * (S - 1), arcs


def lds_need(S, A, n):
    """The LDS an item's tables take (kernels/lattice_nbest.hpp): 16 B per list entry, five
    words per state, two per arc."""
    return 16 * n * S + 4 * (5 * S + 2 * A)


def lds_budget(n):
    return 4096 + 1024 * n


def budget_pair(n):
    """Two items about the LDS budget at n: the first's tables are the largest that fit (one
    more arc would not), the second has that one arc more."""
    B = lds_budget(n)
    S = (B - 1024) // (16 * n + 28)
    A = (B - 16 * n * S - 20 * S) // 8
    assert A >= S - 1 and lds_need(S, A, n) <= B < lds_need(S, A + 1, n)
    out = []
    for extra in (A - (S - 1), A + 1 - (S - 1)):
        start, finals, arcs = chain(S, False)
        arcs[0] += [(3, 3, 0.5 + 0.25 * (k % 4), 1) for k in range(extra)]
        out.append((start, finals, arcs))
    return out


def shape_items(n):
    items = []
    for S in SIZES:
        items += [chain(S, False), chain(S, True), ladder(S)]
    items += [sausage(40, 3), fan(70)]
    return items + budget_pair(n)


@pytest.fixture(scope="module")
def shapes():
    """items and the model's answer per n, computed once."""
    return {n: (shape_items(n), [expect(it, n) for it in shape_items(n)]) for n in (1, 3, 16)}


@pytest.mark.parametrize("n", (1, 3, 16))
@pytest.mark.parametrize("tier", TIERS)
def test_shapes(shapes, n, tier, monkeypatch, capfd):
    set_tier(monkeypatch, tier)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    items, exp = shapes[n]
    assert exp[3 * SIZES.index(257)][0][0] == OK and len(exp[3 * SIZES.index(257)][0][1]) == 256
    assert all(s[0] == OK for s in exp[len(SIZES) * 3])        # the sausage fills every rank
    got = check(items, n, exp=exp)
    count, lds, hbm = nb_line(capfd)
    assert count == len(items) == lds + hbm
    if tier == "hbm":
        assert lds == 0
    else:
        fits = sum(lds_need(len(it[1]), sum(len(a) for a in it[2]), n) <= lds_budget(n)
                   for it in items)
        assert (lds, hbm) == (fits, len(items) - fits) and lds > 0 and hbm > 0
    assert got.status.reshape(-1, n)[:, 0].tolist().count(OK) == len(items)


@pytest.mark.parametrize("n", (1, 3, 16))
def test_lds_budget_edge(shapes, n, monkeypatch, capfd):
    """The item one arc over the budget takes the HBM tier, the one just under it the LDS tier."""
    monkeypatch.delenv("FSTAMD_NBEST_LDS", raising=False)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    items, exp = shapes[n]
    under, over = items[-2:]
    check([under], n, exp=exp[-2:-1])
    assert nb_line(capfd) == (1, 1, 0)
    check([over], n, exp=exp[-1:])
    assert nb_line(capfd) == (1, 0, 1)
    check([under, over], n, exp=exp[-2:])
    assert nb_line(capfd) == (2, 1, 1)
    # the switch moves the budget: with the item's own need it fits again
    S, A = len(over[1]), sum(len(a) for a in over[2])
    monkeypatch.setenv("FSTAMD_NBEST_LDS", str(lds_need(S, A, n) + 15))
    check([under, over], n, exp=exp[-2:])
    assert nb_line(capfd) == (2, 2, 0)


# ---- 3. random sweep -----------------------------------------------------------------------------

def sweep_items():
    rng = random.Random(77)
    items = [M.random_item(rng, 40) for _ in range(300)]
    nan = math.nan
    odd = [(0, [I, nan, 0.0], [[(1, 1, 1.0, 1)], [(1, 1, 1.0, 2)], []]),        # a NaN final
           (0, [I, 0.0], [[(1, 1, nan, 1)], []]),                              # a NaN arc
           (0, [I, I, 0.0], [[(1, 1, 1.0, 1)], [(1, 1, 1.0, 0), (1, 1, 1.0, 2)], []]),  # a cycle
           (2, [0.0, I, I], [[], [(1, 1, 1.0, 2)], [(1, 1, 1.0, 1), (2, 2, 1.0, 0)]]),  # a cycle
           (None, [0.0], [[]]),                                                # no start
           (None, [], [])]                                                     # no states
    for k, it in enumerate(odd * 3):
        items.insert(1 + 17 * k, it)
    return items


@pytest.fixture(scope="module")
def sweep():
    items = sweep_items()
    return items, {n: [expect(it, n) for it in items] for n in (1, 2, 5, 16)}


@pytest.mark.parametrize("n", (1, 2, 5, 16))
@pytest.mark.parametrize("tier", TIERS)
def test_random_sweep(sweep, n, tier, monkeypatch):
    set_tier(monkeypatch, tier)
    items, exp = sweep
    got = check(items, n, exp=exp[n])
    first = got.status.reshape(-1, n)[:, 0].tolist()
    assert first.count(UNSUPPORTED) == 12 and first.count(EMPTY) >= 6 and first.count(OK) > 150
    if n == 16:                                   # items with fewer than n paths are common
        assert got.status.tolist().count(EMPTY) > len(items)


# ---- 4. agreement with the shortest path entry ---------------------------------------------------

def total_of(got, i):
    """The left fold of string i, as the contract writes it."""
    g = 0.0
    for w in got.weights[int(got.offsets[i]):int(got.offsets[i + 1])].tolist():
        g = g + w
    return g + float(got.finals[i])


def test_agrees_with_shortest_path_lhs_batch():
    """On weights >= +0 the best path's total is the shortest path's, as an f64 value.  The
    paths themselves may differ on ties: the two entries break them by different rules."""
    rng = random.Random(5)
    items = []
    while len(items) < 200:
        it = M.random_item(rng, 24)
        ws = [a[2] for lst in it[2] for a in lst]
        if all(w >= 0.0 and w != I and not math.copysign(1.0, w) < 0 for w in ws):
            items.append(it)
    cyclic = (0, [I, 0.0], [[(1, 1, 1.0, 1)], [(1, 1, 1.0, 0)]])
    items.append(cyclic)
    lhs = F.LhsBatch.from_fsts(items)
    sp = F.shortest_path_lhs_batch(lhs)
    one = F.nbest_lhs_batch(lhs, 1)
    four = F.nbest_lhs_batch(lhs, 4)
    ok = 0
    for i in range(len(items) - 1):
        assert int(one.status[i]) == int(sp.status[i]) == int(four.status[4 * i]), i
        if int(sp.status[i]) == OK:
            ok += 1
            assert total_of(one, i) == total_of(sp, i) == total_of(four, 4 * i), i
    assert ok > 100
    assert int(one.status[-1]) == UNSUPPORTED and int(sp.status[-1]) == OK    # the cyclic item


# ---- 5. end to end -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def utterances():
    texts = SY.utterances(np.random.default_rng(3), 256)
    rhs = load_blob(tagger_blob())
    labels, offsets = SY.to_labels(texts)
    lat = F.compose_frozen_batch(rhs, labels, offsets, project_output=True, connect=True)
    assert np.all(lat.status == OK)
    items = [lat.item(i) for i in range(len(lat))]
    return rhs, texts, labels, offsets, lat, [expect(it, 4) for it in items]


def test_end_to_end(utterances):
    rhs, texts, labels, offsets, lat, exp = utterances
    num, n = len(texts), 4
    got = F.nbest_lhs_batch(lat.as_lhs(), n)
    assert F.last_launch_stats().engine == 13
    assert strings_of(got, num * n) == [s for e in exp for s in e]
    text = F.batch_result_to_text(got)
    assert len(text.status) == num * n and len(text.texts()) == num * n
    eager = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, F.FST_SEM_EAGER)
    etext = F.batch_result_to_text(eager)
    alternatives = 0
    for i in range(num):
        if int(eager.status[i]) != OK:
            assert int(got.status[i * n]) == EMPTY, i
            continue
        assert float(text.total_weight[i * n]) == float(etext.total_weight[i]), i
        alternatives += int(np.sum(got.status[i * n:(i + 1) * n] == OK))
    assert alternatives > 2 * num                 # the lattices do hold more than one reading


# ---- 6. device entry -----------------------------------------------------------------------------

def run_device_nbest(cs, num, n, cap):
    out = DeviceOut(num * n, cap)
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    rc = F.lib().fst_device_nbest_lhs(C.byref(cs), n, C.byref(opts), C.byref(out.desc), None)
    assert rc == FF.FST_OK
    return out


def test_device_entry(utterances):
    rhs, texts, labels, offsets, host_lat, exp = utterances
    num, n = len(texts), 4
    host = F.nbest_lhs_batch(host_lat.as_lhs(), n)
    host_items = strings_of(host, num * n)
    host_texts = F.batch_result_to_text(host).texts()
    ns, na = int(host_lat.state_offsets[-1]), int(host_lat.arc_offsets[-1])
    lat = DeviceLattices(num, ns, na)                          # chains -> lattices on the device
    needed = (C.c_uint64 * 2)(0, 0)
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    d_lab, d_off = dev_tensor(labels), dev_tensor(offsets)
    flags = FF.FST_LATTICE_PROJECT_OUTPUT | FF.FST_LATTICE_CONNECT
    rc = F.lib().fst_device_compose_frozen(rhs.h, d_lab.data_ptr(), d_off.data_ptr(), num,
                                           max(len(t) for t in texts), flags, C.byref(opts),
                                           C.byref(lat.desc), needed, None)
    assert rc == FF.FST_OK and (int(needed[0]), int(needed[1])) == (ns, na)
    cs = lat.as_device_lhs()
    paths = run_device_nbest(cs, num, n, n * ns)               # n * states always suffice
    assert F.last_launch_stats().engine == 13
    assert paths.items() == host_items
    need = sum(len(e[1]) for e in host_items if e[0] == OK)
    assert paths.cursor() == need == int(host.offsets[-1])
    got_texts, text_status = emit_text(paths, num * n, 8 * n * na + 64)
    assert got_texts == host_texts and text_status == [e[0] for e in host_items]
    # an arena one arc short: the strings that do not fit say so, the cursor says what is needed
    short = run_device_nbest(cs, num, n, need - 1)
    st = short.status.cpu().numpy()[:num * n].tolist()
    assert short.cursor() == need and FULL in st
    for i, e in enumerate(short.items()):
        assert e == host_items[i] or e == (FULL,), i
    exact = run_device_nbest(cs, num, n, short.cursor())
    assert exact.items() == host_items


def test_device_entry_validates_per_item(sweep):
    items, exp = sweep
    items, exp = items[:60], exp[5][:60]
    lhs = F.LhsBatch.from_fsts(items)
    victim = next(i for i, it in enumerate(items) if any(it[2]) and exp[i][0][0] == OK)
    bad = F.LhsBatch(lhs.state_offsets, lhs.start, lhs.final_weights, lhs.arc_offsets, lhs.ilabels,
                     lhs.olabels, lhs.weights, lhs.nextstates.copy())
    a0 = int(lhs.arc_offsets[int(lhs.state_offsets[victim])])
    bad.nextstates[a0] = len(items[victim][1])                 # one past the item's last state
    d = DeviceLhs(bad)
    out = run_device_nbest(d.cs, len(items), 5, 5 * int(lhs.state_offsets[-1]))
    have = out.items()
    for i, e in enumerate(exp):
        assert have[5 * i:5 * i + 5] == ([(UNSUPPORTED,)] * 5 if i == victim else e), i


# ---- 7. sharding ---------------------------------------------------------------------------------

def test_shards_do_not_show(sweep):
    items, exp = sweep
    items = items[:100]
    assert len(items) % 3
    lhs = F.LhsBatch.from_fsts(items)
    one = F.nbest_lhs_batch(lhs, 5)
    assert strings_of(one, 500) == [s for e in exp[5][:100] for s in e]
    for shards in (2, 3):
        got = F.nbest_lhs_batch(lhs, 5, devices=[0], shards=shards)
        for name in ("status", "offsets", "ilabels", "olabels", "weights", "finals"):
            assert getattr(got, name).tobytes() == getattr(one, name).tobytes(), (name, shards)
