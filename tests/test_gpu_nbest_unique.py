"""fst_nbest_unique_lhs_batch / fst_device_nbest_unique_lhs on the GPU against
tests/nbest_unique_model.py, string by string: status, length, ilabels, olabels and the bits of
every arc weight and final weight.  The model is the definition (include/fst_batch.h);
tests/test_nbest_unique_model.py checks it against the declarative form on the CPU.  Both tiers
run everything: the LDS tier (with the largest budget where the shapes need it) and the HBM tier
with FSTAMD_NBEST_LDS=0 (no item fits a budget of no bytes)."""
import ctypes as C
import math
import random
import re

import numpy as np
import pytest

import libfst_amd as F
import libfst_amd.fst as FF
import nbest_model as M
import nbest_unique_model as U
from libfst_amd import synthetic as SY
from test_gpu_lattice_sp import emit_text, tagger_blob, verbalizer_blob
from test_gpu_lhs_batch import bits, got_item
from test_gpu_lhs_device import DeviceLhs, DeviceOut
from test_gpu_parity import load_blob

pytestmark = pytest.mark.gpu

OK, EMPTY, UNSUPPORTED, FULL = (F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED,
                                F.FST_PATH_OUTPUT_FULL)
I = math.inf
TIERS = ("lds", "hbm")
ARRAYS = ("status", "offsets", "ilabels", "olabels", "weights", "finals")


def set_tier(monkeypatch, tier, lds_bytes=None):
    """lds_bytes: the LDS tier's budget where the default (4 KiB + n KiB) holds too little."""
    if tier == "hbm":
        monkeypatch.setenv("FSTAMD_NBEST_LDS", "0")
    elif lds_bytes is not None:
        monkeypatch.setenv("FSTAMD_NBEST_LDS", str(lds_bytes))
    else:
        monkeypatch.delenv("FSTAMD_NBEST_LDS", raising=False)


def expect(item, n, model=U.nbest_unique):
    """The n strings of one item as got_item gives them, from the model."""
    start, finals, arcs = item
    res = model(start, finals, arcs, n)
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
    got = F.nbest_unique_lhs_batch(F.LhsBatch.from_fsts(items), n, **kw)
    assert len(got.status) == len(items) * n and int(got.offsets[0]) == 0
    exp = exp if exp is not None else [expect(it, n) for it in items]
    have = strings_of(got, len(items) * n)
    for i, e in enumerate(exp):
        assert have[i * n:(i + 1) * n] == e, (i, n, items[i] if len(items[i][1]) < 12 else "...")
    return got


def same_bytes(a, b, what):
    for name in ARRAYS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (name, what)


def route_line(capfd):
    """(items, lds, hbm) of the last route line of the unique entry."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lattice nbest-unique:" in ln]
    assert lines, err
    assert not any("lattice nbest:" in ln for ln in err.split("\n"))
    m = re.search(r"lattice nbest-unique: items (\d+) \| lds (\d+) hbm (\d+) \| [\d.]+ ms",
                  lines[-1])
    return tuple(int(x) for x in m.groups())


# ---- 1. known answers ----------------------------------------------------------------------------

@pytest.mark.parametrize("tier", TIERS)
def test_known_answers(tier, monkeypatch):
    set_tier(monkeypatch, tier)
    known = U.KNOWN_UNIQUE + M.KNOWN          # the plain entry's statuses and order hold too
    items = [k[1] for k in known]
    for n in (1, 2, 3, 16):
        got = check(items, n)
        have = strings_of(got, len(items) * n)
        for i, (name, item, answers) in enumerate(U.KNOWN_UNIQUE):   # the answers written by hand
            if n not in answers:
                continue
            want = answers[n]
            mine = have[i * n:(i + 1) * n]
            flat = [a for lst in item[2] for a in lst]
            assert [s[0] for s in mine] == [OK] * len(want) + [EMPTY] * (n - len(want)), name
            for s, (seq, t) in zip(mine, want):
                assert s[1] == [flat[a][0] for a in seq], name
                assert s[2] == [flat[a][1] for a in seq], name
                assert s[4] == int(bits([item[1][t]])[0]), name
        for i, (name, item, answers) in enumerate(M.KNOWN, start=len(U.KNOWN_UNIQUE)):
            if n in answers and not isinstance(answers[n], list):
                assert have[i * n:(i + 1) * n] == [(answers[n],)] * n, name
    assert F.last_launch_stats().engine == 14


# ---- 2. random items -----------------------------------------------------------------------------

NS = (1, 2, 3, 5, 16)


def sweep_items():
    rng = random.Random(1414)
    items = [U.random_item_dup(rng, 24) for _ in range(300)]
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
    return items, {n: [expect(it, n) for it in items] for n in NS}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("tier", TIERS)
def test_random_sweep(sweep, n, tier, monkeypatch):
    set_tier(monkeypatch, tier)
    items, exp = sweep
    got = check(items, n, exp=exp[n])
    first = got.status.reshape(-1, n)[:, 0].tolist()
    assert first.count(UNSUPPORTED) == 12 and first.count(EMPTY) >= 6 and first.count(OK) > 150
    if n > 1:     # the rule does remove paths here: the plain answer differs on many items
        plain = [expect(it, n, model=M.nbest) for it in items]
        assert sum(p != e for p, e in zip(plain, exp[n])) > 60


@pytest.mark.parametrize("tier", TIERS)
def test_hash_masks_do_not_show(sweep, tier, monkeypatch):
    """With mask 0 every comparison of two texts is decided by the walk, with F unequal texts
    collide often: the result is the default mask's, byte for byte."""
    set_tier(monkeypatch, tier)
    items, exp = sweep
    monkeypatch.delenv("FSTAMD_NBEST_HASH_MASK", raising=False)
    default = {n: check(items, n, exp=exp[n]) for n in (5, 16)}
    for mask in ("0", "F"):
        monkeypatch.setenv("FSTAMD_NBEST_HASH_MASK", mask)
        for n in (5, 16):
            same_bytes(check(items, n, exp=exp[n]), default[n], (mask, n))


# ---- 3. the engine, and the plain entry where the two must agree -------------------------------

def test_engine_and_agreement_with_the_plain_entry(sweep):
    items, exp = sweep
    lhs = F.LhsBatch.from_fsts(items)
    one = F.nbest_unique_lhs_batch(lhs, 1)
    assert F.last_launch_stats().engine == 14
    same_bytes(one, F.nbest_lhs_batch(lhs, 1), "n = 1")
    assert F.last_launch_stats().engine == 13
    # prefix trees: every complete path prints another text, nothing is removed
    rng = np.random.default_rng(8)
    unions = [SY.nbest_union(rng, SY.utterances(rng, 6, 3, 12)) for _ in range(64)]
    ulhs = F.LhsBatch.from_fsts(unions)
    four = F.nbest_unique_lhs_batch(ulhs, 4)
    same_bytes(four, F.nbest_lhs_batch(ulhs, 4), "nbest_union, n = 4")
    assert four.status.tolist().count(OK) == 4 * 64


# ---- 4. ladders: one text over 2^k paths, walks of the whole depth ---------------------------------

LADDERS = (1, 63, 64, 65, 255, 256, 257)


def ladder(S, falling, first_differs):
    """S states in a chain, two arcs per rung with the same olabel (an epsilon on every fourth
    rung), equal weights on every third: 2^(S-1) paths that print one text.  first_differs: the
    second arc of the first rung prints another label, so there are two texts and the walk that
    tells them apart runs back to the start."""
    sid = (lambda s: S - 1 - s) if falling else (lambda s: s)
    arcs = [[] for _ in range(S)]
    finals = [I] * S
    for s in range(S - 1):
        ol = s % 4
        arcs[sid(s)].append((1, ol, 1.0, sid(s + 1)))
        arcs[sid(s)].append((2, 9 if first_differs and s == 0 else ol, 1.0 + 0.25 * (s % 3),
                             sid(s + 1)))
    finals[sid(S - 1)] = 0.25
    return sid(0), finals, arcs


def ladder_items():
    return [ladder(S, falling, differs) for S in LADDERS for falling in (False, True)
            for differs in (False, True)]


@pytest.fixture(scope="module")
def ladders():
    items = ladder_items()
    return items, {n: [expect(it, n) for it in items] for n in (2, 16)}


@pytest.mark.parametrize("n", (2, 16))
@pytest.mark.parametrize("tier", TIERS)
def test_ladders(ladders, n, tier, monkeypatch, capfd):
    set_tier(monkeypatch, tier, lds_bytes=61440)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    items, exp = ladders
    got = check(items, n, exp=exp[n])
    count, lds, hbm = route_line(capfd)
    assert count == len(items) == lds + hbm
    if tier == "hbm":
        assert lds == 0
    else:
        fits = sum(lds_need(len(it[1]), sum(len(a) for a in it[2]), n) <= 61440 for it in items)
        assert (lds, hbm) == (fits, len(items) - fits) and lds > 0
    st = got.status.reshape(-1, n).tolist()
    k = 0
    for S in LADDERS:
        for falling in (False, True):
            for differs in (False, True):
                texts = 1 if S == 1 or not differs else 2
                assert st[k] == [OK] * texts + [EMPTY] * (n - texts), (S, falling, differs)
                assert len(exp[n][k][0][1]) == S - 1
                k += 1


# ---- 5. many finals --------------------------------------------------------------------------------

def many_finals():
    """A hub into 70 mids into one sink (in-degree 70, three texts among the 70 prefixes), the
    sink into 64 final states by epsilons and into one more by a label: six texts in all, and
    the selection passes over 62 * 3 winners of a text it has chosen."""
    mids, fins = 70, 64
    sink = 1 + mids
    S = sink + 1 + fins + 1
    arcs = [[] for _ in range(S)]
    finals = [I] * S
    for k in range(mids):
        arcs[0].append((1 + k % 5, 5, 0.25 * (k % 7), 1 + k))
        arcs[1 + k].append((2, 1 + k % 3, 0.5 * (k % 3), sink))
    for j in range(fins):
        arcs[sink].append((3, 0, 0.125 * (j % 5), sink + 1 + j))
        finals[sink + 1 + j] = 0.25 * (j % 2)
    arcs[sink].append((3, 7, 0.0, S - 1))
    finals[S - 1] = 4.0
    return 0, finals, arcs


@pytest.mark.parametrize("tier", TIERS)
def test_many_finals(tier, monkeypatch):
    set_tier(monkeypatch, tier, lds_bytes=61440)
    item = many_finals()
    for n in (1, 4, 16):
        exp = expect(item, n)
        assert [s[0] for s in exp] == [OK] * min(n, 6) + [EMPTY] * (n - min(n, 6))
        check([item, item], n, exp=[exp, exp])


# ---- 6. the LDS boundary ---------------------------------------------------------------------------

def lds_need(S, A, n):
    """The LDS an item's tables take in the unique kernels (kernels/lattice_nbest.hpp): 24 B per
    list entry, five words per state, two per arc."""
    return 24 * n * S + 4 * (5 * S + 2 * A)


def lds_budget(n):
    return 4096 + 1024 * n


def budget_pair(n):
    """Two items about the LDS budget at n: the first's tables are the largest that fit (one
    more arc would not), the second has that one arc more.  A chain with parallel arcs of one
    olabel on its first rung."""
    B = lds_budget(n)
    S = (B - 1024) // (24 * n + 28)
    A = (B - 24 * n * S - 20 * S) // 8
    assert A >= S - 1 and lds_need(S, A, n) <= B < lds_need(S, A + 1, n)
    out = []
    for extra in (A - (S - 1), A + 1 - (S - 1)):
        start, finals, arcs = ladder(S, False, False)
        arcs = [lst[:1] for lst in arcs]
        arcs[0] += [(3, k % 2, 0.5 + 0.25 * (k % 4), 1) for k in range(extra)]
        out.append((start, finals, arcs))
    return out


@pytest.mark.parametrize("n", (1, 3, 16))
def test_lds_budget_edge(n, monkeypatch, capfd):
    """The item one arc over the unique kernels' need takes the HBM tier, the one just under it
    the LDS tier; with the plain kernels' 16 B per entry both would fit."""
    monkeypatch.delenv("FSTAMD_NBEST_LDS", raising=False)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    under, over = budget_pair(n)
    exp = [expect(under, n), expect(over, n)]
    check([under], n, exp=exp[:1])
    assert route_line(capfd) == (1, 1, 0)
    check([over], n, exp=exp[1:])
    assert route_line(capfd) == (1, 0, 1)
    check([under, over], n, exp=exp)
    assert route_line(capfd) == (2, 1, 1)
    S, A = len(over[1]), sum(len(a) for a in over[2])
    assert 16 * n * S + 4 * (5 * S + 2 * A) <= lds_budget(n)
    monkeypatch.setenv("FSTAMD_NBEST_LDS", str(lds_need(S, A, n) + 15))
    check([under, over], n, exp=exp)
    assert route_line(capfd) == (2, 2, 0)


# ---- 7. device entry and shards --------------------------------------------------------------------

def run_device_unique(cs, num, n, cap):
    out = DeviceOut(num * n, cap)
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    rc = F.lib().fst_device_nbest_unique_lhs(C.byref(cs), n, C.byref(opts), C.byref(out.desc),
                                             None)
    assert rc == FF.FST_OK
    return out


def test_device_entry_small_arena(sweep):
    items, exp = sweep
    items, n = items[:120], 5
    want = [s for e in exp[n][:120] for s in e]
    lhs = F.LhsBatch.from_fsts(items)
    d = DeviceLhs(lhs)
    full = run_device_unique(d.cs, len(items), n, n * int(lhs.state_offsets[-1]))
    assert F.last_launch_stats().engine == 14
    assert full.items() == want
    need = sum(len(e[1]) for e in want if e[0] == OK)
    assert full.cursor() == need > 0
    # an arena one arc short: the strings that do not fit say so, the cursor says what is needed
    short = run_device_unique(d.cs, len(items), n, need - 1)
    assert short.cursor() == need
    have = short.items()
    assert (FULL,) in have
    for i, e in enumerate(have):
        assert e == want[i] or e == (FULL,), i
    assert run_device_unique(d.cs, len(items), n, short.cursor()).items() == want


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
    out = run_device_unique(d.cs, len(items), 5, 5 * int(lhs.state_offsets[-1]))
    have = out.items()
    for i, e in enumerate(exp):
        assert have[5 * i:5 * i + 5] == ([(UNSUPPORTED,)] * 5 if i == victim else e), i


def test_shards_do_not_show(sweep):
    items, exp = sweep
    items = items[:100]
    assert len(items) % 3
    lhs = F.LhsBatch.from_fsts(items)
    one = F.nbest_unique_lhs_batch(lhs, 5)
    assert strings_of(one, 500) == [s for e in exp[5][:100] for s in e]
    got = F.nbest_unique_lhs_batch(lhs, 5, devices=[0], shards=3)
    same_bytes(got, one, "three shards")


# ---- 8. end to end: hypotheses in, n distinct readings out -----------------------------------------

def test_end_to_end_on_the_device():
    """256 hypothesis lists whose members differ in the spelling of digits, through tagger and
    verbalizer: the unique entry's readings are pairwise different and the model's, while the
    plain entry at the same n repeats texts."""
    rng = np.random.default_rng(14)
    num, n = 256, 4
    items = [SY.respelled_union(rng, t, 4) for t in SY.utterances(rng, num, 4, 10)]
    tagged = F.compose_frozen_lhs_batch(load_blob(tagger_blob()), F.LhsBatch.from_fsts(items),
                                        project_output=True, connect=True)
    spoken = F.compose_frozen_lhs_batch(load_blob(verbalizer_blob()), tagged.as_lhs(),
                                        connect=True)
    assert np.all(tagged.status == OK) and np.all(spoken.status == OK)
    lhs = spoken.as_lhs()
    exp = [expect(spoken.item(i), n) for i in range(num)]
    d = DeviceLhs(lhs)
    ns, na = int(lhs.state_offsets[-1]), int(lhs.arc_offsets[-1])
    paths = run_device_unique(d.cs, num, n, n * ns)
    assert paths.items() == [s for e in exp for s in e]
    texts, text_status = emit_text(paths, num * n, 8 * n * na + 64)
    assert text_status == [s[0] for e in exp for s in e]
    plain = F.batch_result_to_text(F.nbest_lhs_batch(lhs, n)).texts()
    plain_status = F.nbest_lhs_batch(lhs, n).status.reshape(num, n)
    repeats = 0
    for i in range(num):
        mine = [texts[i * n + k] for k in range(n) if exp[i][k][0] == OK]
        assert mine and len(set(mine)) == len(mine), i
        assert mine == [bytes(l - 1 for l in s[2] if l) for s in exp[i] if s[0] == OK], i
        theirs = [plain[i * n + k] for k in range(n) if int(plain_status[i, k]) == OK]
        repeats += len(theirs) - len(set(theirs))
        assert set(theirs) <= set(mine) or len(mine) == n, i
    assert repeats > 0          # the reason for the entry: the plain n-best does repeat texts
