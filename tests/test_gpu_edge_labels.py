"""Labels whose values collide with the engines' markers, and blobs whose arcs are not in
olabel order: every engine against the oracle, bit for bit (statuses, ilabels, olabels,
weight bits, final bits -- test_gpu_parity.check).

**Marker-label rhs** (`marker_rhs`).  0xFFFFFFFE and 0xFFFFFFFF are legal labels in the
reference, and they are also the values of `kSpanMixed` / `kSpanNone` in the per-state
summaries (`RhsView::sspan`), of the padding ilabel in the band replay's strided arc table
and of several "no entry" words.  The rhs has at most 60 states, start 0, forward arcs
only; mixed states carry 1, 0xFFFFFFFE and 0xFFFFFFFF side by side, one state carries only
0xFFFFFFFE (its summary word equals `kSpanMixed`: the mirror build used to read one arc
past such a state), one only 0xFFFFFFFF (`kSpanNone`), the last state has no arc; olabels
include 0 and 0xFFFFFFFF; every state has 0, 3, 5, 6 or 7 arcs, so each state of the
band's 8-slot table has padding.  Two variants: with input epsilons (the dense / band
family) and without (pull, layered, rounds).  64 strings of length 0..15 over the three
labels; the oracle answers >= 80 % of them OK (asserted; 64 / 64 with epsilons, 52 / 64 without).

The band replay used to match a 0xFFFFFFFF label against the table's padding slots
(phantom zero-weight arcs into state 0).  It now marks such a string UNSUPPORTED when the
table is in use, as it does for label 0, and the rounds engine answers it:
`test_marker_band_takes_the_other_strings` pins both halves.

**Unsorted-olabel blobs** (`unsort`, fixture `unsorted`).  fromBytes checks ilabel order only.  Each
state has groups of two to four equal-weight parallel arcs into one target, for its
epsilon arcs and its labelled arcs, and the blob lists each group in descending olabel
order.  Finding on the CPU oracle: the lazy path for the unsorted blob equals the path for
the sorted blob -- on a tie the smaller
olabel wins wherever the arc sits (compose-shortest-path.zig:112-126) -- which
`test_unsorted_oracle_path_equals_sorted` pins.  The band's slot fold keeps the lowest
arc position instead, so an rhs whose arcs are not in (ilabel, olabel) order
(`DeviceFst::band_ol_sorted`) takes the label-comparing fold: the route log's plan line
says "slot fold off".

These tests were first run on the GPU after the fixes (padding labels, the olabel-order
flag, the bounded read in build_mirror_kernel) were in place.
"""
import math
import re

import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
from test_gpu_parity import EAGER, LAZY, bits, check, compare_single, csr, expected_status, load_blob

pytestmark = pytest.mark.gpu

FE, FF = 0xFFFFFFFE, 0xFFFFFFFF
MARKERS = [1, FE, FF]


# ---------------------------------------------------------------------------------------
# engine selectors (restated from test_gpu_lazy_rounds.py, test_gpu_eager_tiers.py and
# test_gpu_lazy_pull.py)
# ---------------------------------------------------------------------------------------

LAZY_ENV = ["FSTAMD_LAZY_ENGINE", "FSTAMD_LAZY_LAYERED", "FSTAMD_LAZY_TINY", "FSTAMD_LAZY_TINY_START",
            "FSTAMD_TINY_WAVES", "FSTAMD_NO_BAND", "FSTAMD_NO_BAND_TABLE", "FSTAMD_LAZY_ONLY_FIRST",
            "FSTAMD_PULL_INDIRECT", "FSTAMD_LP_F64"]


@pytest.fixture(params=["rounds", "general", "replay", "replay_hbm", "dense", "lds", "lds_chain"])
def engine(request, monkeypatch):
    """The seven lazy engines of test_gpu_lazy_rounds.py.  "dense" also sets FSTAMD_NO_BAND:
    these rhs go forward only, so the band would run first and the dense replay would see
    nothing (the band has its own cases below)."""
    for k in LAZY_ENV:
        monkeypatch.delenv(k, raising=False)
    p = request.param
    if p.startswith("lds"):
        monkeypatch.setenv("FSTAMD_LAZY_ENGINE", "lds")
        if p == "lds_chain":
            monkeypatch.setenv("FSTAMD_LAZY_TINY_START", "1")
            monkeypatch.setenv("FSTAMD_TINY_WAVES", "4")
    elif p == "replay_hbm":
        monkeypatch.setenv("FSTAMD_LAZY_ENGINE", "replay")
        monkeypatch.setenv("FSTAMD_LAZY_TINY", "0")
    elif p == "replay":
        monkeypatch.setenv("FSTAMD_LAZY_ENGINE", "replay")
    elif p == "dense":
        monkeypatch.setenv("FSTAMD_LAZY_ENGINE", "dense")
        monkeypatch.setenv("FSTAMD_NO_BAND", "1")
    else:
        monkeypatch.setenv("FSTAMD_LAZY_ENGINE", "rounds")
        if p == "general":
            monkeypatch.setenv("FSTAMD_LAZY_LAYERED", "0")
    return p


@pytest.fixture(params=["", "window", "wave", "wg"], ids=["P", "A0", "A", "B"])
def tier(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("FSTAMD_EAGER_TIER1", request.param)
    else:
        monkeypatch.delenv("FSTAMD_EAGER_TIER1", raising=False)
    return request.param


@pytest.fixture(params=["direct", "indirect", "f64"])
def only_lp(request, monkeypatch):
    for k in LAZY_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FSTAMD_LAZY_ONLY_FIRST", "1")
    if request.param == "indirect":
        monkeypatch.setenv("FSTAMD_PULL_INDIRECT", "1")
    if request.param == "f64":
        monkeypatch.setenv("FSTAMD_LP_F64", "1")


@pytest.fixture(params=["table", "no_table"])
def band(request, monkeypatch):
    """Straight to the band replay (no LDS replays first), with and without its strided arc
    table; FSTAMD_LAZY_ENGINE=dense sends an rhs without input epsilons there too."""
    for k in LAZY_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    monkeypatch.setenv("FSTAMD_LAZY_TINY", "0")
    monkeypatch.setenv("FSTAMD_LAZY_ENGINE", "dense")
    if request.param == "no_table":
        monkeypatch.setenv("FSTAMD_NO_BAND_TABLE", "1")
    return request.param


def handed_on(err):
    return [int(x) for x in re.findall(r"band replay \([^)]*\) handed on (\d+)", err)]


def band_plans(err):
    """(arc table, slot fold) of every band launch plan in the route log."""
    return re.findall(r"band plan: .* arc table (on|off), slot fold (on|off)", err)


# ---------------------------------------------------------------------------------------
# marker-label rhs
# ---------------------------------------------------------------------------------------

def marker_rhs(eps):
    rng = np.random.default_rng(8100 + int(eps))
    ns = 48
    f = O.Fst()
    for s in range(ns):
        f.add_state(float(rng.integers(0, 3)) if s % 5 else math.inf)
    f.start = 0
    ols = [0, 1, 2, FF]

    def arc(s, il, lo=0):
        t = min(ns - 1, s + int(rng.integers(lo, 4)))
        f.add_arc(s, il, ols[int(rng.integers(4))], float(rng.integers(0, 3)), t)

    for s in range(ns - 1):          # the last state has no arc
        if s in (5, 9):              # one ilabel, whose value is a marker's
            for _ in range(3):
                arc(s, FE if s == 5 else FF, 1)
            continue
        base = ([0] if eps else []) + MARKERS
        extra = int(rng.choice([1, 2, 3] if eps else [0, 2, 3]))
        for il in base + [int(rng.choice(base)) for _ in range(extra)]:
            arc(s, il, 1 if il == 0 and rng.random() < 0.7 else 0)
    return f


def marker_seqs():
    rng = np.random.default_rng(8200)
    seqs = [[int(rng.choice(MARKERS)) for _ in range(int(rng.integers(0, 16)))] for _ in range(60)]
    return seqs + [[], [FF], [FE] * 15, [1] * 15]


@pytest.fixture(scope="module", params=["eps", "noeps"])
def marker(request):
    """(variant, fst, blob, seqs, labels, offsets): built once, never changed."""
    f = marker_rhs(request.param == "eps")
    arcs = [len(a) for a in f.arcs]
    assert f.num_states <= 60 and f.start == 0 and arcs[-1] == 0
    assert all(n & (n - 1) for n in arcs if n) and max(arcs) <= 7  # padding in every state
    assert [il for il, _, _, _ in f.arcs[5]] == [FE] * 3 and [il for il, _, _, _ in f.arcs[9]] == [FF] * 3
    assert any({FE, FF} < {a[0] for a in al} for al in f.arcs)
    assert {0, FF} <= {a[1] for al in f.arcs for a in al}
    assert all(t >= s for s, al in enumerate(f.arcs) for _, _, _, t in al)
    blob = O.freeze(f)
    seqs = marker_seqs()
    labels, offsets = csr(seqs)
    for sem in (LAZY, EAGER):
        ref = O.batch_run(blob, labels, offsets, 0 if sem == LAZY else 1, 1)
        ok = (ref.status == O.OR_OK) & (ref.empty == 0)
        assert ok.mean() >= 0.8, (request.param, sem, ok.mean())
    return request.param, f, blob, seqs, labels, offsets


def check_taken(blob, labels, offsets, sem, all_taken=True):
    """check() for a run that may leave strings OVERFLOW / UNSUPPORTED (a tier run alone)."""
    got = F.compose_frozen_shortest_path_batch(load_blob(blob), labels, offsets, 1, sem)
    ref = O.batch_run(blob, labels, offsets, 0 if sem == LAZY else 1, 1)
    exp = expected_status(ref)
    took = (got.status == F.FST_PATH_OK) | (got.status == F.FST_PATH_EMPTY)
    if all_taken:
        assert took.all(), np.unique(got.status, return_counts=True)
    assert np.all((got.status[~took] == F.FST_PATH_OVERFLOW) |
                  (got.status[~took] == F.FST_PATH_UNSUPPORTED))
    assert np.array_equal(got.status[took], exp[took]), np.nonzero(got.status != exp)[0][:8]
    for i in np.nonzero(took & (exp == F.FST_PATH_OK))[0]:
        a0, a1 = int(got.offsets[i]), int(got.offsets[i + 1])
        b0, b1 = int(ref.offsets[i]), int(ref.offsets[i + 1])
        assert np.array_equal(got.ilabels[a0:a1], ref.ilabels[b0:b1]), i
        assert np.array_equal(got.olabels[a0:a1], ref.olabels[b0:b1]), i
        assert np.array_equal(bits(got.weights[a0:a1]), bits(ref.weights[b0:b1])), i
        assert bits(got.finals[i:i + 1])[0] == bits(ref.finals[i:i + 1])[0], i
    return got, took


def test_marker_lazy_engines(marker, engine):
    _, _, blob, _, labels, offsets = marker
    check(blob, labels, offsets, LAZY)


def test_marker_lazy_default_route(marker, monkeypatch):
    for k in LAZY_ENV:
        monkeypatch.delenv(k, raising=False)
    _, _, blob, _, labels, offsets = marker
    check(blob, labels, offsets, LAZY)


def test_marker_lazy_pull(marker, only_lp):
    # the tier alone: whatever it takes is exact, the rest is left OVERFLOW / UNSUPPORTED
    # (with input epsilons the pull does not apply and the default chain answers everything)
    variant, _, blob, _, labels, offsets = marker
    check_taken(blob, labels, offsets, LAZY, all_taken=variant == "eps")


def test_marker_band(marker, band, capfd):
    variant, _, blob, _, labels, offsets = marker
    check(blob, labels, offsets, LAZY)
    err = capfd.readouterr().err
    assert handed_on(err), err[-2000:]  # the band launch ran
    table = "on" if (variant == "eps" and band == "table") else "off"
    plans = band_plans(err)
    assert plans and all(p == (table, "on") for p in plans), plans


def test_marker_band_takes_the_other_strings(marker, band, capfd, monkeypatch):
    # the band alone (FSTAMD_DENSE_NOFALLBACK: no rounds engine behind it).  With the arc
    # table, strings that hold 0xFFFFFFFF are left UNSUPPORTED (their label equals the padding
    # slots' ilabel) and every other string of the batch is answered by the band, exactly;
    # without the table the band answers all of them
    variant, _, blob, seqs, labels, offsets = marker
    monkeypatch.setenv("FSTAMD_DENSE_NOFALLBACK", "1")
    got, took = check_taken(blob, labels, offsets, LAZY, all_taken=False)
    err = capfd.readouterr().err
    assert handed_on(err) and set(handed_on(err)) == {0}, err[-2000:]
    has_ff = np.array([FF in s for s in seqs])
    if variant == "eps" and band == "table":
        assert has_ff.any() and not has_ff.all()
        assert np.all(got.status[has_ff] == F.FST_PATH_UNSUPPORTED)
        assert took[~has_ff].all()
    else:
        assert took.all()


def test_marker_eager_tiers(marker, tier):
    _, _, blob, _, labels, offsets = marker
    check(blob, labels, offsets, EAGER)


def chain_lhs(seq):
    f = O.Fst()
    for _ in range(len(seq) + 1):
        f.add_state(math.inf)
    f.start = 0
    f.finals[len(seq)] = 0.0
    for i, x in enumerate(seq):
        f.add_arc(i, x, x, 0.0, i + 1)
    return f


def test_marker_single_call(marker):
    _, _, blob, seqs, _, _ = marker
    longest = max((s for s in seqs if FF in s and FE in s), key=len)
    compare_single(chain_lhs(longest), blob)


# ---------------------------------------------------------------------------------------
# unsorted-olabel blobs
# ---------------------------------------------------------------------------------------

def parallel_rhs(rng, ns, jump):
    """Forward arcs only, integer weights (the slot fold's domain); every arc comes as a
    group of two to four equal-weight arcs into one target that differ in their olabel."""
    f = O.Fst()
    for _ in range(ns):
        f.add_state(float(rng.integers(0, 3)) if rng.random() < 0.7 else math.inf)
    f.start = 0
    for s in range(ns):
        for il in (0, 1, 2):
            for _ in range(int(rng.integers(1, 3))):
                lo = 1 if il == 0 else 0
                # (mostly short jumps: wide ones alone would end every string in the last state)
                t = min(ns - 1, s + int(rng.integers(lo, (jump if rng.random() < 0.1 else 3) + 1)))
                if il == 0 and t == s:
                    continue
                w = float(rng.integers(0, 3))
                n = int(rng.integers(2, 5))
                for ol in rng.choice(9, n, replace=False):
                    f.add_arc(s, il, int(ol) + 1, w, t)
    return f


def unsort(blob):
    """Swap arcs of the blob in place (the byte-swap technique of
    test_gpu_lazy_pull.py::test_fromBytes_blob_out_of_olabel_order_skips_the_tier): the arcs of
    one state with the same ilabel, target and weight trade places so that their olabels
    descend.  Ilabels stay sorted and each target keeps its first position in the state."""
    hdr = np.frombuffer(blob, "<u4", 6)
    ns, na = int(hdr[2]), int(hdr[3])
    st = np.frombuffer(blob, np.dtype([("off", "<u4"), ("n", "<u4"), ("fin", "<f8")]), ns, 24)
    out = bytearray(blob)
    arcs = np.frombuffer(out, O.ARC_DTYPE, na, 24 + 16 * ns)
    swapped = 0
    for s in range(ns):
        a, e = int(st["off"][s]), int(st["off"][s]) + int(st["n"][s])
        while a < e:
            b = a
            while b < e and arcs["il"][b] == arcs["il"][a]:
                b += 1
            groups = {}
            for i in range(a, b):
                groups.setdefault((int(arcs["next"][i]), float(arcs["w"][i])), []).append(i)
            for pos in groups.values():  # the group's arcs swap places among themselves
                arcs["ol"][pos] = arcs["ol"][pos][::-1].copy()
                swapped += len(pos) > 1
            a = b
    assert swapped
    return bytes(out)


UNSORTED = [(0, 12, 3), (1, 60, 31), (2, 120, 32), (3, 200, 6)]  # (seed, states, jump_fwd)


@pytest.fixture(scope="module", params=UNSORTED, ids=lambda p: "ns%d-jf%d" % (p[1], p[2]))
def unsorted(request):
    seed, ns, jump = request.param
    rng = np.random.default_rng(8300 + seed)
    f = parallel_rhs(rng, ns, jump)
    # (the widest jump itself, so that jump_fwd is exactly `jump`)
    f.add_arc(0, 1, 1, 1.0, min(ns - 1, jump))
    f.add_arc(0, 1, 2, 1.0, min(ns - 1, jump))
    sorted_blob = O.freeze(f)
    blob = unsort(sorted_blob)
    assert O.lib().or_validate(blob, len(blob), 0) == O.lib().or_validate(sorted_blob, len(sorted_blob), 0)
    seqs = [[int(x) for x in rng.integers(1, 3, int(rng.integers(0, 41)))] for _ in range(30)]
    seqs += [[], [1] * 40]
    labels, offsets = csr(seqs)
    return jump, sorted_blob, blob, labels, offsets


def test_unsorted_oracle_path_equals_sorted(unsorted):
    # the CPU finding: composeShortestPath's tie rule looks at the labels, not at the arc's
    # place.  (Eager shortestPath(compose()) does follow the arc order, so its paths differ
    # between the two blobs; the eager engines are compared on the unsorted blob below.)
    _, sorted_blob, blob, labels, offsets = unsorted
    a = O.batch_run(sorted_blob, labels, offsets, 0, 1)
    b = O.batch_run(blob, labels, offsets, 0, 1)
    for k in ("status", "empty", "offsets", "ilabels", "olabels"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(bits(a.weights), bits(b.weights))
    assert np.array_equal(bits(a.finals), bits(b.finals))
    assert ((a.status == O.OR_OK) & (a.empty == 0)).mean() >= 0.8


def test_unsorted_band(unsorted, band, capfd):
    jump, sorted_blob, blob, labels, offsets = unsorted
    check(blob, labels, offsets, LAZY)
    err = capfd.readouterr().err
    assert handed_on(err), err[-2000:]  # the band still ran
    table = "on" if band == "table" else "off"
    plans = band_plans(err)
    assert plans and all(p == (table, "off") for p in plans), plans
    # the same rhs in frozen order keeps the slot fold when jump_fwd < 32
    check(sorted_blob, labels, offsets, LAZY)
    plans = band_plans(capfd.readouterr().err)
    assert plans and all(p == (table, "on" if jump < 32 else "off") for p in plans), plans


def test_unsorted_lazy_engines(unsorted, engine):
    _, _, blob, labels, offsets = unsorted
    check(blob, labels, offsets, LAZY)


def test_unsorted_lazy_default_route(unsorted, monkeypatch):
    for k in LAZY_ENV:
        monkeypatch.delenv(k, raising=False)
    _, _, blob, labels, offsets = unsorted
    check(blob, labels, offsets, LAZY)


def test_unsorted_eager_tiers(unsorted, tier):
    _, _, blob, labels, offsets = unsorted
    check(blob, labels, offsets, EAGER)
