"""The band replay (kernels/lazy_band.hpp): exact lazy composeShortestPath over a sliding
window of rhs states, for rhs whose arcs all go forward (RhsView::jump_back == 0) -- config
3's epsilon-dense transducer.  Every case is bit-compared with the oracle, and the route
log (FSTAMD_ROUTE_LOG, C-level stderr) shows which strings the band took:

* epsilon-dense lattices larger than the window (slides), lengths 0..251;
* random forward-only rhs with epsilon arcs, epsilon self-loops, tie-heavy weights and
  finals, with the 1-, 2- and 4-byte back-pointer encodings (arcs per state, jump sizes);
* a window forced too small (FSTAMD_BAND_WS): every string overflows to the dense replay,
  whose answers are the same;
* strings the band does not take (label 0: lhs epsilon phases) go on to the rounds engine;
* a sweep of 200 random forward-only rhs in ten families, one per fast path of the replay
  (test_sweep, sweep_case), each run with and without the early exit against one oracle call.
"""
import math
import re

import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
from test_gpu_parity import LAZY, bits, check, csr, expected_status, load_blob

pytestmark = pytest.mark.gpu


def handed_on(err):
    """Strings each band launch handed on: the capped launch with the early exit, then
    (if any) the whole-rhs launch."""
    m = re.findall(r"band replay \([^)]*\) handed on (\d+)", err)
    return [int(x) for x in m]


@pytest.fixture(params=["early", "full"])
def early_mode(request, monkeypatch):
    """Both ways of running the band: with the exact early exit (the default) and the
    reference's whole-product replay (FSTAMD_NO_EARLY=1)."""
    if request.param == "full":
        monkeypatch.setenv("FSTAMD_NO_EARLY", "1")
    return request.param


@pytest.fixture
def route(monkeypatch):
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    monkeypatch.setenv("FSTAMD_LAZY_TINY", "0")  # straight to the band (no LDS replays)


def forward_rhs(rng, ns, deg, jump, labels=3, wmax=2, frac=False, eps_loops=True):
    """A rhs whose arcs go forward (t >= s): deg arcs per state, t - s <= jump."""
    f = O.Fst()
    for _ in range(ns):
        f.add_state(float(rng.integers(0, 3)) if rng.random() < 0.6 else math.inf)
    f.start = 0
    for s in range(ns):
        for _ in range(int(rng.integers(1, deg + 1))):
            il = int(rng.integers(0, labels + 1))
            t = min(ns - 1, s + int(rng.integers(0 if (il or eps_loops) else 1, jump + 1)))
            w = float(rng.integers(0, wmax + 1)) + (float(rng.random()) if frac else 0.0)
            f.add_arc(s, il, int(rng.integers(0, labels + 1)), w, t)
    return f


@pytest.mark.parametrize("T", [1024, 3000])
def test_eps_dense_slides(route, capfd, early_mode, T):
    blob = O.freeze(O.gen("eps_dense", T, 12))
    lens = [0, 1, 2, 11, 64, 130, 200, 251]
    check(blob, *csr([[1] * L for L in lens]), LAZY)
    assert handed_on(capfd.readouterr().err) == [0]


@pytest.mark.parametrize("seed", range(12))
def test_random_forward(route, capfd, early_mode, seed):
    rng = np.random.default_rng(7100 + seed)
    # deg / jump chosen so the back pointer takes 1 B (seeds 0-3), 2 B (4-7), 4 B (8-11)
    deg, jump = [(4, 3), (40, 5), (30, 5000)][seed // 4]
    ns = int(rng.integers(20, 400)) if seed < 8 else 6000
    f = forward_rhs(rng, ns, deg, jump, frac=seed % 3 == 0)
    blob = O.freeze(f)
    seqs = [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, 40)))] for _ in range(24)]
    check(blob, *csr(seqs), LAZY)
    err = capfd.readouterr().err
    assert handed_on(err), err[-2000:]  # the band ran


def test_window_too_small_falls_back(route, capfd, monkeypatch):
    monkeypatch.setenv("FSTAMD_BAND_WS", "64")
    blob = O.freeze(O.gen("eps_dense", 512, 12))
    lens = [70, 90, 151]  # open states span L + 3 > 64
    check(blob, *csr([[1] * L for L in lens]), LAZY)
    # both band launches (capped, then the whole rhs) hand all three on
    assert handed_on(capfd.readouterr().err) == [3, 3]


def test_label0_strings_go_on(route, capfd):
    blob = O.freeze(O.gen("eps_dense", 256, 12))
    seqs = [[1] * 20, [1, 0, 1], [0], [1] * 33]
    got, _ = check(blob, *csr(seqs), LAZY)
    assert got.status[0] == F.FST_PATH_OK and got.status[3] == F.FST_PATH_OK


def test_early_exit_beyond_state_cap(route, capfd):
    # the capped launch keeps back pointers for 2 x window states past the start; strings
    # whose best final lies further (the epsilon-dense rhs with only its last state final)
    # overflow there and are answered by the whole-rhs launch (and again if the host entry
    # reruns the batch with a larger path arena: the paths carry ~T epsilon arcs)
    f = O.gen("eps_dense", 1000, 12)
    f.finals = [math.inf] * (f.num_states - 1) + [0.0]
    blob = O.freeze(f)
    check(blob, *csr([[1] * L for L in (1, 3, 8)]), LAZY)
    h = handed_on(capfd.readouterr().err)
    assert h and h[0::2] == [3] * len(h[0::2]) and h[1::2] == [0] * len(h[1::2]), h


@pytest.mark.parametrize("seed", range(4))
def test_negative_finals_no_early_exit(route, capfd, seed):
    # a negative final weight breaks the early exit's bound (total >= dist): such an rhs
    # goes to the hashed replay (weights not all >= +0), which takes no early exit, and the
    # answers stay the oracle's
    rng = np.random.default_rng(7300 + seed)
    f = forward_rhs(rng, int(rng.integers(20, 200)), 4, 3)
    for s in range(0, f.num_states, 3):
        f.finals[s] = -float(rng.integers(1, 4))
    blob = O.freeze(f)
    seqs = [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, 30)))] for _ in range(24)]
    check(blob, *csr(seqs), LAZY)
    assert handed_on(capfd.readouterr().err) == []  # not the band


def test_without_arc_table(route, capfd, monkeypatch):
    # the strided per-state arc table (DeviceFst::band_il / band_rec) is the default; the
    # span-then-arcs reads without it must give the same answers
    monkeypatch.setenv("FSTAMD_NO_BAND_TABLE", "1")
    blob = O.freeze(O.gen("eps_dense", 1024, 12))
    check(blob, *csr([[1] * L for L in (0, 1, 11, 64, 200)]), LAZY)
    rng = np.random.default_rng(7400)
    f = forward_rhs(rng, 300, 40, 5)
    blob = O.freeze(f)
    seqs = [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, 40)))] for _ in range(24)]
    check(blob, *csr(seqs), LAZY)
    assert handed_on(capfd.readouterr().err)


@pytest.mark.parametrize("seed", range(4))
def test_slot_fold_mixed_pops(route, capfd, early_mode, seed):
    # the slot fold takes a pop only when every candidate distance is a finite, >= +0 value
    # with 6 clear low mantissa bits; integer and dyadic weights with a few 0.1 ones make
    # pops of both kinds within one string, and states past 64 arcs (seeds 2, 3: no arc
    # table, the wave-wide span search) take the old fold throughout
    rng = np.random.default_rng(7500 + seed)
    deg = 8 if seed < 2 else 90
    f = forward_rhs(rng, int(rng.integers(40, 300)), deg, 6, labels=2)
    for st in range(len(f.arcs)):
        arcs = []
        for il, ol, w, t in f.arcs[st]:
            r = rng.random()
            arcs.append((il, ol, w + (0.1 if r < 0.1 else 0.5 if r < 0.3 else 0.0), t))
        f.arcs[st] = arcs
    blob = O.freeze(f)
    seqs = [[int(x) for x in rng.integers(1, 3, int(rng.integers(0, 40)))] for _ in range(32)]
    check(blob, *csr(seqs), LAZY)
    assert handed_on(capfd.readouterr().err)


# ---------------------------------------------------------------------------------------
# The sweep: 200 random forward-only rhs of 64 strings, ten families of 20 seeds.  One
# oracle call per rhs; the GPU runs twice (early exit, FSTAMD_NO_EARLY=1) against it.
# ---------------------------------------------------------------------------------------

# MODEL_COUNTS.  What the Python replay model (lazy_model.lazy_via_buckets with counters added
# by hand, whole replay, the six longest strings of the seed) counts on these rhs:
#   ids open at one distance span this many 64-id bitmap words (> 1: pops advance past the
#   cached word): ties 37 (seed 7600), mixed 10 (7620), backptr 20 (7640), jump32 5 (7660),
#   span64 16 (7680), wide 14 (7700) and 18 (7707), ids 8 (7720), slide 2 (7740), finals 18
#   (7760), start 4 (7787);
#   pops of an id more than 256 behind the newest (the LDS ring's reach: the HBM ring is
#   read): ties 28,815 of 82,560 pops, backptr 50,561 of 95,123, span64 13,024 of 47,773,
#   finals 16,232 of 48,604, ids 652 of 9,379 (7720) and 1,461 of 19,856 (7727), mixed 3,428
#   of 19,811, wide 493 of 7,592; none in slide;
#   no popped id falls 4,032 behind the newest (the band's id ring) in the eight longest
#   strings of any of the 200 rhs;
#   finals: 14 of the 120 longest strings (six per rhs), in 10 of the 20 rhs, meet a final
#   tuple that ties the best total with a smaller id after the best was set, with and
#   without the early exit.
SWEEP_SEED = 7600
SWEEP_FAMILIES = ["ties", "mixed", "backptr", "jump32", "span64", "wide", "ids", "slide",
                  "finals", "start"]
SWEEP_PER_FAMILY = 20
SWEEP_CHUNK = 5  # rhs per test id: 4 ids per family, 40 ids


def sweep_case(family, seed):
    """(rhs, strings) of one sweep seed; family i owns seeds SWEEP_SEED + 20 i .. + 19.

    Slides and cached-word advances are not counted in release builds; they follow from the
    construction; the replay model's counters agree (MODEL_COUNTS below).

    Every rhs goes forward only (the band's domain), has input epsilons, a final last state
    with a self-loop per label (a string that runs to the end still ends OK), weights and
    finals >= +0 and finite (the early exit applies).  Most jumps are short (<= 3) even where
    the widest is long, or every string would sit in the last state after a few labels.

    ties     weights {0, 1, 2}; a 0-weight epsilon chain s -> s + 1 through half the
             states and epsilon self-loops (0-weight ones too): many equal distances, the
             relax rule's (id, ilabel, olabel) tie-breaks decide.
    mixed    integer, dyadic (+0.5) and 0.1-step weights mixed within one state: a string's
             pops alternate between the slot fold (every candidate distance has its 6 low
             mantissa bits clear) and the label-comparing fold.
    backptr  back pointers of 1 B (up to 6 arcs, jump 3: 1 + 2 + 3 bits), 2 B (two states of
             40 arcs, jump 5: 1 + 3 + 6 bits) and 4 B (two states of 70 arcs and a widest jump
             of 600, one arc in a hundred: 1 + 10 + 7 bits), by seed % 3.
    jump32   the widest jump is exactly 31 (seed even: the slot fold's precondition holds)
             or 32 (odd: it does not; the route log's plan line is asserted).
    span64   a few states, the start among them, carry exactly 64 arcs (even seeds: the arc
             table's limit, 64 slots without padding) or 65 (odd: no table, and the state
             takes the wave-wide span search).
    wide     85 % of the weights are 0 and every final costs >= 1, so that hundreds of
             tuples are open at distance 0 (more than the 64 ids of the cached bitmap word:
             pops advance past it), none of them a final that would end the replay early.
    ids      long strings (30..55) on 96..128 states with up to 8 arcs per state and weights
             {0, 1}: lattices of 10^4 tuples whose open set outgrows the 256-id LDS ring, so
             a pop finds its window index in the HBM ring.
    slide    strings of length <= 15 (window: 64 states) on an rhs of 200..260 states, more
             than three windows, whose only finals are its last 3 states, reached through
             epsilon arcs: the window slides the whole way, and the capped launch (back
             pointers for 2 windows of states) overflows to the whole-rhs launch (asserted).
             Every arc costs 1 or 2 and moves at most 3 states on, so the tuples at one
             distance d lie within about 3 min(d, L) states of each other: the open set fits
             the window while it slides.
    finals   weights {0, 1, 2, 3}; the only finals are those of a pair of epsilon arcs at
             every fourth state, built so that two final tuples tie at the best total and the
             one with the smaller id is popped later (at a larger distance, with a smaller
             final): the early exit must still wait for it.
    start    start states above 0 (the back pointers' index is relative to the start).
    """
    rng = np.random.default_rng(seed)
    deg, jump, labels, wmax = 4, 3, 3, 2
    lens = (0, 80)
    if family == "backptr":
        jump = [3, 5, 600][seed % 3]
    elif family == "jump32":
        jump = 31 + seed % 2
    elif family == "mixed":
        deg, jump, labels, lens = 4, 4, 2, (0, 48)
    elif family == "wide":
        lens = (10, 50)
    elif family == "ids":
        deg, jump, wmax, lens = 6, 8, 1, (30, 56)
    elif family == "slide":
        lens = (0, 16)
    elif family == "finals":
        wmax = 3
    # The band's window holds 2 (L + 1) + 2 (jump + 1) states, rounded up to a power of two (L:
    # the batch's longest string).  The whole replay of a random rhs opens tuples over far
    # more states than that (0-weight epsilon chains reach everywhere at one distance), which
    # is the dense replay's case, not the band's: outside `slide` the rhs is no larger than
    # the window of a batch whose longest string has 3/4 of the family's top length.
    win = 64
    while win < 2 * (lens[1] * 3 // 4 + 1) + 2 * (jump + 1):
        win *= 2
    ns = int(rng.integers(min(40, win // 2), min(400, win) + 1))
    if family == "backptr" and seed % 3 == 2:
        ns = int(rng.integers(700, 900))  # (window: 2,048 states)
    elif family == "ids":
        ns = int(rng.integers(win * 3 // 4, win + 1))
    elif family == "slide":
        ns = int(rng.integers(200, 261))
    f = O.Fst()
    for _ in range(ns):
        if family == "wide":
            f.add_state(float(rng.integers(1, 3)) if rng.random() < 0.6 else math.inf)
        elif family in ("finals", "slide"):
            f.add_state(math.inf)
        else:
            f.add_state(float(rng.integers(0, 3)) if rng.random() < 0.6 else math.inf)
    if family == "slide":
        for s in range(ns - 3, ns):
            f.finals[s] = float(rng.integers(0, 3))
    f.finals[ns - 1] = 1.0 if family == "wide" else 0.0
    f.start = int(rng.integers(1, ns // 2)) if family == "start" else 0

    def weight():
        if family == "wide":
            return 0.0 if rng.random() < 0.85 else 1.0
        if family == "slide":
            return float(rng.integers(1, 3))
        w = float(rng.integers(0, wmax + 1))
        if family == "mixed":
            r = rng.random()
            w += 0.1 if r < 0.1 else 0.5 if r < 0.3 else 0.0
        return w

    def target(s, lo):
        j = jump if (jump <= 8 or rng.random() < (0.1 if jump < 100 else 0.01)) else 3
        return min(ns - 1, s + int(rng.integers(lo, j + 1)))

    full = {}  # states with a set number of arcs
    if family == "span64":
        full = {f.start: 64 + seed % 2, ns // 3: 64 + seed % 2, ns // 2: 64 + seed % 2}
    if family == "backptr" and seed % 3:
        full = {0: 30 * (seed % 3) + 10, ns // 3: 30 * (seed % 3) + 10}
    for s in range(ns - 1):
        # one arc per label (no string dies for want of one), then up to deg - 1 more of any
        # ilabel, epsilon included; epsilon arcs move on (t > s) except the ties family's loops
        ils = list(range(1, labels + 1))
        n = full[s] if s in full else labels + int(rng.integers(0, deg))
        ils += [int(rng.integers(0, labels + 1)) for _ in range(n - labels)]
        for il in ils:
            f.add_arc(s, il, int(rng.integers(0, labels + 1)), weight(), target(s, 0 if il else 1))
        if family == "ties":
            if rng.random() < 0.5:
                f.add_arc(s, 0, int(rng.integers(0, 4)), 0.0, s + 1)
            if rng.random() < 0.1:
                f.add_arc(s, 0, int(rng.integers(0, 4)), float(rng.integers(0, 2)), s)
        if family == "finals" and s % 4 == 0 and s + 2 < ns - 1:
            # from s the epsilon arc into s + 1 is relaxed first (olabel 1) and costs 2, the one
            # into s + 2 costs 0: at the string's end the tuple at s + 2 (final 2) is popped
            # first and sets the best total, then the tuple at s + 1 (final 0), whose id is
            # the smaller, is popped at that very distance and ties it
            f.add_arc(s, 0, 1, 2.0, s + 1)
            f.add_arc(s, 0, 2, 0.0, s + 2)
            f.finals[s], f.finals[s + 1], f.finals[s + 2] = math.inf, 0.0, 2.0
        if family == "slide":  # an epsilon path to the finals from everywhere
            f.add_arc(s, 0, int(rng.integers(0, 4)), weight(), target(s, 1))
    for il in range(1, labels + 1):
        f.add_arc(ns - 1, il, il, weight(), ns - 1)
    if family in ("jump32", "backptr") and jump > 8:  # the widest jump itself
        f.add_arc(f.start, 1, 1, 1.0, min(ns - 1, f.start + jump))
    seqs = [[int(x) for x in rng.integers(1, labels + 1, int(rng.integers(*lens)))]
            for _ in range(64)]
    return f, seqs


def compare(got, ref, exp):
    """test_gpu_parity.check's comparison against a reference computed once."""
    assert np.array_equal(got.status, exp), (np.nonzero(got.status != exp)[0][:10],
                                             got.status[got.status != exp][:10],
                                             exp[got.status != exp][:10])
    okm = exp == F.FST_PATH_OK
    assert np.array_equal(np.diff(got.offsets)[okm], np.diff(ref.offsets)[okm])
    for i in np.nonzero(okm)[0]:
        a0, a1 = int(got.offsets[i]), int(got.offsets[i + 1])
        b0, b1 = int(ref.offsets[i]), int(ref.offsets[i + 1])
        assert np.array_equal(got.ilabels[a0:a1], ref.ilabels[b0:b1]), i
        assert np.array_equal(got.olabels[a0:a1], ref.olabels[b0:b1]), i
        assert np.array_equal(bits(got.weights[a0:a1]), bits(ref.weights[b0:b1])), i
    assert np.array_equal(bits(got.finals[okm]), bits(ref.finals[okm]))


SWEEP_IDS = [(fam, c) for fam in SWEEP_FAMILIES for c in range(SWEEP_PER_FAMILY // SWEEP_CHUNK)]


@pytest.mark.parametrize("family,chunk", SWEEP_IDS, ids=["%s-%d" % p for p in SWEEP_IDS])
def test_sweep(route, capfd, monkeypatch, family, chunk):
    """Five rhs of one family (sweep_case names the families and their seeds).  Each id
    holds the sweep's conditions on its own 320 strings, which is stricter than holding
    them per family: the oracle answers >= 80 % OK, the band hands on <= 10 % (the last
    `handed on` line of each run), it reports early exits in early mode and none with
    FSTAMD_NO_EARLY=1."""
    monkeypatch.setenv("FSTAMD_BFS_PROF", "1")
    first = SWEEP_SEED + SWEEP_PER_FAMILY * SWEEP_FAMILIES.index(family) + SWEEP_CHUNK * chunk
    n_str = n_ok = 0
    passed_on = {"early": 0, "full": 0}
    exits = {"early": 0, "full": 0}
    capped_over = 0
    for seed in range(first, first + SWEEP_CHUNK):
        f, seqs = sweep_case(family, seed)
        blob = O.freeze(f)
        labels, offsets = csr(seqs)
        ref = O.batch_run(blob, labels, offsets, 0, 1, threads=4)
        exp = expected_status(ref)
        n_str += len(seqs)
        n_ok += int((exp == F.FST_PATH_OK).sum())
        rhs = load_blob(blob)
        for mode in ("early", "full"):
            if mode == "full":
                monkeypatch.setenv("FSTAMD_NO_EARLY", "1")
            else:
                monkeypatch.delenv("FSTAMD_NO_EARLY", raising=False)
            capfd.readouterr()
            got = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, LAZY)
            err = capfd.readouterr().err
            compare(got, ref, exp)
            h = handed_on(err)
            assert h, (seed, mode, err[-2000:])  # the band ran
            passed_on[mode] += h[-1]
            if mode == "early":
                capped_over += h[0]
            exits[mode] += sum(int(x) for x in re.findall(r"early exits (\d+)", err))
            plans = re.findall(r"arc table (on|off), slot fold (on|off)", err)
            if family == "jump32":
                assert plans and set(plans) == {("on", "on" if seed % 2 == 0 else "off")}, (seed, plans)
            if family == "span64":
                assert plans and set(plans) == {("on" if seed % 2 == 0 else "off", "on")}, (seed, plans)
    print("sweep %s-%d: %d strings, %d OK in the oracle, handed on %s, capped launch overflows "
          "%d, early exits %s" % (family, chunk, n_str, n_ok, passed_on, capped_over, exits))
    assert n_ok >= 0.8 * n_str, (n_ok, n_str)
    assert passed_on["early"] <= 0.1 * n_str and passed_on["full"] <= 0.1 * n_str, passed_on
    assert exits["early"] > 0 and exits["full"] == 0, exits
    if family == "slide":
        assert capped_over >= n_ok, (capped_over, n_ok)  # every OK string lies past the cap
