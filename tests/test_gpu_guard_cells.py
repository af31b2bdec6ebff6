"""GPU parity of the guard bands around tier P's packed cells (kernels/eager_pull.hpp RK 6,
kernels/pull_window.hpp): the cell array is 64 absent cells, the 320 window cells, 128 absent
cells, and a row lane reads the cell at base - delta4 with no clamp -- sources outside the
window, blocks without records and every read of a label-miss row land in a guard.

As in test_gpu_packed_cells.py every case is compared bit for bit with the oracle, runs again
with FSTAMD_NO_PACK=1 (the unpacked RK 3 path) and asserts the route from the log line "eager
pull: packed cells on|off".  check() goes through the host entry, whose streamed route runs
the weight-code instances (code_pull.hip); device_call() through the device entry (the label
instances, eager_pull.hip); the text cases through the streamed text route (text_pull.hip).

Each case is the smallest shape that reaches one address range of the padded array:
  - backward arcs: the layer's tuples sit at the window's origin and their targets' sources
    below slot 0 (the low guard);
  - a jump span of exactly 63 (20 back, 43 forward): a single live state in the last slots of
    a 316-cell window, so the next window's only row reads past slot 320 (the high guard);
  - three in-labels (1 + t % 3): rows of mixed hits and misses, whole layers of misses, hub
    states (more in-arcs than a block holds) between them;
  - the last states of the rhs: the window's last row runs past num_states - 1;
  - several strings per wave (FSTAMD_P_GRID=3): wide, narrow, handed on, narrow -- the reset by
    the last window's width must leave the window absent and the guards alone;
  - the metric's shape at T = 300, B = 12;
  - the gate: a span of 64 logs "off".
"""
import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
from test_gpu_packed_cells import assert_device_result, check_both, device_call, routes
from test_gpu_parity import EAGER, csr, load_blob
from test_gpu_text import expected as text_expected, same as text_same

pytestmark = pytest.mark.gpu


def device_both(blob, seqs, monkeypatch, capfd, want="on"):
    """the device entry on the default route (asserted: `want`), then with FSTAMD_NO_PACK=1"""
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    rhs = load_blob(blob)
    labels, offsets = csr(seqs)
    ref = O.batch_run(blob, labels, offsets, 1, 1)
    max_len = max([len(s) for s in seqs] + [1])
    capfd.readouterr()
    assert_device_result(device_call(rhs, seqs, max_len), ref)
    assert routes(capfd.readouterr().err) == {want}
    monkeypatch.setenv("FSTAMD_NO_PACK", "1")
    assert_device_result(device_call(rhs, seqs, max_len), ref)
    assert routes(capfd.readouterr().err) == {"off"}
    monkeypatch.delenv("FSTAMD_NO_PACK")


def banded(ns, back, fwd, start, seed, fan_of=lambda t: 1 + t % 12):
    """Every arc into state t carries the ilabel 1 + t % 3 and comes from a source in [t - fwd,
    t + back] (so the rhs jumps at most `back` states back and `fwd` forward, and does both:
    the two extreme arcs are added for every state that has them); fan-in fan_of(t), weights
    half 7 and half from {0, 1, 2}, finals 0..4 or +inf"""
    rng = np.random.default_rng(seed)
    f = O.Fst()
    for _ in range(ns):
        f.add_state(float(rng.integers(0, 5)) if rng.random() < 0.7 else float("inf"))
    f.start = start
    run = {}  # arcs of one source with one ilabel: at most 8 fit the key's j

    def arc(s, t, ol):
        il = 1 + t % 3
        if run.get((s, il), 0) >= 8:
            return False
        run[(s, il)] = run.get((s, il), 0) + 1
        w = 7.0 if rng.random() < 0.5 else float(rng.integers(0, 3))
        f.add_arc(s, il, ol, w, t)
        return True

    for t in range(ns):
        lo, hi = max(0, t - fwd), min(ns - 1, t + back)
        added = 0
        for s in (t - fwd, t + back):
            if 0 <= s < ns:
                added += arc(s, t, 1 + added)
        tries = 0
        while added < fan_of(t) and tries < 200:
            tries += 1
            added += arc(int(rng.integers(lo, hi + 1)), t, 1 + added)
    return f


def walks(rng, num, max_len):
    return [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, max_len + 1)))] for _ in range(num)]


def test_backward_arcs_read_below_slot_zero(monkeypatch, capfd):
    # s -> s - 6 .. s + 3 from state 150 of 200: the window's origin is cmin - 6, and the
    # strings that only step 6 back keep their one tuple there, with every source of the
    # row's first lanes below slot 0
    ns, start = 200, 150
    blob = O.freeze(banded(ns, 6, 3, start, 611))
    down = [[1 + (start - 6 * (k + 1)) % 3 for k in range(L)] for L in (1, 2, 3, 10, 24)]
    seqs = down + walks(np.random.default_rng(612), 150, 40)
    check_both(blob, seqs, monkeypatch, capfd)
    device_both(blob, seqs, monkeypatch, capfd)


def funnel(tail, extra=None):
    """States with arcs s -> s - 20 and s -> s + 43 (and s -> s + 1, s -> s + 7), all of
    ilabel 1 except the arcs into state z = 315, which carry ilabel 2.  From the start state
    100 the prefix 1^4 spreads the layer over [20, 272]; the label 2 then leaves z alone alive
    (from 272) in the last slot of the 316-cell window [0, 315]; the next window's one row
    owns the targets [295, 358] and reads sources up to slot 378.  tail: states past z (10:
    that row runs past the last state and hi is clipped); extra: one more arc 0 -> extra"""
    z = 100 + 5 * 43
    ns = z + tail
    rng = np.random.default_rng(621)
    f = O.Fst()
    for s in range(ns):
        f.add_state(float(s % 4) if s % 5 else float("inf"))
    f.start = 100
    for s in range(ns):
        for k, d in enumerate((-20, 43, 1, 7)):
            t = s + d
            if 0 <= t < ns:
                w = 7.0 if rng.random() < 0.5 else float(rng.integers(0, 3))
                f.add_arc(s, 2 if t == z else 1, 1 + k, w, t)
    if extra:
        f.add_arc(0, 1, 9, 0.0, extra)
    return f, z


@pytest.mark.parametrize("tail", [100, 10])
def test_span_63_reads_past_slot_w(tail, monkeypatch, capfd):
    f, _ = funnel(tail)
    blob = O.freeze(f)
    seqs = [[1] * 4 + [2] + [1] * j for j in range(5)]
    seqs += [[1] * k + [2] + [1] * j for k in (1, 2, 3) for j in (0, 2)]  # (no 2-arc yet: EMPTY)
    seqs += [[1] * L for L in range(5)] + [[1, 1, 1, 1, 2, 2], [2]]
    check_both(blob, seqs, monkeypatch, capfd)
    device_both(blob, seqs, monkeypatch, capfd)


def test_gate_refuses_span_64(monkeypatch, capfd):
    # the same rhs with one arc 0 -> 44: 20 back + 44 forward does not fit the guards (nor
    # the record's delta byte)
    f, _ = funnel(100, extra=44)
    blob = O.freeze(f)
    seqs = [[1] * 4 + [2] + [1] * j for j in range(3)] + [[1] * L for L in range(5)]
    check_both(blob, seqs, monkeypatch, capfd, want="off")


def test_miss_rows_mixed_labels_and_hubs(monkeypatch, capfd):
    # three in-labels: every row mixes hits and misses; label 4 has no arc (a layer whose
    # every row misses); fan-in up to 12, and 30 for every 7th state (hub blocks whose
    # neighbours are miss lanes, inactive in the hub loop)
    blob = O.freeze(banded(180, 6, 3, 0, 631, fan_of=lambda t: 30 if t % 7 == 3 else 1 + t % 12))
    rng = np.random.default_rng(632)
    seqs = walks(rng, 200, 50)
    seqs += [[4], [1, 4], [1, 2, 4, 1], [1 + k % 3 for k in range(20)] + [4]]
    check_both(blob, seqs, monkeypatch, capfd)
    device_both(blob, seqs, monkeypatch, capfd)


def test_last_states_of_the_rhs(monkeypatch, capfd):
    # the start 8 states before the end of an rhs that jumps 40 forward and 23 back: from the
    # first layer on the window's last row runs past num_states - 1 and hi is clipped
    ns = 120
    blob = O.freeze(banded(ns, 23, 40, ns - 8, 641, fan_of=lambda t: 1 + t % 9))
    seqs = walks(np.random.default_rng(642), 150, 30)
    check_both(blob, seqs, monkeypatch, capfd)
    device_both(blob, seqs, monkeypatch, capfd)


def fan_chain(ns):
    """s -> s + d for d = 0..6, all ilabel 1: after k labels the states 0..6k hold tuples"""
    rng = np.random.default_rng(651)
    f = O.Fst()
    for s in range(ns):
        f.add_state(float(s % 4) if s % 5 else float("inf"))
    f.start = 0
    for s in range(ns):
        for d in range(7):
            w = 7.0 if rng.random() < 0.5 else float(rng.integers(1, 3))
            f.add_arc(s, 1, 1 + d, w, min(ns - 1, s + d))
    return f


def test_several_strings_per_wave(monkeypatch, capfd):
    # three waves take all the strings, each a run of: wide (301 tuples in the last layer),
    # narrow, one that outgrows the window at layer 54 (handed on to the push tiers), narrow.
    # A cell the reset left behind, or a guard it touched, would show in the next string
    monkeypatch.setenv("FSTAMD_P_GRID", "3")
    blob = O.freeze(fan_chain(420))
    seqs = []
    for r in range(12):
        seqs += [[1] * (50 - r % 3), [1] * (r % 4), [1] * (60 + r % 5), [1] * (1 + r % 2)]
    check_both(blob, seqs, monkeypatch, capfd)
    device_both(blob, seqs, monkeypatch, capfd)


def test_metric_shape(monkeypatch, capfd):
    # the ambiguous chain at T = 300, B = 12: the streamed host entry (the weight-code
    # instance) and the device entry (the label instance)
    blob = O.freeze(O.gen("ambiguous", 300, 12))
    seqs = [[1] * L for L in range(65)]
    check_both(blob, seqs, monkeypatch, capfd)
    device_both(blob, seqs, monkeypatch, capfd)


def test_metric_shape_text_route(monkeypatch, capfd):
    # ... and the streamed text route (the text instance): the byte 0 is the label 1
    blob = O.freeze(O.gen("ambiguous", 300, 12))
    texts = [bytes(L) for L in range(65)]
    want = text_expected([blob], texts, EAGER)
    stage = F.Fst.from_bytes(blob)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    capfd.readouterr()
    text_same(F.normalize_text_batch([stage], texts, EAGER), want)
    assert routes(capfd.readouterr().err) == {"on"}
    monkeypatch.setenv("FSTAMD_NO_PACK", "1")
    text_same(F.normalize_text_batch([stage], texts, EAGER), want)
    assert routes(capfd.readouterr().err) == {"off"}
