"""GPU parity of tier P's packed (distance, key) cells (kernels/eager_pull.hpp, RK 6).

The host picks the packed cells when the rhs has the packed records (tier P's 4-B records,
a jump span of at most 63 states: build_reverse_mirror) and no distance field of the launch
can wrap ((max_len + 1) * weight < 0x7F00: pull_pack).  Every case is compared bit for bit
with the oracle (check), runs a second time with FSTAMD_NO_PACK=1 (the unpacked RK 3 path),
and asserts the route from the log line "eager pull: packed cells on|off".

The direct layout, which tier P's 4-B records need, wants one in-label per state: every arc
into state t carries the ilabel 1 + t % 3 -- except on the chains of the wide-layer and the
jump-span cases, whose arcs all carry ilabel 1 (as the metric's chain does): with three
in-labels at most a third of a 320-state window can hold tuples, and the wide layer must
pass 256 of them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import libfst_amd as F
import libfst_amd.fst as FF
import oracle_ffi as O
from test_gpu_parity import bits, check, csr, expected_status, load_blob

pytestmark = pytest.mark.gpu

EAGER = F.FST_SEM_EAGER
TAG = "[libfst_amd route] eager pull: packed cells "


def routes(err):
    return {ln[len(TAG):].strip() for ln in err.splitlines() if ln.startswith(TAG)}


def check_both(blob, seqs, monkeypatch, capfd, want="on"):
    """check() on the default route (asserted: `want`), then with FSTAMD_NO_PACK=1 (off)"""
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    rhs = load_blob(blob)
    labels, offsets = csr(seqs)
    capfd.readouterr()
    check(blob, labels, offsets, EAGER, rhs=rhs)
    assert routes(capfd.readouterr().err) == {want}
    monkeypatch.setenv("FSTAMD_NO_PACK", "1")
    check(blob, labels, offsets, EAGER, rhs=rhs)
    assert routes(capfd.readouterr().err) == {"off"}
    monkeypatch.delenv("FSTAMD_NO_PACK")


def test_metric_shape_small(monkeypatch, capfd):
    # the ambiguous chain at T = 300, B = 12; 1^64 reaches 257 tuples in a layer
    blob = O.freeze(O.gen("ambiguous", 300, 12))
    seqs = [[1] * L for L in range(65)]
    for L, at in ((1, 0), (9, 8), (30, 0), (64, 63), (64, 31)):
        s = [1] * L
        s[at] = 2  # a dead label: every rhs arc has ilabel 1
        seqs.append(s)
    check_both(blob, seqs, monkeypatch, capfd)


def ties_rhs(ns=150):
    """Fan-in 1..12 per state (padded blocks, and further blocks for the hubs), weights half 7
    and half from {0, 1}, finals 0..4 or +inf, sources within [t - 6, t + 3] (so backward
    arcs within the span), parallel arcs s -> t with one ilabel and different olabels"""
    rng = np.random.default_rng(601)
    f = O.Fst()
    for _ in range(ns):
        f.add_state(float(rng.integers(0, 5)) if rng.random() < 0.7 else float("inf"))
    f.start = 0
    run = {}  # arcs of one source with one ilabel: at most 8 fit the key's j
    for t in range(ns):
        il = 1 + t % 3
        fan = 1 + t % 12
        lo, hi = max(0, t - 6), min(ns - 1, t + 3)
        added = 0
        while added < fan:
            s = int(rng.integers(lo, hi + 1))
            if run.get((s, il), 0) >= 8:
                continue
            run[(s, il)] = run.get((s, il), 0) + 1
            w = 7.0 if rng.random() < 0.5 else float(rng.integers(0, 2))
            f.add_arc(s, il, 1 + added, w, t)  # (a repeated source: a parallel arc, its own olabel)
            added += 1
    return f


@pytest.fixture(scope="module")
def ties():
    rng = np.random.default_rng(602)
    blob = O.freeze(ties_rhs())
    seqs = [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, 51)))] for _ in range(300)]
    return blob, seqs


def test_ties_padding_hubs(ties, monkeypatch, capfd):
    blob, seqs = ties
    check_both(blob, seqs, monkeypatch, capfd)


def wide_chain(ns, extra=None):
    """s -> s + d for d = 0..6, all ilabel 1: after k labels the states 0..6k hold tuples.
    extra = (source, span): one more arc of weight 0 spanning `span` states"""
    rng = np.random.default_rng(603)
    f = O.Fst()
    for s in range(ns):
        f.add_state(float(s % 4) if s % 5 else float("inf"))
    f.start = 0
    for s in range(ns):
        for d in range(7):
            w = 7.0 if rng.random() < 0.5 else float(rng.integers(1, 3))
            f.add_arc(s, 1, 1 + d, w, min(ns - 1, s + d))
    if extra:
        f.add_arc(extra[0], 1, 9, 0.0, extra[0] + extra[1])
    return f


def test_wide_layer(monkeypatch, capfd):
    # 50 labels: 301 tuples in the last layer, ranks past 255 (the rank field's high bits)
    blob = O.freeze(wide_chain(330))
    seqs = [[1] * L for L in (50, 50, 49, 47, 43, 44, 20, 1, 0)]
    check_both(blob, seqs, monkeypatch, capfd)


@pytest.mark.parametrize("span,want", [(63, "on"), (64, "off")])
def test_jump_span_bound(span, want, monkeypatch, capfd):
    # delta4 = 4 * (t - s - dlo) must fit a byte: a span of 63 states packs, 64 does not
    blob = O.freeze(wide_chain(330, extra=(0, span)))
    seqs = [[1] * L for L in (1, 2, 3, 4, 5, 8, 13, 21, 30, 40)]
    check_both(blob, seqs, monkeypatch, capfd, want=want)


def device_call(rhs, seqs, max_len, want_work=False):
    labels, offsets = csr(seqs)
    dev = torch.device("cuda", 0)
    lab = torch.as_tensor(labels.astype(np.int32), device=dev)
    off = torch.as_tensor(offsets.astype(np.int64), device=dev)
    n = len(seqs)
    cap = int(offsets[-1]) * 4 + 64
    status = torch.empty(n, dtype=torch.int32, device=dev)
    plen = torch.empty(n, dtype=torch.int32, device=dev)
    poff = torch.empty(n, dtype=torch.int64, device=dev)
    fin = torch.empty(n, dtype=torch.float64, device=dev)
    il = torch.empty(cap, dtype=torch.int32, device=dev)
    ol = torch.empty(cap, dtype=torch.int32, device=dev)
    w = torch.empty(cap, dtype=torch.float64, device=dev)
    cur = torch.zeros(1, dtype=torch.int64, device=dev)
    work = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    desc = FF.FstDeviceBatch(status.data_ptr(), plen.data_ptr(), poff.data_ptr(),
                             fin.data_ptr(), il.data_ptr(), ol.data_ptr(), w.data_ptr(), cap,
                             cur.data_ptr(), work.data_ptr() if want_work else 0)
    opts = FF.FstBatchOptions(0, EAGER, 0)
    rc = F.lib().fst_device_compose_shortest_path(
        rhs.h, C.c_void_p(lab.data_ptr()), C.c_void_p(off.data_ptr()), n, max_len, 1,
        C.byref(opts), C.byref(desc), None)
    assert rc == FF.FST_OK
    torch.cuda.synchronize()
    return (status.cpu().numpy(), plen.cpu().numpy(), poff.cpu().numpy(), fin.cpu().numpy(),
            il.cpu().numpy().view(np.uint32), ol.cpu().numpy().view(np.uint32), w.cpu().numpy(),
            work.cpu().numpy().view(np.uint32))


def assert_device_result(res, ref):
    status, plen, poff, fin, il, ol, w, _ = res
    exp = expected_status(ref)
    assert np.array_equal(status, exp)
    for i in np.nonzero(exp == F.FST_PATH_OK)[0]:
        a, b = int(ref.offsets[i]), int(ref.offsets[i + 1])
        assert plen[i] == b - a, i
        g = slice(int(poff[i]), int(poff[i]) + b - a)
        assert np.array_equal(il[g], ref.ilabels[a:b]), i
        assert np.array_equal(ol[g], ref.olabels[a:b]), i
        assert np.array_equal(bits(w[g]), bits(ref.weights[a:b])), i
        assert bits(fin[i:i + 1])[0] == bits(ref.finals[i:i + 1])[0], i


RING = 40
LONG = 4643  # (LONG + 1) * 7 = 32,508 < 0x7F00 = 32,512 <= (LONG + 2) * 7


@pytest.fixture(scope="module")
def ring():
    """s -> (s + 1) % 40 with weight 7, and a second arc (a loop on s) of weight 0..6; one
    string walks the ring for 4643 labels: its distance reaches 32,501"""
    f = O.Fst()
    for s in range(RING):
        f.add_state(float(s % 3))
    f.start = 0
    for s in range(RING):
        t = (s + 1) % RING
        f.add_arc(s, 1 + t % 3, 1 + s % 7, 7.0, t)
        f.add_arc(s, 1 + s % 3, 8, float(s % 7), s)
    blob = O.freeze(f)
    walk = [1 + ((k + 1) % RING) % 3 for k in range(LONG)]
    rng = np.random.default_rng(604)
    seqs = [walk, walk[:1000], walk[:40] + [1, 1, 2], [], walk[:7]]
    seqs += [[int(x) for x in rng.integers(1, 4, int(rng.integers(0, 30)))] for _ in range(20)]
    labels, offsets = csr(seqs)
    return blob, load_blob(blob), seqs, O.batch_run(blob, labels, offsets, 1, 1)


@pytest.mark.parametrize("claimed,want", [(LONG, "on"), (LONG + 1, "off")])
def test_distance_bound(ring, claimed, want, monkeypatch, capfd):
    blob, rhs, seqs, ref = ring
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    capfd.readouterr()
    res = device_call(rhs, seqs, claimed)
    assert routes(capfd.readouterr().err) == {want}
    assert_device_result(res, ref)
    monkeypatch.setenv("FSTAMD_NO_PACK", "1")
    res = device_call(rhs, seqs, claimed)
    assert routes(capfd.readouterr().err) == {"off"}
    assert_device_result(res, ref)


def test_understated_max_len_hands_the_string_on(ring, monkeypatch, capfd):
    # the caller claims 1000: packed by that bound, and the 4643-label string, whose absent
    # distances could wrap the field, must be handed on
    blob, rhs, seqs, ref = ring
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    capfd.readouterr()
    res = device_call(rhs, seqs, 1000)
    assert routes(capfd.readouterr().err) == {"on"}
    assert_device_result(res, ref)


def test_work_counters_ignore_padding_copies(ties, monkeypatch, capfd):
    # tuples and relaxations per string: the padding copies of a block's first record must
    # not count
    blob, seqs = ties
    rhs = load_blob(blob)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    max_len = max(len(s) for s in seqs)
    capfd.readouterr()
    packed = device_call(rhs, seqs, max_len, want_work=True)
    assert routes(capfd.readouterr().err) == {"on"}
    monkeypatch.setenv("FSTAMD_NO_PACK", "1")
    plain = device_call(rhs, seqs, max_len, want_work=True)
    assert routes(capfd.readouterr().err) == {"off"}
    assert np.array_equal(packed[0], plain[0])
    assert plain[7][1::2].sum() > 0
    assert np.array_equal(packed[7], plain[7])
