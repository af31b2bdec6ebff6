"""GPU: the device-resident lhs entry (fst_device_compose_shortest_path_lhs) and its prepare
kernel.  The inputs are torch tensors on the device; the expected result is the host lhs batch
entry's on the same items, bit for bit (that entry is pinned to the oracle by
tests/test_gpu_lhs_batch.py), plus one oracle comparison of this entry's own.

What is under test is what the prepare kernel derives on the device and run_lhs_shard derives
on the host: descriptors, local arc offsets, flags, the largest out-degree, the two eager item
lists, and the per-item validation the host entry does before it starts.
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
from test_gpu_lhs_batch import batch_of, bits, expect, got_item, weighted_dag
from test_gpu_parity import load_blob, random_rhs

pytestmark = pytest.mark.gpu

EAGER, LAZY = F.FST_SEM_EAGER, F.FST_SEM_LAZY
SEMS = [LAZY, EAGER]
INF = math.inf
OK, UNSUPPORTED, FULL = F.FST_PATH_OK, F.FST_PATH_UNSUPPORTED, F.FST_PATH_OUTPUT_FULL


def dev_tensor(a: np.ndarray):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.as_tensor(a.view(signed) if signed else a, device="cuda:0")


class DeviceLhs:
    """An LhsBatch uploaded as torch tensors, and its FstLhsBatch of device pointers."""

    FIELDS = ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
              "weights", "nextstates")

    def __init__(self, lhs: F.LhsBatch):
        self.num = len(lhs)
        self.t = {k: dev_tensor(getattr(lhs, k)) for k in self.FIELDS}
        self.cs = FF.FstLhsBatch(self.num, *[self.t[k].data_ptr() if self.t[k].numel() else None
                                             for k in self.FIELDS])


class DeviceOut:
    def __init__(self, num, cap):
        dev = "cuda:0"
        self.num, self.cap = num, cap
        self.status = torch.full((max(num, 1),), -1, dtype=torch.int32, device=dev)
        self.plen = torch.zeros(max(num, 1), dtype=torch.int32, device=dev)
        self.poff = torch.zeros(max(num, 1), dtype=torch.int64, device=dev)
        self.fin = torch.zeros(max(num, 1), dtype=torch.float64, device=dev)
        self.il = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
        self.ol = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
        self.w = torch.zeros(max(cap, 1), dtype=torch.float64, device=dev)
        self.cur = torch.full((1,), 12345, dtype=torch.int64, device=dev)
        self.desc = FF.FstDeviceBatch(self.status.data_ptr(), self.plen.data_ptr(),
                                      self.poff.data_ptr(), self.fin.data_ptr(),
                                      self.il.data_ptr(), self.ol.data_ptr(), self.w.data_ptr(),
                                      cap, self.cur.data_ptr(), 0)

    def items(self):
        """Per item what got_item gives for a host result."""
        st, ln, off = self.status.cpu().numpy(), self.plen.cpu().numpy(), self.poff.cpu().numpy()
        fin = self.fin.cpu().numpy()
        il = self.il.cpu().numpy().view(np.uint32)
        ol = self.ol.cpu().numpy().view(np.uint32)
        w = self.w.cpu().numpy()
        out = []
        for i in range(self.num):
            if int(st[i]) != OK:
                out.append((int(st[i]),))
                continue
            a0, a1 = int(off[i]), int(off[i]) + int(ln[i])
            assert a1 <= self.cap
            out.append((OK, il[a0:a1].tolist(), ol[a0:a1].tolist(), bits(w[a0:a1]).tolist(),
                        int(bits(fin[i:i + 1])[0])))
        return out

    def cursor(self):
        return int(self.cur.cpu()[0])


def run_device(rhs, lhs: F.LhsBatch, sem, n=1, cap=None, dlhs=None):
    d = dlhs or DeviceLhs(lhs)
    out = DeviceOut(d.num, 16 * len(lhs.ilabels) + 1024 if cap is None else cap)
    opts = FF.FstBatchOptions(0, sem, 0, 0, 0)
    rc = F.lib().fst_device_compose_shortest_path_lhs(rhs.h, C.byref(d.cs), n, C.byref(opts),
                                                      C.byref(out.desc), None)
    assert rc == FF.FST_OK
    # (no torch synchronisation: the call itself synchronises its stream)
    return out


def host_items(rhs, lhs: F.LhsBatch, sem, n=1):
    got = F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, n, sem)
    return [got_item(got, i) for i in range(len(lhs))]


def check_against_host(rhs, fsts, sem, n=1):
    lhs = batch_of(fsts)
    dev, host = run_device(rhs, lhs, sem, n).items(), host_items(rhs, lhs, sem, n)
    for i, (d, h) in enumerate(zip(dev, host)):
        assert d == h, (i, sem, n)
    return dev


def route(capfd):
    """(columns of the last `lhs batch:` route line, its replay count)."""
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lhs batch:" in ln]
    assert lines, err
    m = re.search(r"lhs batch: (\w+) items (\d+) \| (.*) \| replay (\d+)", lines[-1])
    return m.group(1), int(m.group(2)), m.group(3), int(m.group(4)), err


# ---- 1. random graphs --------------------------------------------------------------------------

def random_case(seed):
    rng = np.random.default_rng(7000 + seed)
    frac = seed % 2 == 1
    rhs_fst = random_rhs(rng, int(rng.integers(1, 20)), int(rng.integers(1, 80)), 3, eps=True,
                         frac=frac)
    blob = O.freeze(rhs_fst)
    fsts = [random_rhs(rng, int(rng.integers(1, 11)), int(rng.integers(1, 31)), 3, eps=True,
                       frac=frac) for _ in range(64)]
    return blob, load_blob(blob), fsts


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("seed", range(3))
def test_random_graphs(seed, sem):
    blob, rhs, fsts = random_case(seed)
    dev = check_against_host(rhs, fsts, sem)
    if seed == 0:  # this entry's own oracle comparison
        for i, f in enumerate(fsts):
            assert dev[i] == expect(f, blob, sem), (i, sem)
    for n in (0, 2):
        check_against_host(rhs, fsts[:16], sem, n=n)


# ---- 2. out-degrees ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_out_degrees(sem, monkeypatch, capfd):
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    rng = np.random.default_rng(41)
    rhs = load_blob(O.freeze(random_rhs(rng, 6, 40, 4, eps=True)))
    fsts = []
    for deg in (1, 63, 64, 65, 130):
        f = O.Fst(start=0, finals=[INF, 0.0, 1.0, INF], arcs=[[], [], [], []])
        for k in range(deg):
            ol = 0 if k % 3 == 1 else int(rng.integers(1, 5))
            f.add_arc(0, int(rng.integers(0, 5)), ol, float(rng.integers(0, 4)),
                      int(rng.integers(1, 4)))
        f.add_arc(3, 1, 2, 1.0, 1)
        f.add_arc(2, 0, 0, 0.0, 3)
        fsts.append(f)
        fsts.append(O.Fst(start=0, finals=[INF, 0.0],
                          arcs=[[(1, int(rng.integers(1, 5)), 0.5, 1)], []]))
    big = fsts[8]       # the 130-arc item sizes the lazy table wherever it sits
    rest = fsts[:8] + fsts[9:]
    for order in (fsts, [big] + rest, rest + [big]):
        capfd.readouterr()
        check_against_host(rhs, order, sem)
        assert "lhs prepare: items 10 invalid 0 max out-degree 130 " in capfd.readouterr().err
    # without the large item the maximum is the next one's
    capfd.readouterr()
    check_against_host(rhs, rest, sem)
    assert "lhs prepare: items 9 invalid 0 max out-degree 65 " in capfd.readouterr().err


# ---- 3. flags ----------------------------------------------------------------------------------------

def flag_items():
    rng = np.random.default_rng(92)
    plain = lambda: weighted_dag(rng, [0.0, 1.0, 2.5], [0.0, 1.0])

    def with_arc_weight(w):
        f = plain()
        s = next(s for s, al in enumerate(f.arcs) if al)
        f.arcs[s][0] = f.arcs[s][0][:2] + (w,) + f.arcs[s][0][3:]
        return f

    def with_final(w):
        f = plain()
        f.finals[5] = w
        return f

    eps_out = plain()
    s = next(s for s, al in enumerate(eps_out.arcs) if al)
    eps_out.arcs[s][0] = (eps_out.arcs[s][0][0], 0) + eps_out.arcs[s][0][2:]
    no_eps = O.Fst(start=0, finals=[INF, 0.5], arcs=[[(1, 2, 1.0, 1), (2, 1, 0.0, 1)], []])
    items = [with_arc_weight(-1.0), with_arc_weight(-0.0), with_final(-0.0),
             with_arc_weight(INF), with_arc_weight(math.nan), with_final(math.nan), eps_out,
             no_eps]
    return items + [plain() for _ in range(4)]


@pytest.mark.parametrize("sem", SEMS)
def test_flags_and_route(sem, monkeypatch, capfd):
    rng = np.random.default_rng(93)
    rhs = load_blob(O.freeze(random_rhs(rng, 7, 45, 3, eps=True)))
    fsts = flag_items()
    lhs = batch_of(fsts)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    capfd.readouterr()
    host = host_items(rhs, lhs, sem)
    host_route = route(capfd)[:4]
    dev = run_device(rhs, lhs, sem).items()
    dev_route = route(capfd)
    assert dev == host
    assert [host[4][0], host[5][0]] == [UNSUPPORTED, UNSUPPORTED]          # the NaN items
    assert dev_route[:4] == host_route
    if sem == EAGER:
        assert host_route[3] == 4            # negative, -0.0 weight, -0.0 final, +inf arc
    assert re.search(r"lhs prepare: items 12 invalid 0 max out-degree \d+ \| nonneg 8 replay 4",
                     dev_route[4])


# ---- 4. many items per wave ----------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_many_items_per_wave(sem, monkeypatch, capfd):
    rng = np.random.default_rng(77)
    rhs = load_blob(O.freeze(random_rhs(rng, 8, 30, 3, eps=True)))
    fsts = [random_rhs(rng, int(rng.integers(1, 6)), int(rng.integers(1, 9)), 3, eps=True)
            for _ in range(3000)]
    fsts[17].arcs[0].append((1, 1, -0.0, 0))      # replay items spread over the list
    fsts[1500].arcs[0].append((1, 1, -2.0, 0))
    fsts[2999].finals[0] = -0.0
    lhs = batch_of(fsts)
    host = host_items(rhs, lhs, sem)
    monkeypatch.setenv("FSTAMD_GRAPH_GRID", "2")   # two waves prepare (and run) 3,000 items
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    capfd.readouterr()
    dev = run_device(rhs, lhs, sem).items()
    assert F.last_launch_stats().grid <= 2
    # the totals: exact whatever wave saw the item
    want = "lhs prepare: items 3000 invalid 0 max out-degree %d | nonneg 2997 replay 3" % int(
        np.diff(lhs.arc_offsets.astype(np.int64)).max())
    assert want in capfd.readouterr().err
    for i, (d, h) in enumerate(zip(dev, host)):
        assert d == h, (i, sem)


# ---- 5. zero-state and one-state items --------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_zero_and_one_state_items(sem):
    rng = np.random.default_rng(5)
    rhs = load_blob(O.freeze(O.Fst(start=0, finals=[1.5, 0.0],
                                   arcs=[[(1, 1, 0.25, 1), (2, 3, 0.0, 1)], [(1, 1, 0.0, 1)]])))
    none = lambda: O.Fst()
    one = lambda: O.Fst(start=0, finals=[0.5], arcs=[[]])
    loop = lambda: O.Fst(start=0, finals=[0.25], arcs=[[(1, 2, 1.0, 0)]])
    mid = [random_rhs(rng, 3, 6, 2, eps=True) for _ in range(4)]
    fsts = [none(), one(), mid[0], mid[1], none(), loop(), one(), mid[2], mid[3], one(), none()]
    check_against_host(rhs, fsts, sem)
    check_against_host(rhs, [none(), none()], sem)
    check_against_host(rhs, [one()], sem)
    empty = run_device(rhs, batch_of([]), sem)       # no items: OK, and the cursor is reset
    assert empty.items() == [] and empty.cursor() == 0


# ---- 6. invalid items ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("defect", ["start", "nextstate", "arc_offset"])
def test_invalid_item_in_the_middle(defect, sem, monkeypatch, capfd):
    """The defect sits in the middle item, so what a missing check would read lies inside the
    batch's own arrays: a wrong answer, never an access outside the buffers."""
    _, rhs, fsts = random_case(1)
    fsts = fsts[:9]
    victim = O.Fst(start=0, finals=[INF, INF, 0.0],
                   arcs=[[(1, 1, 0.5, 1), (2, 2, 0.0, 1)], [(1, 2, 1.0, 2)], [(1, 1, 0.0, 0)]])
    good = fsts[:4] + fsts[5:]
    host = host_items(rhs, batch_of(good), sem)
    lhs = batch_of(fsts[:4] + [victim] + fsts[5:])
    s0, a0 = int(lhs.state_offsets[4]), int(lhs.arc_offsets[int(lhs.state_offsets[4])])
    if defect == "start":
        lhs.start[4] = 3                         # the state count
    elif defect == "nextstate":
        lhs.nextstates[a0 + 2] = 3
    else:
        lhs.arc_offsets[s0 + 1] = a0 + 4         # then state 1's arcs "end" before they begin
        assert lhs.arc_offsets[s0 + 2] < lhs.arc_offsets[s0 + 1]
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    capfd.readouterr()
    dev = run_device(rhs, lhs, sem).items()
    assert dev[4] == (UNSUPPORTED,)
    assert dev[:4] + dev[5:] == host
    assert "lhs prepare: items 9 invalid 1 " in capfd.readouterr().err


@pytest.mark.parametrize("sem", SEMS)
def test_decreasing_state_offsets_invalidate_the_batch(sem, monkeypatch, capfd):
    """state_offsets = [.., a, b < a, c, ..]: the item in the middle is invalid on its own, and
    the items around it would pass their own checks while sharing states -- and words of the
    local-offset workspace, which the general kernels would then read as written by either.
    No item of such a batch is run.  (Every offset stays inside the batch's own arrays.)"""
    _, rhs, fsts = random_case(2)
    fsts = fsts[:9]
    lhs = batch_of(fsts)
    assert int(lhs.state_offsets[5]) - int(lhs.state_offsets[4]) >= 1
    lhs.state_offsets[5] = lhs.state_offsets[3]     # item 4: s0 > s1; items 3 and 5 overlap
    assert lhs.state_offsets[5] < lhs.state_offsets[4] <= lhs.state_offsets[6]
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    capfd.readouterr()
    dev = run_device(rhs, lhs, sem)
    assert dev.items() == [(UNSUPPORTED,)] * 9 and dev.cursor() == 0
    err = capfd.readouterr().err
    assert "lhs prepare: items 9 invalid 9 max out-degree 0 " in err
    assert "decreasing state offsets 1" in err
    # n == 0 is EMPTY before anything else, as in the single call
    assert run_device(rhs, lhs, sem, n=0).items() == [(F.FST_PATH_EMPTY,)] * 9
    # and the same tensors' batch is answered once the offsets are in order again
    check_against_host(rhs, fsts, sem)


# ---- 7. a small arena -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_small_arena(sem):
    rng = np.random.default_rng(23)
    spec = SY.tagger()
    rhs = load_blob(O.freeze(O.Fst(start=spec[1], finals=spec[2], arcs=spec[3])))
    fsts = []
    for t in SY.utterances(rng, 40, 1, 24):
        cn = SY.confusion_network(rng, t, 3, 0.15)
        fsts.append(O.Fst(start=cn[0], finals=cn[1], arcs=cn[2]))
    lhs = batch_of(fsts)
    host = F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, 1, sem)
    need = int(host.offsets[-1])
    dlhs = DeviceLhs(lhs)
    small = run_device(rhs, lhs, sem, cap=need // 3, dlhs=dlhs)
    st = small.status.cpu().numpy()
    assert set(st.tolist()) == {OK, FULL} and small.cursor() == need
    for i, e in enumerate(small.items()):        # what fitted is right
        if e[0] == OK:
            assert e == got_item(host, i)
    full = run_device(rhs, lhs, sem, cap=small.cursor(), dlhs=dlhs)
    assert full.items() == [got_item(host, i) for i in range(len(fsts))]
    assert full.cursor() == need


# ---- 8. device-resident pipeline ----------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_device_resident_pipeline(sem):
    rng = np.random.default_rng(31)
    specs = [SY.tagger(), SY.verbalizer()]
    stages = [load_blob(O.freeze(O.Fst(start=s[1], finals=s[2], arcs=s[3]))) for s in specs]
    fsts = []
    for t in SY.utterances(rng, 24, 1, 12):
        cn = SY.confusion_network(rng, t, 4, 0.2)
        fsts.append(O.Fst(start=cn[0], finals=cn[1], arcs=cn[2]))
    lhs = batch_of(fsts)
    want = F.normalize_lhs_batch(stages, lhs, sem)
    L, num, dev = F.lib(), len(fsts), "cuda:0"
    opts = FF.FstBatchOptions(0, sem, 0, 0, 0)
    s1 = run_device(stages[0], lhs, sem)
    used = s1.cursor()
    nlab = torch.zeros(used + num, dtype=torch.int32, device=dev)
    noff = torch.zeros(num + 1, dtype=torch.int64, device=dev)
    pst = torch.zeros(num, dtype=torch.int32, device=dev)
    max_len = C.c_uint32(0)
    assert L.fst_device_project_output(C.byref(s1.desc), num, nlab.data_ptr(), noff.data_ptr(),
                                       pst.data_ptr(), C.byref(max_len), None) == FF.FST_OK
    assert pst.cpu().numpy().tolist() == [OK] * num
    s2 = DeviceOut(num, 8 * (used + num) + 64)
    assert L.fst_device_compose_shortest_path(stages[1].h, nlab.data_ptr(), noff.data_ptr(), num,
                                              max_len.value, 1, C.byref(opts), C.byref(s2.desc),
                                              None) == FF.FST_OK
    cap = 16 * (used + num)
    text = torch.zeros(cap, dtype=torch.uint8, device=dev)
    toff = torch.zeros(num + 1, dtype=torch.int64, device=dev)
    tst = torch.zeros(num, dtype=torch.int32, device=dev)
    tw = torch.zeros(num, dtype=torch.float64, device=dev)
    total = C.c_uint64(0)
    assert L.fst_device_emit_text(C.byref(s2.desc), num, text.data_ptr(), cap, toff.data_ptr(),
                                  tst.data_ptr(), tw.data_ptr(), C.byref(total),
                                  None) == FF.FST_OK
    assert total.value == int(want.offsets[-1]) <= cap
    assert tst.cpu().numpy().tolist() == want.status.tolist() == [OK] * num
    assert toff.cpu().numpy().view(np.uint64).tolist() == want.offsets.tolist()
    assert text.cpu().numpy()[:total.value].tobytes() == want.text.tobytes()
    assert bits(tw.cpu().numpy()).tolist() == bits(want.total_weight).tolist()
