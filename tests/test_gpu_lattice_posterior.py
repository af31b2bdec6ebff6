"""GPU: fst_posterior_lhs_batch / fst_device_posterior_lhs against tests/posterior_model.py.

Every case runs at both tiers (the default LDS budget, and FSTAMD_POSTERIOR_LDS=0: every item
through the workgroup tier).  Values are compared within the tolerances derived in
posterior_model.tolerances, per item from the item itself; where no logadd meets two finite
operands they are compared bit for bit.  The largest observed error / tolerance ratio of every
case goes to profiles/lattice_posterior/accuracy.json (the 2-ulp figure for the device's exp and
log1p is the documented one, not measured: a ratio above 1 would be a finding)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import libfst_amd as F
import libfst_amd.fst as FF
import posterior_model as PM
from libfst_amd import synthetic as SY
from test_gpu_lattice_sp import tagger_blob
from test_gpu_lhs_device import DeviceLhs
from test_gpu_parity import load_blob
from test_posterior_model import random_item

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
OK, EMPTY, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED
U64 = np.uint64
RATIOS = {}


@pytest.fixture(params=["default", "0"], autouse=True)
def tier(request, monkeypatch):
    if request.param != "default":
        monkeypatch.setenv("FSTAMD_POSTERIOR_LDS", request.param)
    return request.param


@pytest.fixture(scope="module", autouse=True)
def accuracy_record():
    yield
    path = os.path.join(REPO, "profiles", "lattice_posterior", "accuracy.json")
    rec = {"what": "largest |device - model| / tolerance per test case and tier "
                   "(tests/test_gpu_lattice_posterior.py); the bound holds while every ratio is <= 1",
           "ratios": {k: float("%.4g" % v) for k, v in sorted(RATIOS.items())}}
    try:
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write("\n")
    except OSError:
        pass


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(U64)


def arrays(res):
    return {k: getattr(res, k).copy() for k in ("status", "total", "alpha", "beta", "arc_cost")}


def same(a, b):
    for k in ("status", "total", "alpha", "beta", "arc_cost"):
        assert a[k].tobytes() == b[k].tobytes(), k


def run(fsts, **kw):
    lhs = F.LhsBatch.from_fsts(fsts)
    got = F.posterior_lhs_batch(lhs, **kw)
    assert F.last_launch_stats().engine == 16
    assert len(got) == len(fsts) and len(got.alpha) == len(lhs.final_weights) == len(got.beta)
    assert len(got.arc_cost) == len(lhs.weights)
    return lhs, arrays(got)


def compare(case, fsts, lhs, got, model, exact=False, tier=""):
    """Statuses equal; a non-OK item all +inf; an OK item within its tolerances (or bit for bit),
    with +inf exactly where the model has +inf."""
    worst = 0.0
    for i, (fst, m) in enumerate(zip(fsts, model)):
        s0, s1 = int(lhs.state_offsets[i]), int(lhs.state_offsets[i + 1])
        a0, a1 = int(lhs.arc_offsets[s0]), int(lhs.arc_offsets[s1])
        assert int(got["status"][i]) == m[0], (case, i, int(got["status"][i]), m[0])
        parts = [(got["total"][i:i + 1], [m[1]], 0), (got["alpha"][s0:s1], m[2], 0),
                 (got["beta"][s0:s1], m[3], 0), (got["arc_cost"][a0:a1], m[4], 1)]
        if m[0] != OK:
            for g, _, _ in parts:
                assert np.all(g == INF), (case, i)
            continue
        tols = PM.tolerances(fst, m)
        for g, w, which in parts:
            w = np.asarray(w, np.float64)
            assert len(g) == len(w)
            assert np.array_equal(g == INF, w == INF), (case, i, which)
            if exact:
                assert bits(g).tolist() == bits(w).tolist(), (case, i, which)
                continue
            fin = w != INF
            if fin.any():
                err = float(np.max(np.abs(g[fin] - w[fin])))
                print(f"{case}[{tier}] item {i} part {which}: err {err:.3g} tol {tols[which]:.3g}")
                worst = max(worst, err / tols[which])
                assert err <= tols[which], (case, i, which, err, tols[which])
    if not exact:
        key = f"{case}[{tier}]"
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)


def route_line(capfd):
    err = capfd.readouterr().err
    lines = [ln for ln in err.split("\n") if "lattice posterior:" in ln]
    assert lines, err
    m = re.search(r"lattice posterior: items (\d+) \| lds (\d+) hbm (\d+) \| [0-9.]+ ms", lines[-1])
    assert m, lines[-1]
    return tuple(int(x) for x in m.groups())


# ---- 1. known answers and statuses ---------------------------------------------------------------

def test_known_answers_and_statuses(tier):
    # the status items between the known ones: a neighbour's failure leaves an item untouched
    fsts, want = [], []
    for k in range(max(len(PM.KNOWN), len(PM.STATUSES))):
        if k < len(PM.STATUSES):
            fsts.append(PM.STATUSES[k][0])
            want.append(PM.STATUSES[k][1])
        if k < len(PM.KNOWN):
            fsts.append(PM.KNOWN[k][0])
            want.append(PM.KNOWN[k][1])
    lhs, got = run(fsts)
    assert got["status"].tolist() == want
    compare("known", fsts, lhs, got, PM.posterior_batch(fsts), tier=tier)
    # ... and against the hand-written answers themselves
    known = [k[0] for k in PM.KNOWN]
    lhs, got = run(known)
    compare("known-by-hand", known, lhs, got, [k[1:] for k in PM.KNOWN], tier=tier)


# ---- 2. bit-exact where it must be ---------------------------------------------------------------

def chain(n_arcs, dead=False, unreachable=False, inf_arcs=False):
    """A single-path item: a chain of n_arcs arcs with non-dyadic weights and a negative final.
    dead: every fifth state has an arc to a dead-end state; unreachable: extra states with arcs
    into the chain; inf_arcs: a parallel arc of +inf beside every third arc."""
    n = n_arcs + 1
    finals = [INF] * n
    finals[n - 1] = -0.7
    arcs = [[] for _ in range(n)]
    for s in range(n_arcs):
        if inf_arcs and s % 3 == 0:
            arcs[s].append((9, 9, INF, s + 1))
        arcs[s].append((s % 200 + 1, 1, 0.1 * (s % 17) - 0.45, s + 1))
    extra = []
    if dead:
        for s in range(0, n_arcs, 5):
            arcs[s].append((7, 7, 0.3, n + len(extra)))
            extra.append([])
    if unreachable:
        for s in range(0, n, 4):
            extra.append([(8, 8, 0.2, s)])
    return 0, finals + [INF] * len(extra), arcs + extra


SINGLE = [chain(n, **kw) for n in (1, 2, 63, 64, 65, 300)
          for kw in ({}, {"dead": True}, {"unreachable": True}, {"inf_arcs": True},
                     {"dead": True, "unreachable": True, "inf_arcs": True})]


@pytest.fixture(scope="module")
def single_model():
    return PM.posterior_batch(SINGLE)


def test_single_path_items_are_bit_exact(single_model, tier):
    lhs, got = run(SINGLE)
    assert np.all(got["status"] == OK)
    compare("single", SINGLE, lhs, got, single_model, exact=True)


# ---- 3. fold order -------------------------------------------------------------------------------

def fold_item(fan, seed):
    """State T = 1 has `fan` in-arcs from sources of different depths.  Within an item the arc
    index follows the source's id (CSR), so the sources' ids are shuffled against their depths:
    the order of the fold differs from the order of the depths and from any order the fill's
    atomics may give.  Weights spread over 30 units, so the order changes the bits."""
    rng = np.random.default_rng(seed)
    depth = rng.integers(1, 6, fan)            # source k hangs on a chain of depth[k] arcs
    n_src = int(fan * 0.75)                    # some sources carry two parallel arcs
    finals, arcs = [INF, 0.25], [[], []]

    def new_state():
        finals.append(INF)
        arcs.append([])
        return len(finals) - 1

    src = []
    for k in rng.permutation(n_src):
        s = new_state()
        src.append((s, int(depth[k])))
    for s, d in src:                           # a chain of d arcs from the start to s
        prev = 0
        for _ in range(d - 1):
            mid = new_state()
            arcs[prev].append((1, 1, float(rng.uniform(-1, 1)), mid))
            prev = mid
        arcs[prev].append((1, 1, float(rng.uniform(-1, 1)), s))
    for j in range(fan):
        s = src[j % n_src][0]
        arcs[s].append((2, 2, float(rng.uniform(-15, 15)), 1))
    return 0, finals, arcs


FOLD = [fold_item(20, 1), fold_item(40, 2), fold_item(90, 3)]


@pytest.fixture(scope="module")
def fold_runs():
    return {"model": PM.posterior_batch(FOLD), "runs": {}}


def test_fold_order(fold_runs, tier):
    lhs, got = run(FOLD)
    assert np.all(got["status"] == OK)
    compare("fold", FOLD, lhs, got, fold_runs["model"], tier=tier)
    for _ in range(19):
        same(got, run(FOLD)[1])
    fold_runs["runs"][tier] = got
    if len(fold_runs["runs"]) == 2:            # the two tiers give the same bytes
        same(fold_runs["runs"]["default"], fold_runs["runs"]["0"])


def test_fold_order_changes_the_bits():
    """The test above can tell orders apart: folding T's in-arcs backwards moves alpha(T)."""
    fst = FOLD[1]
    m = PM.posterior_item(fst)
    terms = [(m[2][s] + a[2]) for s in range(len(fst[1])) for a in fst[2][s] if a[3] == 1]
    fwd = rev = INF
    for v in terms:
        fwd = PM.logadd(fwd, v)
    for v in reversed(terms):
        rev = PM.logadd(rev, v)
    assert fwd == m[2][1] and rev != fwd


# ---- 4. wide levels and high degree --------------------------------------------------------------

def fan(width, seed):
    """start -> `width` states -> one final state: a level of `width`, a start of that many
    out-arcs, a last state of that many in-arcs."""
    rng = np.random.default_rng(seed)
    n = width + 2
    finals = [INF] * n
    finals[n - 1] = 0.5
    arcs = [[] for _ in range(n)]
    for k in rng.permutation(width):
        arcs[0].append((1, 1, float(rng.uniform(-2, 2)), 1 + int(k)))
    for k in range(width):
        arcs[1 + k].append((2, 2, float(rng.uniform(-2, 2)), n - 1))
    return 0, finals, arcs


def diamonds(k):
    finals = [INF] * (3 * k + 1)
    finals[3 * k] = 0.0
    arcs = [[] for _ in range(3 * k + 1)]
    for j in range(k):
        a, b, c, d = 3 * j, 3 * j + 1, 3 * j + 2, 3 * j + 3
        arcs[a] = [(1, 1, 0.3, b), (2, 2, 0.7, c)]
        arcs[b] = [(3, 3, 0.2, d)]
        arcs[c] = [(4, 4, 0.1, d)]
    return 0, finals, arcs


WIDE = [fan(65, 1), fan(257, 2), fan(300, 3), fan(33, 4), fan(32, 5), diamonds(150)]


@pytest.fixture(scope="module")
def wide_model():
    return PM.posterior_batch(WIDE)


def test_wide_levels_and_high_degree(wide_model, tier):
    lhs, got = run(WIDE)
    assert np.all(got["status"] == OK)
    compare("wide", WIDE, lhs, got, wide_model, tier=tier)


# ---- 5. random acyclic items ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def randoms():
    rng = np.random.default_rng(77)
    fsts = [random_item(rng, 1, 40, 0.08) for _ in range(200)]
    return fsts, PM.posterior_batch(fsts)


def test_random_items(randoms, tier):
    fsts, model = randoms
    assert sum(m[0] == OK for m in model) > 120 and sum(m[0] == EMPTY for m in model) > 2
    lhs, got = run(fsts)
    compare("random", fsts, lhs, got, model, tier=tier)


# ---- 6. tier routing -----------------------------------------------------------------------------

def test_tier_routing(randoms, monkeypatch, capfd):
    fsts = randoms[0][:20] + [diamonds(140)] + randoms[0][20:30]    # 421 states: 13 KiB of tables
    monkeypatch.delenv("FSTAMD_POSTERIOR_LDS", raising=False)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    _, a = run(fsts)
    items, lds, hbm = route_line(capfd)
    assert items == len(fsts) and lds + hbm == items and hbm == 1
    monkeypatch.setenv("FSTAMD_POSTERIOR_LDS", "0")
    _, b = run(fsts)
    items, lds, hbm = route_line(capfd)
    n_start = sum(f[0] is not None and len(f[1]) > 0 for f in fsts)
    assert hbm == n_start and lds == items - n_start
    same(a, b)


# ---- 7. sharding and entries ---------------------------------------------------------------------

class DevicePost:
    SENTINEL = 777.0

    def __init__(self, num, ns, na, with_ab=True):
        dev = "cuda:0"
        self.status = torch.full((max(num, 1),), -1, dtype=torch.int32, device=dev)
        mk = lambda n: torch.full((max(n, 1),), self.SENTINEL, dtype=torch.float64, device=dev)
        self.total, self.alpha, self.beta, self.arc_cost = mk(num), mk(ns), mk(ns), mk(na)
        self.num, self.ns, self.na = num, ns, na
        self.desc = FF.FstDevicePosteriors(self.status.data_ptr(), self.total.data_ptr(),
                                           self.alpha.data_ptr() if with_ab else None,
                                           self.beta.data_ptr() if with_ab else None,
                                           self.arc_cost.data_ptr())

    def arrays(self):
        return {"status": self.status.cpu().numpy()[:self.num],
                "total": self.total.cpu().numpy()[:self.num],
                "alpha": self.alpha.cpu().numpy()[:self.ns],
                "beta": self.beta.cpu().numpy()[:self.ns],
                "arc_cost": self.arc_cost.cpu().numpy()[:self.na]}


def run_device(d: DeviceLhs, out: DevicePost):
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    rc = F.lib().fst_device_posterior_lhs(C.byref(d.cs), C.byref(opts), C.byref(out.desc), None)
    assert rc == FF.FST_OK
    assert F.last_launch_stats().engine == 16
    return out.arrays()        # (no torch synchronisation: the call synchronises its stream)


def test_shards_do_not_show(randoms, tier):
    fsts = randoms[0] + WIDE[:2]
    assert len(fsts) % 3
    _, one = run(fsts)
    _, three = run(fsts, devices=[0], shards=3)
    same(one, three)
    _, many = run(fsts, devices=[0], shards=7)
    same(one, many)


def test_device_entry(randoms, tier):
    fsts = randoms[0] + [PM.STATUSES[k][0] for k in range(len(PM.STATUSES))] + WIDE[:2]
    lhs, host = run(fsts)
    ns, na = len(lhs.final_weights), len(lhs.weights)
    d = DeviceLhs(lhs)
    same(host, run_device(d, DevicePost(len(fsts), ns, na)))
    # alpha and beta NULL: the same arc costs, and nothing of the two is written
    out = DevicePost(len(fsts), ns, na, with_ab=False)
    got = run_device(d, out)
    for k in ("status", "total", "arc_cost"):
        assert got[k].tobytes() == host[k].tobytes(), k
    assert np.all(got["alpha"] == DevicePost.SENTINEL) and np.all(got["beta"] == DevicePost.SENTINEL)


def test_device_entry_refused_item(randoms, tier):
    fsts = randoms[0][:60]
    lhs, host = run(fsts)
    ns = np.diff(lhs.state_offsets.astype(np.int64))
    victim = next(i for i in range(5, 60) if ns[i] > 1 and
                  lhs.arc_offsets[int(lhs.state_offsets[i + 1])] > lhs.arc_offsets[int(lhs.state_offsets[i])])
    bad = F.LhsBatch(lhs.state_offsets, lhs.start, lhs.final_weights, lhs.arc_offsets, lhs.ilabels,
                     lhs.olabels, lhs.weights, lhs.nextstates.copy())
    s0, s1 = int(lhs.state_offsets[victim]), int(lhs.state_offsets[victim + 1])
    a0, a1 = int(lhs.arc_offsets[s0]), int(lhs.arc_offsets[s1])
    bad.nextstates[a0] = len(fsts[victim][1])                 # one past the item's last state
    got = run_device(DeviceLhs(bad), DevicePost(60, len(lhs.final_weights), len(lhs.weights)))
    assert got["status"][victim] == UNSUPPORTED and got["total"][victim] == INF
    # only status and total are written for it: its ranges cannot be trusted
    S = DevicePost.SENTINEL
    assert np.all(got["alpha"][s0:s1] == S) and np.all(got["beta"][s0:s1] == S)
    assert np.all(got["arc_cost"][a0:a1] == S)
    keep_s = np.ones(len(lhs.final_weights), bool)
    keep_s[s0:s1] = False
    keep_a = np.ones(len(lhs.weights), bool)
    keep_a[a0:a1] = False
    keep_i = np.arange(60) != victim
    for k, keep in (("status", keep_i), ("total", keep_i), ("alpha", keep_s), ("beta", keep_s),
                    ("arc_cost", keep_a)):
        assert got[k][keep].tobytes() == host[k][keep].tobytes(), k


def test_device_entry_decreasing_state_offsets(tier):
    fsts = [k[0] for k in PM.KNOWN]
    lhs = F.LhsBatch.from_fsts(fsts)
    d = DeviceLhs(lhs)
    d.t["state_offsets"][2] = d.t["state_offsets"][1] - 1
    got = run_device(d, DevicePost(len(fsts), len(lhs.final_weights), len(lhs.weights)))
    assert np.all(got["status"] == UNSUPPORTED) and np.all(got["total"] == INF)
    S = DevicePost.SENTINEL
    assert np.all(got["alpha"] == S) and np.all(got["beta"] == S) and np.all(got["arc_cost"] == S)


def start_mass(lhs, got, i):
    """sum over the start's out-arcs of exp(-arc_cost), plus exp(-(final(start) - total))."""
    s = int(lhs.state_offsets[i]) + int(lhs.start[i])
    a0, a1 = int(lhs.arc_offsets[s]), int(lhs.arc_offsets[s + 1])
    mass = sum(math.exp(-c) for c in got["arc_cost"][a0:a1].tolist() if c != INF)
    f = float(lhs.final_weights[s])
    if f != INF:
        mass += math.exp(-(f - float(got["total"][i])))
    return mass, a1 - a0


def test_compose_output_runs_end_to_end(tier):
    texts = SY.utterances(np.random.default_rng(15), 64, 4, 12)
    lat = F.compose_frozen_batch(load_blob(tagger_blob()), *SY.to_labels(texts))
    assert np.all(lat.status == OK)
    lhs = lat.as_lhs()
    got = arrays(F.posterior_lhs_batch(lhs))
    assert F.last_launch_stats().engine == 16
    assert np.all(got["status"] == OK) and np.all(np.isfinite(got["total"]))
    fsts = [lat.item(i) for i in range(len(lat))]
    model = PM.posterior_batch(fsts)
    compare("tagger", fsts, lhs, got, model, tier=tier)
    for i in range(len(lat)):
        mass, deg = start_mass(lhs, got, i)
        # each term exp(-c) carries c's error relative to itself, plus exp's and the sum's roundings
        tol_state, tol_arc = PM.tolerances(fsts[i], model[i])
        assert abs(mass - 1.0) <= tol_arc + tol_state + 2.0 ** -52 * (deg + 2), (i, mass)


# ---- 8. cross-checks against the other engines -----------------------------------------------------

@pytest.fixture(scope="module")
def few_paths():
    """Random items with at most 16 complete paths of finite cost, and their models."""
    rng = np.random.default_rng(31)
    fsts, model = [], []
    while len(fsts) < 60:
        fst = random_item(rng, 2, 9, 0.05)
        m = PM.posterior_item(fst)
        if m[0] != OK:
            continue

        def count(s):
            c = 1 if fst[1][s] != INF else 0
            return c + sum(count(a[3]) for a in fst[2][s] if a[2] != INF)

        if 1 <= count(fst[0]) <= 16:
            fsts.append(fst)
            model.append(m)
    return fsts, model


def test_against_nbest_and_path_costs(few_paths, tier):
    fsts, model = few_paths
    lhs, got = run(fsts)
    nb = F.nbest_lhs_batch(lhs, 16)
    costs = F.batch_result_path_costs(nb, 16, got["total"])
    for i, (fst, m) in enumerate(zip(fsts, model)):
        tol_state, tol_arc = PM.tolerances(fst, m)
        D, d, _ = PM.shape(fst)
        M = max([abs(v) for v in list(fst[1]) + [a[2] for x in fst[2] for a in x]
                 if math.isfinite(v)] + [abs(m[1])])
        # a path's own left fold of at most D weights errs by D * D * M * 2^-53 at most
        tol_path = 2.0 ** -52 * D * D * (M + 1.0)
        totals = []
        for k in range(16):
            s = i * 16 + k
            if nb.status[s] != OK:
                assert costs[s] == INF
                continue
            c = 0.0
            for w in nb.weights[int(nb.offsets[s]):int(nb.offsets[s + 1])].tolist():
                c += w
            totals.append(c + float(nb.finals[s]))
            assert bits([costs[s]])[0] == bits([totals[-1] - float(got["total"][i])])[0]
        # -log sum exp(-path total) is the total: each term within tol_path, the sum's own
        # rounding within 16 * 2^-52 relative, the device's total within tol_state of the exact one
        lo = min(totals)
        z = lo - math.log(sum(math.exp(-(t - lo)) for t in totals))
        assert abs(z - float(got["total"][i])) <= 2 * tol_state + tol_path + 2.0 ** -47, i
        # the confidences sum to one: d(sum p) <= sum p * (dc) + 16 roundings
        p = sum(math.exp(-c) for c in costs[i * 16:(i + 1) * 16].tolist() if c != INF)
        assert abs(p - 1.0) <= 2 * tol_state + tol_path + 2.0 ** -47, (i, p)
        # ... and so does what leaves the start state
        mass, deg = start_mass(lhs, got, i)
        assert abs(mass - 1.0) <= tol_arc + tol_state + 2.0 ** -52 * (deg + 2), (i, mass)
