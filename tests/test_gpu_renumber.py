"""The device copy's state renumbering (device_engine.hip bfs_renumbering): every engine
under FSTAMD_RENUMBER=0 and =1, each on a fresh handle, against the CPU oracle bit for bit
(statuses, ilabels, olabels, weight bits, final bits), on inputs built for ties.

The contract under test: no kernel orders anything by rhs state id, so breadth-first ids on
the device change no result.  Renumbering changes `RhsView::start`, `jump_fwd`,
`jump_back`, every `ArcRec::next`, the reverse mirror's in-arc order and whether the band
replay and its table exist at all.  The inputs (tests/renumber_model.py; their conditions
are asserted on the CPU by tests/test_renumber_model.py):

  A  forward-only rhs whose breadth-first ids are not forward-only: =1 takes the band
     replay away (the marker rhs of test_gpu_edge_labels.py, a tie_rhs whose epsilon arcs
     skip a layer);
  B  scattered layered rhs: breadth-first ids make them forward-only again, and auto mode
     (the variable unset) renumbers them (tie_rhs in three weight sets and two layouts,
     eps_dense 64, ambiguous 256);
  C  a cyclic rhs with epsilons whose breadth-first ids move at least half of its states.

Every case reads the `rhs mirror:` route-log line of each device copy it built and compares
it with the model: states, arcs, renumbered yes / no, states moved, jump_fwd, jump_back.
That pins tests/renumber_model.py to the C++ rule.

Tier P's records (`records N`, read as test_gpu_f32_cells.py reads them) are the same under
both settings in every case.  One thing does follow the band: the packed cells need a jump
span of at most 63 states, so B-split and B-split-half run them under =1 and unset and the
unpacked 4-B records under =0 (test_eager_tiers takes the span from the model).
"""
import functools
import re

import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
import renumber_model as M
import test_gpu_lhs_batch as LB
from test_gpu_eager_general import compare_compose
from test_gpu_edge_labels import (LAZY_ENV, band, band_plans, check_taken, engine,  # noqa: F401
                                  handed_on, only_lp, tier)
from test_gpu_f32_cells import routed_records
from test_gpu_parity import EAGER, LAZY, check, compare_single, csr, load_blob
from test_gpu_text import to_labels
from test_gpu_text_streamed import identical, shard_log

pytestmark = pytest.mark.gpu

MODES = ["0", "1"]
MIRROR = re.compile(r"rhs mirror: states (\d+) arcs (\d+), renumbered (yes|no) \(moved (\d+)\), "
                    r"jump fwd (\d+) back (\d+)")


def case_modes(names, unset=True):
    """(case, mode) pairs: =0 and =1 for every case, and the variable unset (auto mode) for
    class B."""
    out = []
    for n in names:
        for m in MODES + ([None] if unset and n.startswith("B-") else []):
            out.append(pytest.param(n, m, id="%s-%s" % (n, "unset" if m is None else "renumber" + m)))
    return out


def mirror_lines(err):
    return [(int(a), int(b), c, int(d), int(e), int(f)) for a, b, c, d, e, f in MIRROR.findall(err)]


def expected_mirror(blob, mode):
    perm, (jf, jb) = M.device_ids(blob, mode)
    _, arcs = M.frozen(blob)
    return (len(arcs), sum(len(al) for al in arcs), "no" if perm is None else "yes",
            M.moved(perm), jf, jb)


@pytest.fixture
def renumber(monkeypatch, capfd):
    """run(blob, mode, fn): fn() under FSTAMD_RENUMBER=mode with the route log on; every
    device copy built meanwhile must be the one the model predicts.  Returns (fn's value,
    the captured stderr).  may_skip: the call may answer without a device copy."""
    def run(blob, mode, fn, degenerate=False, may_skip=False):
        monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
        if mode is None:
            monkeypatch.delenv("FSTAMD_RENUMBER", raising=False)
        else:
            monkeypatch.setenv("FSTAMD_RENUMBER", mode)
        capfd.readouterr()
        out = fn()
        err = capfd.readouterr().err
        got = mirror_lines(err)
        want = expected_mirror(blob, mode)
        assert (got or may_skip) and set(got) <= {want}, (got, want)
        if not degenerate:  # forced on, forced off; auto mode fires on class B
            assert want[2] == ("no" if mode == "0" else "yes") and (mode == "0" or want[3] > 0)
        return out, err
    return run


def case_of(name):
    c = M.cases()[name]
    labels, offsets = csr([list(s) for s in c.seqs])
    return c, labels, offsets


# ---------------------------------------------------------------------------------------
# lazy: the seven engines, the default route, the band replay, the pull alone
# ---------------------------------------------------------------------------------------

ALL = sorted(M.cases())
EPS = [n for n in ALL if M.cases()[n].eps]


def to_dense_replay(err):
    """How many strings the LDS replays left for the engines behind them (the route log)."""
    return [int(x) for x in re.findall(r"lazy: \d+ strings, LDS-128 .* to the dense replay (\d+)", err)]


@pytest.mark.parametrize("name,mode", case_modes(ALL))
def test_lazy_engines(name, mode, engine, renumber, monkeypatch):
    c, labels, offsets = case_of(name)
    _, err = renumber(c.blob, mode, lambda: check(c.blob, labels, offsets, LAZY))
    # ... and the forced engine is the one that answered.  rounds / general / replay have no
    # engine behind them (last_launch_stats: 4 = the layered engine first, which takes an rhs
    # without input epsilons, 3 = the general rounds engine, 1 = the hashed replay).  The LDS
    # replays and the dense replay do: the route log says how many strings the LDS sizes left
    # over, and the dense replay runs once more without the engines behind it
    want = {"rounds": 3 if c.eps else 4, "general": 3, "replay": 1, "replay_hbm": 1,
            "dense": 5, "lds": 5, "lds_chain": 5}[engine]
    assert F.last_launch_stats().engine == want
    if engine.startswith("lds"):
        left = to_dense_replay(err)
        assert left and left[-1] < len(c.seqs), err[-2000:]
    if engine == "dense":
        monkeypatch.setenv("FSTAMD_DENSE_NOFALLBACK", "1")
        (_, took), _ = renumber(c.blob, mode, lambda: check_taken(c.blob, labels, offsets, LAZY,
                                                                  all_taken=False))
        assert took.any()


@pytest.mark.parametrize("name,mode", case_modes(ALL))
def test_lazy_default_route(name, mode, renumber, monkeypatch):
    for k in LAZY_ENV:
        monkeypatch.delenv(k, raising=False)
    c, labels, offsets = case_of(name)
    renumber(c.blob, mode, lambda: check(c.blob, labels, offsets, LAZY))


@pytest.mark.parametrize("name,mode", case_modes(ALL))
def test_lazy_band(name, mode, band, renumber):
    # class A: the band takes strings under =0 and runs no plan under =1 (jump_back > 0);
    # class B: the reverse, and auto mode is =1; class C: never.  The strided arc table
    # exists only where the band does (epsilon rhs, jump_back == 0)
    c, labels, offsets = case_of(name)
    _, err = renumber(c.blob, mode, lambda: check(c.blob, labels, offsets, LAZY))
    _, (jf, jb) = M.device_ids(c.blob, mode)
    assert (jb == 0) == {"A": mode == "0", "B": mode != "0", "C": False}[c.cls]
    plans = band_plans(err)
    if jb:
        assert not plans and not handed_on(err), err[-2000:]
    else:
        # the line counts the strings the band left OVERFLOW: fewer than all, so it took some
        assert handed_on(err) and handed_on(err)[-1] < len(c.seqs), err[-2000:]
        table = "on" if (c.eps and band == "table") else "off"
        assert plans and all(p == (table, "on" if jf < 32 else "off") for p in plans), plans


BAND_ALONE = [p for p in case_modes(ALL) if M.device_ids(M.cases()[p.values[0]].blob, p.values[1])[1][1] == 0]


@pytest.mark.parametrize("name,mode", BAND_ALONE)
def test_lazy_band_alone(name, mode, band, renumber, monkeypatch):
    # wherever the model says the band exists (class A under =0, class B under =1 and unset):
    # the band without the rounds engine behind it (FSTAMD_DENSE_NOFALLBACK, as
    # test_gpu_edge_labels.py::test_marker_band_takes_the_other_strings).  The band may hand a
    # string on as OVERFLOW -- its window here is 64 states, and the open tuples of a long
    # string on a wide layered rhs can span more -- and the dense replay then answers that
    # string; the log line counts them, so the others are the band's own answers.  With the
    # arc table a string that holds 0xFFFFFFFF is left UNSUPPORTED (the padding slots' label)
    c, labels, offsets = case_of(name)
    monkeypatch.setenv("FSTAMD_DENSE_NOFALLBACK", "1")
    (got, took), err = renumber(c.blob, mode, lambda: check_taken(c.blob, labels, offsets, LAZY,
                                                                  all_taken=False))
    assert band_plans(err) and handed_on(err), err[-2000:]
    has_ff = np.array([0xFFFFFFFF in s for s in c.seqs])
    if c.eps and band == "table" and has_ff.any():
        assert np.all(got.status[has_ff] == F.FST_PATH_UNSUPPORTED) and took[~has_ff].all()
    else:
        assert took.all()
    # answered by the band itself: taken, and not among those handed on to the dense replay
    assert int(took.sum()) - handed_on(err)[-1] > 0, (int(took.sum()), handed_on(err))


@pytest.mark.parametrize("name,mode", case_modes(ALL))
def test_lazy_pull_alone(name, mode, only_lp, renumber):
    # the tier alone: what it takes is exact, the rest is left OVERFLOW / UNSUPPORTED; with
    # input epsilons the pull does not apply and the default chain answers everything
    c, labels, offsets = case_of(name)
    (_, took), _ = renumber(c.blob, mode, lambda: check_taken(c.blob, labels, offsets, LAZY,
                                                              all_taken=c.eps))
    assert took.any()  # (the tier may still hand a string on: an uncertified tuple)


# ---------------------------------------------------------------------------------------
# eager on epsilon-free rhs: tiers P, A0, A, B and the default chain (= tier P first)
# ---------------------------------------------------------------------------------------

# tier P's (records, weight scale) by weight set and layout, by the rule of
# pull_kernel_dispatch.hpp pull_rk / route_rk and eager_pull.hip build_reverse_mirror:
#   2 = the 8-B records: integer weights <= 7 after a power-of-two scale (0.5, 1.5 -> scale 2);
#   3 = the 4-B records: the same weights, and the direct layout (every state has in-arcs of
#       one label: B-split; B-tie's states have in-arcs of both labels, so it stays at 2);
#   4 = the 4-B records with an index into the table of distinct weights, f64 cells: weights
#       that no scale makes integers (0.1, 1.1), at most 64 distinct, direct layout;
#   0 = the 16-B f64 records, f64 cells: such weights without the direct layout.
# The scale is printed as 1 for 0 and 4.  A change of that rule changes these values.
RECORDS = {"B-tie": (2, 1.0), "B-tie-half": (2, 2.0), "B-tie-tenth": (0, 1.0),
           "B-split": (3, 1.0), "B-split-half": (3, 2.0), "B-split-tenth": (4, 1.0)}
# (tier P first, the default: the streamed route launches the pull itself and prints the tier
# line only when the pull hands strings on; its own `records` line shows that it ran)
TIER_LINE = {"window": "tiers P 0 A0 1", "wave": "tiers P 0 A0 0 A 1", "wg": "tiers P 0 A0 0 A 0 B 1"}


@pytest.mark.parametrize("name,mode", case_modes(sorted(RECORDS)))
def test_eager_tiers(name, mode, tier, renumber):
    c, labels, offsets = case_of(name)
    _, err = renumber(c.blob, mode, lambda: check(c.blob, labels, offsets, EAGER))
    if tier:
        assert TIER_LINE[tier] in err, err[-2000:]
    else:
        assert routed_records(err, EAGER) == {RECORDS[name]}
        # the packed cells hold a jump span of at most 63 states
        packed = re.findall(r"eager pull: packed cells (on|off)", err)
        jf, jb = M.device_ids(c.blob, mode)[1]
        if RECORDS[name][0] == 3:
            assert packed and set(packed) == {"on" if jf + jb <= 63 else "off"}, (packed, jf, jb)
            assert (jf + jb <= 63) == (mode != "0")
        else:
            assert not packed


@pytest.mark.parametrize("mode", MODES)
def test_eager_marker_without_epsilons(mode, renumber):
    c, labels, offsets = case_of("A-marker-noeps")
    renumber(c.blob, mode, lambda: check(c.blob, labels, offsets, EAGER))


# ---------------------------------------------------------------------------------------
# eager on epsilon rhs: the general BFS tiers
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("knob", [None, "FSTAMD_BFS_TINY", "FSTAMD_EAGER_CTINY"])
@pytest.mark.parametrize("name,mode", case_modes(EPS))
def test_eager_general(name, mode, knob, renumber, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "0")
    c, labels, offsets = case_of(name)
    assert c.eps
    renumber(c.blob, mode, lambda: check(c.blob, labels, offsets, EAGER))
    assert F.last_launch_stats().engine == 2


# ---------------------------------------------------------------------------------------
# single calls, fst_compose_frozen, the lhs batch entry
# ---------------------------------------------------------------------------------------

LHS_RHS = ["C-cyclic", "B-tie-eps", "B-tie"]


@pytest.mark.parametrize("name,mode", case_modes(LHS_RHS))
def test_single_calls_with_general_lhs(name, mode, renumber):
    c = M.cases()[name]
    renumber(c.blob, mode, lambda: [compare_single(lhs, c.blob) for lhs in M.small_lhs()[:10]])


@pytest.mark.parametrize("name,mode", case_modes(LHS_RHS))
def test_compose_frozen_lattice(name, mode, renumber):
    # the whole lattice: state numbering, arc order, labels, weight bits, finals
    c = M.cases()[name]
    renumber(c.blob, mode, lambda: [compare_compose(lhs, c.blob) for lhs in M.small_lhs()[:10]])


@functools.lru_cache(maxsize=None)
def lhs_expected(name, sem):
    c = M.cases()[name]
    return [LB.expect(f, c.blob, sem) for f in M.small_lhs()]


@pytest.mark.parametrize("sem", [LAZY, EAGER])
@pytest.mark.parametrize("name,mode", case_modes(LHS_RHS))
def test_lhs_batch_entry(name, mode, sem, renumber):
    c = M.cases()[name]
    fsts = M.small_lhs()
    assert len(fsts) == 64
    exp = lhs_expected(name, sem)
    assert sum(e[0] == F.FST_PATH_OK for e in exp) >= 16  # (the items are not all EMPTY)
    renumber(c.blob, mode, lambda: LB.check(load_blob(c.blob), c.blob, fsts, sem, exp=exp))


# ---------------------------------------------------------------------------------------
# text in, text out: the streamed and the sharded route
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [LAZY, EAGER])
@pytest.mark.parametrize("mode", MODES + [None])
def test_text_routes(mode, sem, renumber, monkeypatch):
    c, labels, offsets = case_of("B-tie-bytes")
    texts = [bytes(x - 1 for x in s) for s in c.seqs]
    tl, to = to_labels(texts)
    assert np.array_equal(tl, labels) and np.array_equal(to, offsets)

    def reference():  # the label entry on the blob's own ids, itself checked against the oracle
        got, _ = check(c.blob, labels, offsets, sem)
        return F.batch_result_to_text(got)

    want, _ = renumber(c.blob, "0", reference)
    assert (want.status == F.FST_PATH_OK).mean() >= 0.8
    monkeypatch.setenv("FSTAMD_SHARD_LOG", "1")
    for stream, route in (("1", "streamed-text"), ("0", "sharded")):
        def run():
            with monkeypatch.context() as m:
                if stream == "0":
                    m.setenv("FSTAMD_STREAM", "0")
                return F.normalize_text_batch([load_blob(c.blob)], texts, sem)
        got, err = renumber(c.blob, mode, run)
        assert [ln[-1] for ln in shard_log(err)] == [route], err[-2000:]
        identical(got, want)


# ---------------------------------------------------------------------------------------
# fst_device_adopt_blob
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_adopted_handle(sem, renumber):
    import torch
    from libfst_amd.dist import adopt_on_device
    c, labels, offsets = case_of("B-tie")

    def adopted():
        buf = torch.frombuffer(bytearray(c.blob), dtype=torch.uint8).to("cuda:0")
        rhs = adopt_on_device(buf, 0)
        return check(c.blob, labels, offsets, sem, rhs=rhs)[0]

    a, _ = renumber(c.blob, "1", adopted)
    b, _ = renumber(c.blob, "1", lambda: check(c.blob, labels, offsets, sem)[0])
    assert LB.same_result(a, b)


# ---------------------------------------------------------------------------------------
# degenerate rhs: never renumbered, answered as the oracle answers them
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [LAZY, EAGER])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["no_start", "one_state"])
def test_degenerate_rhs(which, mode, sem, renumber):
    f = M.no_start_rhs() if which == "no_start" else M.one_state_rhs()
    blob = O.freeze(f)
    labels, offsets = csr([[], [1], [1, 1, 1], [2], [1] * 15])
    (got, ref), err = renumber(blob, mode, lambda: check(blob, labels, offsets, sem),
                               degenerate=True)
    assert mirror_lines(err)[0][2:4] == ("no", 0)
    if which == "no_start":
        assert np.all(got.status == F.FST_PATH_EMPTY)
    else:
        assert list(got.status[:3]) == [F.FST_PATH_OK] * 3
    lhs = M.small_lhs()[:4]
    skip = which == "no_start"  # (answered on the host: EMPTY, an empty lattice)
    renumber(blob, mode, lambda: [compare_single(x, blob) for x in lhs], True, skip)
    renumber(blob, mode, lambda: [compare_compose(x, blob) for x in lhs], True, skip)
