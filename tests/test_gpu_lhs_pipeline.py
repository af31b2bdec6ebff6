"""GPU: pipelines on a general first stage (fst_pipeline_lhs_batch, fst_normalize_lhs_batch)
against the CPU oracle, item by item, bit for bit.

Expected values come from the oracle alone: stage 1 per item as tests/test_gpu_lhs_batch.py
expects it (O.compose_shortest_path, or O.compose then O.shortest_path), the projection of a
1-best output tape in Python (non-epsilon olabels; an olabel above 256 is UNSUPPORTED), every
later stage through O.batch_run on the projected chains.  Text: the last stage's olabels - 1
and the f64 left fold of its weights plus the final weight.
"""
import math

import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
from libfst_amd import synthetic as SY
from test_gpu_lhs_batch import (assert_shards_do_not_show, batch_of, bits, expect, got_item,
                                same_result, tagger_rhs)
from test_gpu_parity import csr, expected_status, load_blob

pytestmark = pytest.mark.gpu

EAGER, LAZY = F.FST_SEM_EAGER, F.FST_SEM_LAZY
SEMS = [LAZY, EAGER]
INF = math.inf
OK, EMPTY, ERROR_N, UNSUPPORTED = (F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_ERROR_N,
                                   F.FST_PATH_UNSUPPORTED)


def spec_fst(spec) -> O.Fst:
    return O.Fst(start=spec[1], finals=spec[2], arcs=spec[3])


def cn_fst(item) -> O.Fst:
    return O.Fst(start=item[0], finals=item[1], arcs=item[2])


def byte_copy() -> O.Fst:
    return O.Fst(start=0, finals=[0.0], arcs=[[(l, l, 0.0, 0) for l in range(1, 257)]])


class Stages:
    """Frozen stages: the oracle's blobs and the library's handles."""

    def __init__(self, fsts):
        self.blobs = [O.freeze(f) for f in fsts]
        self.rhs = [load_blob(b) for b in self.blobs]

    def first(self, k):
        s = Stages([])
        s.blobs, s.rhs = self.blobs[:k], self.rhs[:k]
        return s


@pytest.fixture(scope="module")
def standins():
    return Stages([spec_fst(SY.tagger()), spec_fst(SY.verbalizer()), byte_copy()])


def oracle_pipeline(fsts, blobs, sem, n=1, stage1=None):
    """Per item what the pipeline returns after the last stage, from the oracle: (status,)
    or (OK, ilabels, olabels, weight bits, final bits).  stage1: expectations to use in the
    oracle's place for the items it names (a NaN item has no oracle answer)."""
    cur = [(stage1 or {}).get(i) or expect(f, blobs[0], sem, n) for i, f in enumerate(fsts)]
    for blob in blobs[1:]:
        chains, alive = [], []
        for i, e in enumerate(cur):
            if e[0] != OK:
                continue                                  # reports that stage's status
            if any(ol > 256 for ol in e[2]):
                cur[i] = (UNSUPPORTED,)                   # not a byte: no next input
                continue
            alive.append(i)
            chains.append([ol for ol in e[2] if ol != O.EPS])
        labels, offsets = csr(chains)
        ref = O.batch_run(blob, labels, offsets, 0 if sem == LAZY else 1, n)
        st = expected_status(ref)
        for j, i in enumerate(alive):
            if st[j] != OK:
                cur[i] = (int(st[j]),)
                continue
            a0, a1 = int(ref.offsets[j]), int(ref.offsets[j + 1])
            cur[i] = (OK, ref.ilabels[a0:a1].tolist(), ref.olabels[a0:a1].tolist(),
                      bits(ref.weights[a0:a1]).tolist(), int(bits(ref.finals[j:j + 1])[0]))
    return cur


def expected_text(e):
    """(status, bytes, total weight bits) of one expected item in the text entry."""
    if e[0] == OK and any(ol > 256 for ol in e[2]):
        e = (UNSUPPORTED,)
    if e[0] != OK:
        return (e[0], b"", int(bits([INF])[0]))
    d = 0.0
    for wb in e[3]:
        d = d + float(np.array([wb], np.uint64).view(np.float64)[0])
    d = d + float(np.array([e[4]], np.uint64).view(np.float64)[0])
    return (OK, bytes(ol - 1 for ol in e[2] if ol != O.EPS), int(bits([d])[0]))


def check_labels(stages, fsts, sem, exp, n=1, **kw):
    got = F.pipeline_lhs_batch(stages.rhs, batch_of(fsts), n, sem, **kw)
    assert len(got.status) == len(fsts) and int(got.offsets[0]) == 0
    for i, e in enumerate(exp):
        assert got_item(got, i) == e, (i, sem, n)
    return got


def check_text(stages, fsts, sem, exp, **kw):
    got = F.normalize_lhs_batch(stages.rhs, batch_of(fsts), sem, **kw)
    assert len(got.status) == len(fsts) and int(got.offsets[0]) == 0
    texts = got.texts()
    for i, e in enumerate(exp):
        st, text, wbits = expected_text(e)
        assert (int(got.status[i]), texts[i], int(bits(got.total_weight[i:i + 1])[0])) == \
            (st, text, wbits), (i, sem)
    return got


def same_text(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes()
               for k in ("status", "offsets", "text", "total_weight"))


# ---- 1. known answers ------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_known_answers(standins, sem):
    two = standins.first(2)
    rng = np.random.default_rng(3)
    fsts = [cn_fst(SY.confusion_network(rng, "12", 1, 0.0)), O.compile_string(b"a 7")]
    exp = oracle_pipeline(fsts, two.blobs, sem)
    got = check_labels(two, fsts, sem, exp)
    assert F.batch_result_to_text(got).texts() == [b"onetwo", b"a seven"]
    txt = check_text(two, fsts, sem, exp)
    assert txt.texts() == [b"onetwo", b"a seven"]
    # total_weight is the last stage's own best total: the verbalizer's arcs all weigh One
    assert txt.total_weight.tolist() == [0.0, 0.0]
    one = F.normalize_lhs_batch(two.rhs[:1], batch_of(fsts), sem)
    assert one.texts() == [b"#b#c", b"a #h"]
    assert one.total_weight.tolist() == [1.0, 0.5]      # each digit tagged at 0.5


# ---- 2. random sweep ---------------------------------------------------------------------------

def sweep_items(seed):
    rng = np.random.default_rng(8100 + seed)
    texts = SY.utterances(rng, 24, 1, 12)
    fsts = [cn_fst(SY.confusion_network(rng, t, 4, 0.2)) for t in texts]
    for k in range(3):
        fsts.insert(5 + 7 * k, cn_fst(SY.nbest_union(rng, SY.utterances(rng, 4, 1, 10))))
    return fsts


_sweep_cache = {}


def sweep_case(standins, seed, sem):
    key = (seed, sem)
    if key not in _sweep_cache:
        fsts = sweep_items(seed)
        _sweep_cache[key] = (fsts, oracle_pipeline(fsts, standins.blobs[:2], sem))
    return _sweep_cache[key]


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("seed", range(10))
def test_random_sweep(standins, seed, sem):
    two = standins.first(2)
    fsts, exp = sweep_case(standins, seed, sem)
    # the tagger accepts every byte the generators emit and the verbalizer everything the
    # tagger emits: a failure here would make this a test of statuses, not of paths
    assert all(e[0] == OK for e in exp)
    check_labels(two, fsts, sem, exp)
    check_text(two, fsts, sem, exp)


# ---- 3. failure propagation ----------------------------------------------------------------------

def failing_stages():
    """The stand-ins with three more tagger arcs: '~' -> label 300 (no byte), '@' copied (the
    verbalizer has no '@'), '^' -> epsilon."""
    spec = SY.tagger()
    spec[3][0].extend([(SY.lab("~"), 300, 0.0, 0), (SY.lab("@"), SY.lab("@"), 0.0, 0),
                       (SY.lab("^"), 0, 0.0, 0)])
    return Stages([spec_fst(spec), spec_fst(SY.verbalizer())])


def failing_items():
    rng = np.random.default_rng(12)
    ok = lambda: cn_fst(SY.confusion_network(rng, SY.utterances(rng, 1, 2, 8)[0], 3, 0.1))
    nan = O.compile_string(b"ab")
    nan.arcs[0][0] = nan.arcs[0][0][:2] + (math.nan,) + nan.arcs[0][0][3:]
    special = {
        1: (O.compile_string(b"a!b"), EMPTY),            # a label the tagger lacks
        3: (O.compile_string(b"4~2"), UNSUPPORTED),      # olabel 300 at the projection
        5: (O.compile_string(b"x@y"), EMPTY),            # the verbalizer rejects '@'
        7: (nan, UNSUPPORTED),
        9: (O.Fst(), EMPTY),                             # no states
        11: (O.Fst(finals=[0.0, INF], arcs=[[(SY.lab("a"), SY.lab("a"), 0.0, 1)], []]), EMPTY),
        13: (O.compile_string(b"^^"), OK),               # all epsilons: the empty chain
    }
    fsts = [special[i][0] if i in special else ok() for i in range(15)]
    return fsts, {i: st for i, (_, st) in special.items()}


@pytest.mark.parametrize("sem", SEMS)
def test_failure_propagation(sem):
    stages = failing_stages()
    fsts, want = failing_items()
    exp = oracle_pipeline(fsts, stages.blobs, sem, stage1={7: (UNSUPPORTED,)})
    assert [e[0] for e in exp] == [want.get(i, OK) for i in range(len(fsts))]
    assert exp[13] == (OK, [], [], [], int(bits([0.0])[0]))
    check_labels(stages, fsts, sem, exp)
    txt = check_text(stages, fsts, sem, exp)
    for i, e in enumerate(exp):
        if e[0] != OK:
            assert int(txt.offsets[i + 1]) == int(txt.offsets[i]) and txt.total_weight[i] == INF
    # one stage: the olabel of 300 reaches the text conversion itself
    one = stages.first(1)
    exp1 = oracle_pipeline(fsts, one.blobs, sem, stage1={7: (UNSUPPORTED,)})
    assert exp1[3][0] == OK and 300 in exp1[3][2]
    txt1 = check_text(one, fsts, sem, exp1)
    assert int(txt1.status[3]) == UNSUPPORTED
    # n: EMPTY before ERROR_N before UNSUPPORTED, as in the single call
    check_labels(stages, fsts, sem, [(EMPTY,)] * len(fsts), n=0)
    check_labels(stages, fsts, sem,
                 [(EMPTY,) if i in (9, 11) else (ERROR_N,) for i in range(len(fsts))], n=2)


# ---- 4. stage counts ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_stage_counts(standins, sem):
    fsts, _ = sweep_case(standins, 1, sem)
    lhs = batch_of(fsts)
    single = F.compose_frozen_shortest_path_lhs_batch(standins.rhs[0], lhs, 1, sem)
    assert same_result(F.pipeline_lhs_batch(standins.rhs[:1], lhs, 1, sem), single)
    assert same_text(F.normalize_lhs_batch(standins.rhs[:1], lhs, sem),
                     F.batch_result_to_text(single))
    for k in (1, 2, 3):
        st = standins.first(k)
        exp = oracle_pipeline(fsts, st.blobs, sem)
        check_labels(st, fsts, sem, exp)
        check_text(st, fsts, sem, exp)
    two = F.normalize_lhs_batch(standins.rhs[:2], lhs, sem)
    three = F.normalize_lhs_batch(standins.rhs, lhs, sem)
    assert two.texts() == three.texts()                 # the third stage copies bytes


# ---- 5. agreement with the entries it composes ----------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_equals_lhs_batch_then_chain_batch(standins, sem):
    fsts, _ = sweep_case(standins, 0, sem)
    lhs = batch_of(fsts)
    got = F.pipeline_lhs_batch(standins.rhs[:2], lhs, 1, sem)
    s1 = F.compose_frozen_shortest_path_lhs_batch(standins.rhs[0], lhs, 1, sem)
    chains = []
    for i in range(len(fsts)):
        assert int(s1.status[i]) == OK
        ol = s1.olabels[int(s1.offsets[i]):int(s1.offsets[i + 1])]
        assert int(ol.max(initial=0)) <= 256
        chains.append(ol[ol != 0])
    labels, offsets = csr(chains)
    s2 = F.compose_frozen_shortest_path_batch(standins.rhs[1], labels, offsets, 1, sem)
    assert same_result(got, s2)
    for name in ("status", "offsets", "ilabels", "olabels", "weights", "finals"):
        assert getattr(got, name).tobytes() == getattr(s2, name).tobytes(), name


# ---- 6. shards and arenas ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_three_shards_equal_one(standins, sem):
    fsts, exp = sweep_case(standins, 2, sem)
    two = standins.first(2)
    one = check_labels(two, fsts, sem, exp)
    three = check_labels(two, fsts, sem, exp, devices=[0], shards=3)
    for name in ("status", "offsets", "ilabels", "olabels", "weights", "finals"):
        assert getattr(one, name).tobytes() == getattr(three, name).tobytes(), name
    assert same_text(check_text(two, fsts, sem, exp),
                     check_text(two, fsts, sem, exp, devices=[0], shards=3))


@pytest.mark.parametrize("sem", SEMS)
def test_shards_do_not_show_on_the_edge_batch(sem):
    stages = [tagger_rhs(), SY.to_mutable(SY.verbalizer()).freeze()]
    lhs = F.LhsBatch.from_fsts(SY.edge_networks())
    labels = assert_shards_do_not_show(
        lambda **kw: F.pipeline_lhs_batch(stages, lhs, 1, sem, **kw))
    text = assert_shards_do_not_show(lambda **kw: F.normalize_lhs_batch(stages, lhs, sem, **kw))
    assert labels.status.tolist() == text.status.tolist()
    assert labels.status.tolist().count(OK) >= 40 and int(labels.status[9]) != OK   # (9: the NaN)


@pytest.mark.parametrize("sem", SEMS)
def test_arena_growth(standins, sem, monkeypatch):
    fsts, exp = sweep_case(standins, 2, sem)
    two = standins.first(2)
    plain = check_labels(two, fsts, sem, exp)
    plain_text = check_text(two, fsts, sem, exp)
    assert int(plain.offsets[-1]) > 8 * 4      # the first arena (8 arcs) and its x4 are too small
    monkeypatch.setenv("FSTAMD_ARENA_ARCS", "8")
    assert same_result(plain, check_labels(two, fsts, sem, exp))
    assert same_text(plain_text, check_text(two, fsts, sem, exp))
