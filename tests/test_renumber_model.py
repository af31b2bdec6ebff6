"""The inputs of tests/test_gpu_renumber.py, checked on the CPU against the oracle and
tests/renumber_model.py -- never against the library.  These are conditions on the inputs,
not measurements of the code: a kernel that ordered anything by device state id has to meet
strings it answers wrongly, so most strings must be answered OK, most of those must have
several co-optimal paths, and a 1-best that breaks ties by state id (`mutant_best`) must
change its answer between the blob's ids and the breadth-first ids.

The measured shares are pinned as well (SHARES): a change of a seed that moves them has to
move the figures quoted in DESIGN.md too.
"""
import numpy as np
import pytest

import oracle_ffi as O
import renumber_model as M
from test_gpu_parity import csr

NAMES = ["A-marker-eps", "A-marker-noeps", "A-tie-eps", "B-tie", "B-tie-half", "B-tie-tenth",
         "B-split", "B-split-half", "B-split-tenth", "B-tie-bytes", "B-tie-eps", "B-eps-dense",
         "B-ambiguous", "C-cyclic"]


def test_case_list_is_complete():
    assert list(M.cases()) == NAMES


@pytest.fixture(params=NAMES)
def case(request):
    return M.cases()[request.param]


def oracle_ok(case):
    labels, offsets = csr([list(s) for s in case.seqs])
    oks = []
    for sem in (0, 1):
        ref = O.batch_run(case.blob, labels, offsets, sem, 1)
        oks.append((ref.status == O.OR_OK) & (ref.empty == 0))
    return oks


def test_frozen_order_is_the_documented_sort(case):
    # the blob's span order, which bfs_perm walks, is fromMutable's
    # (ilabel, olabel, weight, nextstate) sort of each state's arcs
    start, arcs = M.frozen(case.blob)
    assert start == case.fst.start
    assert arcs == [sorted(al) for al in case.fst.arcs]


def test_bfs_perm_is_a_bijection(case):
    perm = M.bfs_perm(case.blob)
    ns = case.fst.num_states
    assert sorted(perm) == list(range(ns))
    assert perm[case.fst.start] == 0
    # breadth first: ids follow the distance from the start, unreachable states come last
    _, arcs = M.frozen(case.blob)
    dist = {case.fst.start: 0}
    todo = [case.fst.start]
    for s in todo:
        for _, _, _, t in arcs[s]:
            if t not in dist:
                dist[t] = dist[s] + 1
                todo.append(t)
    order = sorted(range(ns), key=lambda s: perm[s])
    keys = [(dist.get(s, ns), 0 if s in dist else s) for s in order]
    assert keys == sorted(keys)


def test_class_band_figures(case):
    perm = M.bfs_perm(case.blob)
    jf, jb = M.band(case.blob)
    nf, nb = M.band(case.blob, perm)
    assert len(case.seqs) <= 64 and max(len(s) for s in case.seqs) <= 15
    assert case.fst.num_states <= 300
    if case.cls == "A":    # forward only, and forced breadth-first ids lose that
        assert jb == 0 and nb > 0
        assert not M.auto_renumbers(case.blob)
    elif case.cls == "B":  # scattered, breadth-first ids restore forward only, auto fires
        assert jb > 0 and nb == 0
        assert jf + jb > 64 and (nf + nb) * 4 <= jf + jb and M.auto_renumbers(case.blob)
        assert M.device_ids(case.blob, None) == (perm, (nf, nb))
    else:                  # cyclic, epsilons, at most 60 states, half of them moved
        assert case.eps and case.fst.num_states <= 60
        assert jb > 0 and nb > 0
        assert M.moved(perm) * 2 >= case.fst.num_states
        assert all(0 <= w <= 3 and w == int(w) for al in case.fst.arcs for _, _, w, _ in al)
    assert M.device_ids(case.blob, "0") == (None, (jf, jb))
    assert M.device_ids(case.blob, "1") == (perm, (nf, nb))


# measured when the cases were chosen: (strings OK in both semantics, strings); tie cases
# also (OK strings with two or more co-optimal paths, strings where the mutant differs)
SHARES = {"A-marker-eps": (64, 64), "A-marker-noeps": (52, 64), "A-tie-eps": (56, 64),
          "B-tie": (63, 64, 63, 60), "B-tie-half": (63, 64, 63, 60), "B-tie-tenth": (63, 64, 63, 60),
          "B-split": (61, 64, 55, 51), "B-split-half": (61, 64, 55, 51),
          "B-split-tenth": (61, 64, 55, 51), "B-tie-bytes": (63, 64, 61, 58),
          "B-tie-eps": (64, 64), "B-eps-dense": (32, 32), "B-ambiguous": (32, 32),
          "C-cyclic": (64, 64)}


def test_oracle_share(case):
    lazy, eager = oracle_ok(case)
    for ok in (lazy, eager):
        assert ok.mean() >= 0.8, (case.name, int(ok.sum()), len(ok))
    assert (int((lazy & eager).sum()), len(lazy)) == SHARES[case.name][:2]


TIES = ["B-tie", "B-tie-half", "B-tie-tenth", "B-split", "B-split-half", "B-split-tenth",
        "B-tie-bytes"]


def test_tie_cases_are_the_epsilon_free_tie_rhs():
    assert [n for n, c in M.cases().items() if c.tie] == TIES
    assert not any(M.cases()[n].eps for n in TIES)


@pytest.mark.parametrize("name", TIES)
def test_tie_shares(name):
    case = M.cases()[name]
    ok = np.logical_and(*oracle_ok(case))
    ident = list(range(case.fst.num_states))
    perm = M.bfs_perm(case.blob)
    co = differs = 0
    labels, offsets = csr([list(s) for s in case.seqs])
    ref = O.batch_run(case.blob, labels, offsets, 0, 1)
    for i, s in enumerate(case.seqs):
        a, n = M.mutant_best(case.blob, s, ident)
        b, m = M.mutant_best(case.blob, s, perm)
        assert n == m and (a is None) == (b is None) == (not ok[i])
        if ok[i]:
            co += n >= 2
            if n == 1:  # a single best path: the mutant has no tie to break
                assert a == b == ref.olabels[int(ref.offsets[i]):int(ref.offsets[i + 1])].tolist()
        differs += a != b
    assert co >= 0.8 * ok.sum(), (case.name, co, int(ok.sum()))
    assert differs * 2 >= len(case.seqs), (case.name, differs, len(case.seqs))
    assert (co, differs) == SHARES[name][2:]


def test_tie_rhs_shape():
    f = M.tie_rhs(np.random.default_rng(3), 5, 4, (1, 2), 3, 1, 1)
    assert f.num_states == 21 and f.start == 0
    for s, al in enumerate(f.arcs):
        layer = 0 if s == 0 else 1 + (s - 1) // 4
        for il in (1, 2):
            mine = [a for a in al if a[0] == il]
            assert len(mine) == (0 if layer == 5 else 3)
            assert len({a[1] for a in mine}) == len(mine) == len({a[3] for a in mine})
            assert all(1 + (a[3] - 1) // 4 == layer + 1 and a[2] in (0.0, 1.0) for a in mine)
        assert sum(a[0] == 0 for a in al) <= 1
    assert any(a[0] == 0 for al in f.arcs for a in al)


def test_scattered_keeps_the_language():
    c = M.cases()["B-tie"]
    labels, offsets = csr([list(s) for s in c.seqs])
    plain = O.freeze(M.tie_rhs(np.random.default_rng(50), 14, 4, (1, 2), 3, 1, 0))
    for sem in (0, 1):
        a = O.batch_run(plain, labels, offsets, sem, 1)
        b = O.batch_run(c.blob, labels, offsets, sem, 1)
        for k in ("status", "empty", "offsets", "ilabels", "olabels"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert np.array_equal(a.weights.view(np.uint64), b.weights.view(np.uint64))


def test_degenerate_rhs_get_no_permutation():
    for f in (M.no_start_rhs(), M.one_state_rhs(), O.Fst()):
        assert M.bfs_perm(f) is None
        assert M.device_ids(f, "1") == (None, M.band(f))
