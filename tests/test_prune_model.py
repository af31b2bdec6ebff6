"""The two restatements of fst_prune_lhs_batch's definition (tests/prune_model.py) against each
other and against the definition's own consequences.  No GPU."""
import math

import numpy as np

import connect_model as CM
import prune_model as PM

INF, NAN = math.inf, math.nan
NO_STATE = CM.NO_STATE


def random_acyclic(rng, max_states=8, weights=(0.0, 0.5, 1.0, 2.0)):
    """A random item whose arcs all go to higher ids, with labels that tell the arcs apart."""
    n = int(rng.integers(1, max_states + 1))
    finals = [float(rng.choice(weights)) if rng.random() < 0.4 else INF for _ in range(n)]
    if rng.random() < 0.8:
        finals[n - 1] = float(rng.choice(weights))
    arcs, lab = [], 1
    for s in range(n):
        al = []
        for _ in range(int(rng.integers(0, 4)) if s + 1 < n else 0):
            al.append((lab, lab + 100, float(rng.choice(weights)), int(rng.integers(s + 1, n))))
            lab += 1
        arcs.append(al)
    return 0, finals, arcs


def same(x, y):
    return x[0] == y[0] and CM.to_lists(x[1]) == CM.to_lists(y[1])


def arc_labels(t):
    return set(t.il.tolist())


def test_numpy_model_equals_brute_force_on_small_acyclic_items():
    rng = np.random.default_rng(15)
    nonempty = 0
    for _ in range(300):
        fst = random_acyclic(rng)
        for beam in (0.0, 0.5, 1.5, INF):
            a, b = PM.prune(*fst, beam), PM.prune_brute(*fst, beam)
            assert same(a, b), (fst, beam)
            nonempty += len(a[1].finals) > 0
    assert nonempty > 300


def test_infinite_beam_is_connect():
    rng = np.random.default_rng(16)
    for _ in range(200):
        fst = random_acyclic(rng)
        st, t = PM.prune(*fst, INF)
        assert st == PM.OK and CM.to_lists(t) == CM.to_lists(CM.connect_lists(*fst))


def test_kept_arcs_are_nested_as_the_beam_grows():
    rng = np.random.default_rng(17)
    for _ in range(200):
        fst = random_acyclic(rng)
        prev = None
        for beam in (0.0, 0.5, 1.0, 2.5, INF):
            cur = arc_labels(PM.prune(*fst, beam)[1])
            assert prev is None or prev <= cur, (fst, beam)
            prev = cur


def test_known_diamond():
    # 0 -1-> 1 -0-> 3 (total 1), 0 -3-> 2 -0-> 3 (total 3); final(3) = 0
    fst = (0, [INF, INF, INF, 0.0],
           [[(1, 1, 1.0, 1), (2, 2, 3.0, 2)], [(3, 3, 0.0, 3)], [(4, 4, 0.0, 3)], []])
    st, t = PM.prune(*fst, 1.0)
    assert st == PM.OK and t.il.tolist() == [1, 3] and t.next.tolist() == [1, 2] and t.start == 0
    st, t = PM.prune(*fst, 2.0)
    assert t.il.tolist() == [1, 2, 3, 4]
    assert same(PM.prune(*fst, 1.0), PM.prune_brute(*fst, 1.0))


def test_negative_zero_equals_positive_zero():
    """The definition's case: every total is a zero of either sign; beam = -0.0 keeps them all.
    A key order that puts -0.0 below +0.0 would cut the arcs whose T is +0.0."""
    fst = (0, [INF, -0.0, 0.0],
           [[(1, 1, -0.0, 1), (2, 2, 0.0, 2)], [(3, 3, -0.0, 2)], []])
    for beam in (-0.0, 0.0):
        st, t = PM.prune(*fst, beam)
        assert st == PM.OK and t.il.tolist() == [1, 2, 3]
        assert CM.to_lists(t) == CM.to_lists(CM.connect_lists(*fst))
        assert same(PM.prune(*fst, beam), PM.prune_brute(*fst, beam))


def test_statuses_in_order():
    # no start wins over a NaN; a NaN or a negative arc is UNSUPPORTED; -0.0 and +inf are not
    assert PM.prune(None, [NAN], [[(1, 1, NAN, 0)]], 1.0)[0] == PM.OK
    assert PM.prune(0, [], [], 1.0)[0] == PM.OK
    for bad in (NAN, -1.0, -INF):
        st, t = PM.prune(0, [INF, 0.0], [[(1, 1, bad, 1)], []], 1.0)
        assert st == PM.UNSUPPORTED and t.start == NO_STATE and len(t.finals) == 0
    assert PM.prune(0, [NAN, 0.0], [[(1, 1, 0.0, 1)], []], 1.0)[0] == PM.UNSUPPORTED
    st, t = PM.prune(0, [INF, -2.0], [[(1, 1, -0.0, 1), (2, 2, INF, 1)], []], 0.0)
    assert st == PM.OK and t.il.tolist() == [1] and t.finals.tolist() == [INF, -2.0]


def test_no_final_and_unreachable_final_are_empty_and_ok():
    st, t = PM.prune(0, [INF, INF], [[(1, 1, 0.0, 1)], []], INF)
    assert st == PM.OK and t.start == NO_STATE
    st, t = PM.prune(0, [INF, 0.0], [[], [(1, 1, 0.0, 0)]], INF)
    assert st == PM.OK and t.start == NO_STATE
    st, t = PM.prune(0, [INF, 0.0], [[(1, 1, INF, 1)], []], INF)     # only over a +inf arc
    assert st == PM.OK and t.start == NO_STATE


def test_final_weight_cut_while_the_state_stays():
    # 0 (final 5) -1-> 1 (final 0): best = 1, the start's own final weight is outside beam 1
    fst = (0, [5.0, 0.0], [[(1, 1, 1.0, 1)], []])
    st, t = PM.prune(*fst, 1.0)
    assert st == PM.OK and t.finals.tolist() == [INF, 0.0] and t.il.tolist() == [1]
    st, t = PM.prune(*fst, 4.0)
    assert t.finals.tolist() == [5.0, 0.0]


def test_start_is_cut_under_rounding():
    """The connect step is needed.  F is a left fold, B a right fold and best a third sum: a
    huge weight absorbs a small one in the left fold and not in the right fold, so the first
    arc's T exceeds best while the later arcs' do not, and nothing links the start to what the
    cut keeps."""
    big, one = 2.0 ** 53, 1.0
    fst = (0, [INF, INF, INF, 0.0],
           [[(1, 1, big, 1)], [(2, 2, one, 2)], [(3, 3, one, 3)], []])
    # F(3) = ((big + 1) + 1) = big (each 1 is absorbed); B(0) = big + (1 + 1) = big + 2 > best
    st, t = PM.prune(*fst, 0.0)
    assert st == PM.OK and t.start == NO_STATE and len(t.finals) == 0 and len(t.next) == 0
    # with the slack the definition asks the caller for, the path is kept whole
    st, t = PM.prune(*fst, 2.0)
    assert t.start == 0 and t.il.tolist() == [1, 2, 3]


def test_cycles_are_allowed():
    # a self-loop of weight 0 on the best path and a 2-cycle of weight 1 beside it
    fst = (0, [INF, 0.0, INF],
           [[(1, 1, 1.0, 1), (2, 2, 0.0, 0)], [(3, 3, 1.0, 2)], [(4, 4, 0.0, 1)]])
    st, t = PM.prune(*fst, 0.0)
    assert st == PM.OK and t.il.tolist() == [1, 2]          # the loop costs nothing: kept
    st, t = PM.prune(*fst, 1.0)
    assert t.il.tolist() == [1, 2, 3, 4]                    # once round the 2-cycle: total 2
