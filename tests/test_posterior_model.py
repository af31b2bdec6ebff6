"""CPU: tests/posterior_model.py against exact arithmetic.  On random acyclic items of at most 8
states every complete path is enumerated and -log sum exp(-cost) is computed per item, per state
and per arc in mpmath at 60 digits; the model must agree within the derived tolerances.  Also
the order of the statuses and the hand-written KNOWN answers."""
import math

import mpmath
import numpy as np
import pytest

import posterior_model as PM

INF = math.inf
mpmath.mp.dps = 60


def random_item(rng, lo=1, hi=8, p_inf=0.1):
    """An acyclic item whose ids are not in topological order; some +inf arcs and finals,
    weights of both signs, a few -0.0."""
    n = int(rng.integers(lo, hi + 1))
    perm = rng.permutation(n)
    arcs = [[] for _ in range(n)]
    for s in range(n):
        for t in range(s + 1, n):
            for _ in range(int(rng.integers(0, 3)) if rng.random() < 0.5 else 0):
                r = rng.random()
                w = INF if r < p_inf else (-0.0 if r < p_inf + 0.05 else float(rng.normal(0.0, 3.0)))
                arcs[perm[s]].append((int(rng.integers(1, 9)), int(rng.integers(0, 9)), w,
                                      int(perm[t])))
    finals = [float(rng.normal(0.0, 2.0)) if rng.random() < 0.4 else INF for _ in range(n)]
    if rng.random() < 0.9:
        finals[int(perm[n - 1])] = float(rng.normal(0.0, 2.0))
    return int(perm[0]), finals, arcs


def exact(fst):
    """(total, alpha, beta, arc_cost) by enumeration in mpmath; None where the mass is zero."""
    start, finals, arcs = fst
    n = len(finals)
    base, k = [], 0
    for x in arcs:
        base.append(k)
        k += len(x)
    z = mpmath.mpf(0)
    za, zb, zc = [mpmath.mpf(0)] * n, [mpmath.mpf(0)] * n, [mpmath.mpf(0)] * k

    def suffix(s):  # the mass of every complete suffix from s
        m = mpmath.exp(-mpmath.mpf(finals[s])) if finals[s] != INF else mpmath.mpf(0)
        for a in arcs[s]:
            if a[2] != INF:
                m += mpmath.exp(-mpmath.mpf(a[2])) * suffix(a[3])
        return m

    def walk(s, mass, used):
        nonlocal z
        za[s] += mass
        if finals[s] != INF:
            m = mass * mpmath.exp(-mpmath.mpf(finals[s]))
            z += m
            for a in used:
                zc[a] += m
        for j, a in enumerate(arcs[s]):
            if a[2] != INF:
                walk(a[3], mass * mpmath.exp(-mpmath.mpf(a[2])), used + [base[s] + j])

    walk(start, mpmath.mpf(1), [])
    seen = PM._reach(start, arcs)
    for s in seen:
        zb[s] = suffix(s)
    nl = lambda m: -mpmath.log(m) if m > 0 else None
    return nl(z), [nl(m) for m in za], [nl(m) for m in zb], [
        (nl(m) - nl(z)) if m > 0 and z > 0 else None for m in zc]


def close(got, want, tol):
    if want is None:
        return got == INF
    return got != INF and abs(mpmath.mpf(got) - want) <= tol


@pytest.mark.parametrize("seed", range(4))
def test_model_against_enumeration(seed):
    rng = np.random.default_rng(900 + seed)
    n_ok = 0
    for _ in range(60):
        fst = random_item(rng)
        res = PM.posterior_item(fst)
        st, total, alpha, beta, cost = res
        ztot, za, zb, zc = exact(fst)
        if ztot is None:
            assert st == PM.EMPTY and total == INF, fst
            continue
        assert st == PM.OK, fst
        n_ok += 1
        tol_state, tol_arc = PM.tolerances(fst, res)
        assert close(total, ztot, tol_state), (fst, total, ztot)
        seen = PM._reach(fst[0], fst[2])
        for s in range(len(alpha)):
            if s in seen:
                assert close(alpha[s], za[s], tol_state), (fst, s)
                assert close(beta[s], zb[s], tol_state), (fst, s)
            else:
                assert alpha[s] == INF and beta[s] == INF
        for a in range(len(cost)):
            assert close(cost[a], zc[a], tol_arc), (fst, a, cost[a], zc[a])
    assert n_ok > 30


def test_known_answers():
    for fst, st, total, alpha, beta, cost in PM.KNOWN:
        res = PM.posterior_item(fst)
        assert res[0] == st
        tol_state, tol_arc = PM.tolerances(fst, res)
        for got, want, tol in [([res[1]], [total], tol_state), (res[2], alpha, tol_state),
                               (res[3], beta, tol_state), (res[4], cost, tol_arc)]:
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert (g == w) if w == INF else (g != INF and abs(g - w) <= tol), (fst, g, w)
    # exact where no logadd meets two finite operands
    assert PM.posterior_item(PM.KNOWN[0][0])[1:] == (1.75, [0.0, 1.5], [1.75, 0.25], [0.0])
    assert PM.posterior_item(PM.KNOWN[1][0])[1] == -math.log1p(1.0)


def test_status_order():
    for fst, st in PM.STATUSES:
        res = PM.posterior_item(fst)
        assert res[0] == st, fst
        if st != PM.OK:
            assert res[1] == INF and all(v == INF for part in res[2:] for v in part)
    assert PM.logadd(INF, 3.0) == 3.0 and PM.logadd(3.0, INF) == 3.0 and PM.logadd(INF, INF) == INF
    assert PM.logadd(0.0, 0.0) == -math.log1p(1.0)
