"""fst_posterior_lhs_batch's definition (include/fst_batch.h) in plain Python floats: the same
folds in the same order, with math.exp and math.log1p.

An item is (start, finals, arcs) as LhsBatch.from_fsts takes it: `start` a state id or None,
`finals` one weight per state (inf: not final), `arcs` per state a list of
(ilabel, olabel, weight, nextstate).  posterior_item gives (status, total, alpha, beta,
arc_cost), arc_cost flat in CSR order.  tolerances gives the derived bounds for one item."""
import math

INF, NAN = math.inf, math.nan
OK, EMPTY, UNSUPPORTED = 0, 1, 5   # FST_PATH_OK, FST_PATH_EMPTY, FST_PATH_UNSUPPORTED
LOG2 = math.log(2.0)


def logadd(x, y):
    if x == INF:
        return y
    if y == INF:
        return x
    m = x if x < y else y
    big = y if x < y else x
    return m - math.log1p(math.exp(-(big - m)))


def _bad(v):
    """NaN or -inf."""
    return not v > -INF


def _reach(start, arcs):
    seen, stack = {start}, [start]
    while stack:
        s = stack.pop()
        for a in arcs[s]:
            if a[3] not in seen:
                seen.add(a[3])
                stack.append(a[3])
    return seen


def _levels(start, arcs, seen):
    """depth per reachable state (the longest path from the start), or None on a cycle."""
    indeg = {s: 0 for s in seen}
    for s in seen:
        for a in arcs[s]:
            indeg[a[3]] += 1
    depth, ready, done = {start: 0}, [s for s in seen if indeg[s] == 0], 0
    while ready:
        s = ready.pop()
        done += 1
        for a in arcs[s]:
            t = a[3]
            depth[t] = max(depth.get(t, 0), depth[s] + 1)
            indeg[t] -= 1
            if indeg[t] == 0:
                ready.append(t)
    return depth if done == len(seen) else None


def posterior_item(fst):
    start, finals, arcs = fst
    n = len(finals)
    na = sum(len(x) for x in arcs)
    fail = lambda st: (st, INF, [INF] * n, [INF] * n, [INF] * na)
    if start is None or n == 0:
        return fail(EMPTY)
    if any(_bad(f) for f in finals) or any(_bad(a[2]) for x in arcs for a in x):
        return fail(UNSUPPORTED)
    seen = _reach(start, arcs)
    depth = _levels(start, arcs, seen)
    if depth is None:
        return fail(UNSUPPORTED)
    # arc index within the item, and the in-arcs of every state in increasing arc index
    base, k = [], 0
    for x in arcs:
        base.append(k)
        k += len(x)
    into = [[] for _ in range(n)]
    for s in range(n):
        if s in seen:
            for j, a in enumerate(arcs[s]):
                into[a[3]].append((base[s] + j, s, a[2]))
    order = sorted(seen, key=lambda s: depth[s])
    alpha, beta = [INF] * n, [INF] * n
    overflow = False
    for t in order:
        if t == start:
            acc = 0.0
        else:
            acc = INF
            for _, s, w in into[t]:     # (appended by rising s, then j: rising arc index)
                acc = logadd(acc, alpha[s] + w)
        overflow |= _bad(acc)
        alpha[t] = acc
    for s in reversed(order):
        acc = finals[s]
        for a in arcs[s]:
            acc = logadd(acc, a[2] + beta[a[3]])
        overflow |= _bad(acc)
        beta[s] = acc
    if overflow:
        return fail(UNSUPPORTED)
    total = beta[start]
    if total == INF:
        return fail(EMPTY)
    cost = []
    for s in range(n):
        for a in arcs[s]:
            cost.append(((alpha[s] + a[2]) + beta[a[3]]) - total if s in seen else INF)
    return OK, total, alpha, beta, cost


def posterior_batch(fsts):
    return [posterior_item(f) for f in fsts]


def shape(fst):
    """(D, d, seen): levels and the largest in- or out-degree among the reachable states."""
    start, finals, arcs = fst
    seen = _reach(start, arcs)
    depth = _levels(start, arcs, seen)
    indeg = {}
    for s in seen:
        for a in arcs[s]:
            indeg[a[3]] = indeg.get(a[3], 0) + 1
    d = max([len(arcs[s]) for s in seen] + list(indeg.values()) + [0])
    return max(depth.values()) + 1, d, seen


def tolerances(fst, res):
    """(tol_state, tol_arc) of an OK item, from the item and the model's own values: with
    u = 2^-53 one logadd errs by at most 8u + u|r| (exp and log1p within 2 ulp each, plus the
    subtraction's rounding), an addition by u|sum|, and logadd does not amplify input errors; so
    device and model each lie within D (d + 1) (M + 8) u of the exact-order value.
    tol_state = 2^-52 (D + 1) (d + 1) (M + 8); tol_arc = 3 tol_state + 2^-50 M."""
    start, finals, arcs = fst
    _, _, alpha, beta, _ = res
    D, d, _ = shape(fst)
    vals = list(finals) + [a[2] for x in arcs for a in x] + list(alpha) + list(beta)
    M = max([abs(v) for v in vals if math.isfinite(v)] + [0.0])
    tol_state = 2.0 ** -52 * (D + 1) * (d + 1) * (M + 8.0)
    return tol_state, 3.0 * tol_state + 2.0 ** -50 * M


def _z(*costs):
    """-log sum exp(-c), the hand-written answers' own arithmetic."""
    return -math.log(sum(math.exp(-c) for c in costs))


_ZD = _z(1.5, 2.25)

# (item, status, total, alpha, beta, arc_cost), written by hand
KNOWN = [
    # a single arc
    ((0, [INF, 0.25], [[(1, 1, 1.5, 1)], []]),
     OK, 1.75, [0.0, 1.5], [1.75, 0.25], [0.0]),
    # two parallel zero-weight arcs: total = -log 2, each arc carries half the mass
    ((0, [INF, 0.0], [[(1, 1, 0.0, 1), (2, 2, 0.0, 1)], []]),
     OK, -LOG2, [0.0, -LOG2], [-LOG2, 0.0], [LOG2, LOG2]),
    # a diamond with unequal weights: paths of 1.5 and 2.25
    ((0, [INF, INF, INF, 0.0],
      [[(1, 1, 1.0, 1), (2, 2, 2.0, 2)], [(3, 3, 0.5, 3)], [(4, 4, 0.25, 3)], []]),
     OK, _ZD, [0.0, 1.0, 2.0, _ZD], [_ZD, 0.5, 0.25, 0.0],
     [1.5 - _ZD, 2.25 - _ZD, 1.5 - _ZD, 2.25 - _ZD]),
    # the start is final and also has arcs out: two paths of cost 1
    ((0, [1.0, 0.5], [[(1, 1, 0.5, 1)], []]),
     OK, 1.0 - LOG2, [0.0, 0.5], [1.0 - LOG2, 0.5], [LOG2]),
    # a dead end
    ((0, [INF, 0.0, INF], [[(1, 1, 1.0, 1), (2, 2, 1.0, 2)], [], []]),
     OK, 1.0, [0.0, 1.0, 1.0], [1.0, 0.0, INF], [0.0, INF]),
    # an unreachable state
    ((0, [INF, 0.0, 0.0], [[(1, 1, 1.0, 1)], [], [(2, 2, 1.0, 1)]]),
     OK, 1.0, [0.0, 1.0, INF], [1.0, 0.0, INF], [0.0, INF]),
    # an arc of +inf
    ((0, [INF, 0.0], [[(1, 1, INF, 1), (2, 2, 2.0, 1)], []]),
     OK, 2.0, [0.0, 2.0], [2.0, 0.0], [INF, 0.0]),
]

# items whose status is decided by the order of the tests: (item, status)
STATUSES = [
    ((None, [NAN], [[(1, 1, NAN, 0)]]), EMPTY),                          # no start before a NaN
    ((None, [], []), EMPTY),                                              # zero states
    ((0, [INF, NAN], [[(1, 1, 0.0, 1)], [(1, 1, 0.0, 0)]]), UNSUPPORTED),   # a NaN and a cycle
    ((0, [INF, 0.0], [[(1, 1, -INF, 1)], []]), UNSUPPORTED),              # a -inf weight
    ((0, [INF, 0.0, -INF], [[(1, 1, 1.0, 1)], [], []]), UNSUPPORTED),     # ... on an unreachable final
    ((0, [INF, 0.0], [[(1, 1, INF, 1), (2, 2, 1.0, 1)], [(3, 3, INF, 0)]]), UNSUPPORTED),  # a cycle through +inf
    ((0, [0.0], [[(1, 1, 1.0, 0)]]), UNSUPPORTED),                        # a self-loop
    ((0, [INF, INF], [[(1, 1, 1.0, 1)], []]), EMPTY),                     # no complete path
    ((0, [INF, 0.0], [[(1, 1, INF, 1)], []]), EMPTY),                     # ... of finite cost
    ((0, [INF, 0.0, INF, INF], [[(1, 1, 1.0, 1)], [], [(2, 2, 0.0, 3)], [(3, 3, 0.0, 2)]]), OK),  # an unreachable cycle
    ((0, [INF, INF, 0.0], [[(1, 1, -1.7e308, 1)], [(2, 2, -1.7e308, 2)], []]), UNSUPPORTED),  # overflow
]
