"""The definition of fst_nbest_unique_lhs_batch (include/fst_batch.h), restated twice, on the
items and with the helpers of nbest_model.

nbest_unique()        the recurrence in the streaming form the kernels use: per state the at most
                      n least prefixes (g, a, r) with pairwise different output texts, built by
                      bounded insertion with the early exit per in-arc and the replacement of an
                      entry of equal text; then the selection that passes over chosen texts;
nbest_unique_brute()  nbest_model.nbest_brute at unbounded n, every path dropped whose output
                      text an earlier path printed, cut to n.

Both return what nbest_model's functions return: a status, or the list of at most n complete
paths, best first, each (arc indices, final state).  The output text of a path is the tuple of
its non-epsilon olabels.
"""
import nbest_model as M
from nbest_model import INF, UNSUPPORTED  # noqa: F401  (the tests read them from here)

OLABELS_DUP = (0, 0, 1, 2)


def text_of(arcs, seq):
    ol = [a[1] for lst in arcs for a in lst]
    return tuple(ol[a] for a in seq if ol[a] != 0)


def nbest_unique(start, finals, arcs, n, arc_order=None):
    """`arc_order`: a key that orders the in-arcs of a state (the kernels fill them in any
    order; the result does not depend on it).  None: by arc index."""
    st = M.precheck(start, finals, arcs)
    if st is not None:
        return st
    S = len(finals)
    flat, out = M.flatten(arcs)
    olab = [a[1] for lst in arcs for a in lst]
    reached, cyclic = M.reachable_cycle(start, S, flat, out)
    if cyclic:
        return UNSUPPORTED
    depth = [None] * S
    depth[start] = 0
    changed = True
    while changed:
        changed = False
        for s, x, _ in flat:
            if depth[s] is not None and (depth[x] is None or depth[x] < depth[s] + 1):
                depth[x] = depth[s] + 1
                changed = True
    into = [[] for _ in range(S)]
    for a, (s, x, _) in enumerate(flat):
        if reached[s]:
            into[x].append(a)
    E = [None] * S   # per state a list of ((g, a, r), text), rising in (g, a, r)
    for t in sorted((t for t in range(S) if reached[t]), key=lambda t: depth[t]):
        if t == start:
            E[t] = [((0.0, None, 0), ())]
            continue
        L = []
        for a in sorted(into[t], key=arc_order):
            s, _, w = flat[a]
            if w == INF:
                continue
            for r, ((g, _, _), txt) in enumerate(E[s]):
                h = g + w
                if h == INF:
                    break                        # the rest of the source list costs no less
                cand = (h, a, r)
                if len(L) == n and not cand < L[-1][0]:
                    break                        # full, and not before the last: leave the arc
                text = txt + ((olab[a],) if olab[a] else ())
                twin = next((j for j, e in enumerate(L) if e[1] == text), None)
                if twin is not None:
                    if not cand < L[twin][0]:
                        continue                 # passed over; the next rank may print another
                    del L[twin]                  # the candidate takes its place
                pos = len(L)
                while pos > 0 and cand < L[pos - 1][0]:
                    pos -= 1
                L.insert(pos, (cand, text))
                if len(L) > n:
                    L.pop()
        E[t] = L
    done = []
    for t in range(S):
        if not reached[t] or finals[t] == INF:
            continue
        for r, ((g, _, _), _) in enumerate(E[t]):
            total = g + finals[t]
            if total != INF:
                done.append((total, t, r))
    done.sort()
    paths, seen = [], set()
    for _, t, r in done:
        if len(paths) == n:
            break
        if E[t][r][1] in seen:
            continue
        seen.add(E[t][r][1])
        seq, s, k = [], t, r
        while True:
            (_, a, k2), _ = E[s][k]
            if a is None:
                break
            seq.append(a)
            s, k = flat[a][0], k2
        paths.append((seq[::-1], t))
    return paths


def nbest_unique_brute(start, finals, arcs, n):
    every = M.nbest_brute(start, finals, arcs, 1 << 62)
    if not isinstance(every, list):
        return every
    paths, seen = [], set()
    for seq, t in every:
        text = text_of(arcs, seq)
        if text not in seen:
            seen.add(text)
            paths.append((seq, t))
    return paths[:n]


def random_item_dup(rng, max_states=7):
    """nbest_model.random_item with the olabels drawn from (0, 0, 1, 2): few labels and many
    epsilons, so that different paths often print the same text."""
    start, finals, arcs = M.random_item(rng, max_states)
    arcs = [[(il, rng.choice(OLABELS_DUP), w, nx) for il, _, w, nx in lst] for lst in arcs]
    return start, finals, arcs


I = INF
# (name, item, {n: expected}) -- answers written by hand; arcs are (il, ol, w, next)
KNOWN_UNIQUE = [
    ("two parallel arcs of one olabel: one path, the cheaper",
     (0, [I, 0.0], [[(1, 5, 2.0, 1), (2, 5, 1.0, 1)], []]),
     {1: [([1], 1)], 2: [([1], 1)], 3: [([1], 1)]}),
    ("two parallel arcs of one olabel at a tie: the lower arc index",
     (0, [I, 0.0], [[(1, 5, 1.0, 1), (2, 5, 1.0, 1)], []]),
     {1: [([0], 1)], 2: [([0], 1)]}),
    ("x:eps eps:y against eps:y x:eps in a diamond",
     (0, [I, I, I, 0.0], [[(7, 0, 1.0, 1), (0, 9, 0.5, 2)], [(0, 9, 1.0, 3)], [(7, 0, 1.0, 3)],
                          []]),
     {1: [([1, 3], 3)], 2: [([1, 3], 3)]}),
    ("(1, eps, 2) equals (1, 2)",
     (0, [I, I, I, I, 0.0], [[(1, 1, 1.0, 1), (1, 1, 1.0, 3)], [(1, 0, 1.0, 2)], [(1, 2, 1.0, 4)],
                             [(1, 2, 1.5, 4)], []]),
     {1: [([1, 4], 4)], 2: [([1, 4], 4)]}),
    ("(1, 2) against (2) and against (1): one walk runs out first, three texts",
     (0, [I, I, I, 0.0], [[(1, 1, 1.0, 1), (1, 2, 2.5, 3), (1, 1, 1.0, 2)], [(1, 2, 1.0, 3)],
                          [(1, 0, 2.0, 3)], []]),
     {1: [([0, 3], 3)], 2: [([0, 3], 3), ([1], 3)], 3: [([0, 3], 3), ([1], 3), ([2, 4], 3)],
      16: [([0, 3], 3), ([1], 3), ([2, 4], 3)]}),
    ("one text into two final states: the lower total",
     (0, [I, 0.5, 0.25], [[(1, 5, 1.0, 1), (1, 5, 1.0, 2)], [], []]),
     {1: [([1], 2)], 2: [([1], 2)]}),
    ("one text into two final states at equal totals: the lower state",
     (0, [I, 0.0, 0.0], [[(1, 5, 1.0, 2), (1, 5, 1.0, 1)], [], []]),
     {1: [([1], 1)], 2: [([1], 1)]}),
    ("the empty text twice: the start as a final and an all-epsilon path",
     (0, [0.5, I, 0.0], [[(1, 0, 0.1, 1)], [(2, 0, 0.1, 2)], []]),
     {1: [([0, 1], 2)], 2: [([0, 1], 2)]}),
    ("a repeat that arrives after its better twin is in a full list",
     (0, [I, 0.0], [[(1, 1, 1.0, 1), (1, 2, 2.0, 1), (2, 1, 1.5, 1)], []]),
     {1: [([0], 1)], 2: [([0], 1), ([1], 1)], 3: [([0], 1), ([1], 1)]}),
    ("a better twin that arrives after the worse one takes its place",
     (0, [I, 0.0], [[(1, 3, 0.5, 1), (1, 1, 1.75, 1), (1, 2, 1.5, 1), (2, 1, 1.0, 1)], []]),
     {1: [([0], 1)], 2: [([0], 1), ([3], 1)], 3: [([0], 1), ([3], 1), ([2], 1)],
      16: [([0], 1), ([3], 1), ([2], 1)]}),
]
