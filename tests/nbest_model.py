"""The definition of fst_nbest_lhs_batch (include/fst_batch.h), restated twice.

An item is (start, finals, arcs) as MutableFst.to_lists() gives it: `start` a state id or None
/ FST_NO_STATE, `finals` one weight per state (+inf: not final), `arcs` per state a list of
(ilabel, olabel, weight, nextstate).  An arc's index is its position in the item's flat arc
list (the states' lists one after the other: the CSR order).

nbest()        the recurrence: per state the at most n best prefixes (g, a, r), pulled level by
               level in increasing depth;
nbest_brute()  every path of the item, sorted with the recursive comparator written out.

Both return a status (EMPTY for no start, UNSUPPORTED for a NaN or a cycle among the reachable
states) or the list of at most n complete paths, best first, each (arc indices, final state).
Python's float is the f64 of the contract, `+` its fl(x + y).
"""
import functools
import math

EMPTY = 1        # FST_PATH_EMPTY
UNSUPPORTED = 5  # FST_PATH_UNSUPPORTED
NO_STATE = 0xFFFFFFFF
INF = math.inf


def flatten(arcs):
    """(src, dst, weight) per arc index, and per state the indices of its out-arcs."""
    flat, out = [], []
    for s, lst in enumerate(arcs):
        out.append(list(range(len(flat), len(flat) + len(lst))))
        flat.extend((s, a[3], a[2]) for a in lst)
    return flat, out


def precheck(start, finals, arcs):
    """The statuses that need no traversal, in the contract's order; None: go on."""
    if start is None or start == NO_STATE or len(finals) == 0:
        return EMPTY
    if any(math.isnan(f) for f in finals) or any(math.isnan(a[2]) for lst in arcs for a in lst):
        return UNSUPPORTED
    return None


def reachable_cycle(start, nstates, flat, out):
    """(reached states, whether a cycle lies among them); every arc counts, whatever its
    weight, and a self-loop is a cycle."""
    colour = [0] * nstates  # 0 new, 1 on the stack, 2 done
    colour[start] = 1
    stack = [(start, 0)]
    cyclic = False
    while stack:
        s, k = stack.pop()
        if k == len(out[s]):
            colour[s] = 2
            continue
        stack.append((s, k + 1))
        x = flat[out[s][k]][1]
        if colour[x] == 1:
            cyclic = True
        elif colour[x] == 0:
            colour[x] = 1
            stack.append((x, 0))
    return [c != 0 for c in colour], cyclic


def nbest(start, finals, arcs, n):
    st = precheck(start, finals, arcs)
    if st is not None:
        return st
    S = len(finals)
    flat, out = flatten(arcs)
    reached, cyclic = reachable_cycle(start, S, flat, out)
    if cyclic:
        return UNSUPPORTED
    # depth(t) = the longest path from the start, by relaxation over the reached states
    depth = [None] * S
    depth[start] = 0
    changed = True
    while changed:
        changed = False
        for a, (s, x, _) in enumerate(flat):
            if depth[s] is not None and (depth[x] is None or depth[x] < depth[s] + 1):
                depth[x] = depth[s] + 1
                changed = True
    into = [[] for _ in range(S)]
    for a, (s, x, _) in enumerate(flat):
        if reached[s]:
            into[x].append(a)
    E = [None] * S
    for t in sorted((t for t in range(S) if reached[t]), key=lambda t: depth[t]):
        if t == start:
            E[t] = [(0.0, None, 0)]
            continue
        cand = []
        for a in into[t]:
            s, _, w = flat[a]
            if w == INF:
                continue  # an arc of +inf is never part of a path
            for r, (g, _, _) in enumerate(E[s]):
                h = g + w
                if h != INF:
                    cand.append((h, a, r))
        # (g, a, r) lexicographic; -0.0 == 0.0 as floats, so tuples compare as the contract does
        cand.sort()
        E[t] = cand[:n]
    done = []
    for t in range(S):
        if not reached[t] or finals[t] == INF:
            continue
        for r, (g, _, _) in enumerate(E[t]):
            total = g + finals[t]
            if total != INF:
                done.append((total, t, r))
    done.sort()
    paths = []
    for _, t, r in done[:n]:
        seq, s, k = [], t, r
        while True:
            _, a, k2 = E[s][k]
            if a is None:
                break
            seq.append(a)
            s, k = flat[a][0], k2
        paths.append((seq[::-1], t))
    return paths


def nbest_brute(start, finals, arcs, n):
    st = precheck(start, finals, arcs)
    if st is not None:
        return st
    S = len(finals)
    flat, out = flatten(arcs)
    _, cyclic = reachable_cycle(start, S, flat, out)
    if cyclic:
        return UNSUPPORTED

    # every prefix: (arc indices, end state, cost), costs by the left fold from 0.0
    prefixes = []

    def walk(s, seq, g):
        prefixes.append((tuple(seq), s, g))
        for a in out[s]:
            _, x, w = flat[a]
            if w == INF:
                continue
            h = g + w
            if h == INF:
                continue  # dropped, by overflow as well
            seq.append(a)
            walk(x, seq, h)
            seq.pop()

    walk(start, [], 0.0)
    cost = {p[0]: p[2] for p in prefixes}

    def cmp_prefix(p, q):
        """The order of two prefixes that end in the same state."""
        gp, gq = cost[p], cost[q]
        if gp < gq:
            return -1
        if gp > gq:
            return 1
        if not p and not q:
            return 0
        if not p:
            return 1  # the empty prefix sorts after any arc at equal g
        if not q:
            return -1
        if p[-1] != q[-1]:
            return -1 if p[-1] < q[-1] else 1
        return cmp_prefix(p[:-1], q[:-1])

    by_end = {}
    for seq, s, _ in prefixes:
        by_end.setdefault(s, []).append(seq)
    rank = {}
    for s, lst in by_end.items():
        lst.sort(key=functools.cmp_to_key(cmp_prefix))
        for r, seq in enumerate(lst):
            rank[seq] = r
    done = []
    for seq, t, g in prefixes:
        if finals[t] == INF:
            continue
        total = g + finals[t]
        if total != INF:
            done.append((total, t, rank[seq], seq))
    done.sort(key=lambda x: x[:3])
    return [(list(seq), t) for _, t, _, seq in done[:n]]


# ---- shared by the model test and the GPU tests ---------------------------------------------

WEIGHT_POOLS = ((0.0, 1.0, 2.0), (0.1, 0.2, 0.3, 0.7), (0.5, -1.0, 0.25, -0.0, INF), (1.0,))
FINAL_POOL = (INF, INF, 0.0, 0.5, 0.1)


def random_item(rng, max_states=7):
    """A random acyclic item: 1 .. max_states states, a random permutation as topological
    order (ids do not rise along arcs), 0 .. 2 parallel arcs per ordered pair, the weights from
    one pool, the start one of the first two states in topological order.  `rng` is a
    random.Random."""
    S = rng.randint(1, max_states)
    topo = list(range(S))
    rng.shuffle(topo)
    pool = rng.choice(WEIGHT_POOLS)
    arcs = [[] for _ in range(S)]
    for i in range(S):
        for j in range(i + 1, S):
            for _ in range(rng.randint(0, 2)):
                arcs[topo[i]].append((rng.randint(1, 5), rng.randint(1, 5), rng.choice(pool),
                                      topo[j]))
    finals = [rng.choice(FINAL_POOL) for _ in range(S)]
    return topo[rng.randrange(min(2, S))], finals, arcs


I = INF
# (name, item, {n: expected}) -- answers written by hand; arcs are (il, ol, w, next)
KNOWN = [
    ("parallel arcs of equal weight: the arc index decides",
     (0, [I, 0.0], [[(1, 1, 1.0, 1), (2, 2, 1.0, 1)], []]),
     {1: [([0], 1)], 2: [([0], 1), ([1], 1)], 3: [([0], 1), ([1], 1)]}),
    ("two finals of equal total: the state id decides",
     (0, [I, 0.0, 0.0], [[(1, 1, 1.0, 2), (1, 1, 1.0, 1)], [], []]),
     {1: [([1], 1)], 2: [([1], 1), ([0], 2)]}),
    ("-0.0 against +0.0 is a tie",
     (0, [I, 0.0], [[(1, 1, 0.0, 1), (2, 2, -0.0, 1)], []]),
     {1: [([0], 1)], 2: [([0], 1), ([1], 1)]}),
    ("an arc of +inf is never part of a path",
     (0, [I, 0.0], [[(1, 1, I, 1), (2, 2, 2.0, 1)], []]),
     {1: [([1], 1)], 2: [([1], 1)]}),
    ("a prefix that overflows to +inf is dropped",
     (0, [I, I, 0.0], [[(1, 1, 1e308, 1)], [(1, 1, 1e308, 2), (2, 2, 0.0, 2)], []]),
     {1: [([0, 2], 2)], 3: [([0, 2], 2)]}),
    ("the start as a final of its own: a path of zero arcs",
     (0, [0.5, 0.0], [[(1, 1, 1.0, 1)], []]),
     {1: [([], 0)], 2: [([], 0), ([0], 1)], 16: [([], 0), ([0], 1)]}),
    ("a self-loop is a cycle",
     (0, [I, 0.0], [[(1, 1, 1.0, 0), (1, 1, 1.0, 1)], []]),
     {1: UNSUPPORTED, 3: UNSUPPORTED}),
    ("a cycle among unreachable states is none",
     (0, [I, 0.0, I, I], [[(1, 1, 1.0, 1)], [], [(1, 1, 1.0, 3)], [(1, 1, 1.0, 2)]]),
     {1: [([0], 1)], 2: [([0], 1)]}),
    ("a start with an in-arc from an unreachable state",
     (0, [I, 0.0, I], [[(1, 1, 1.0, 1)], [], [(1, 1, 1.0, 0)]]),
     {1: [([0], 1)], 2: [([0], 1)]}),
    ("no start comes before a NaN and a cycle",
     (None, [math.nan], [[(1, 1, math.nan, 0)]]),
     {1: EMPTY, 16: EMPTY}),
    ("a NaN comes before a cycle (the same status)",
     (0, [math.nan], [[(1, 1, 1.0, 0)]]),
     {2: UNSUPPORTED}),
]
