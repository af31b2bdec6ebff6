"""The device copy's state renumbering (device_engine.hip bfs_renumbering), restated in
plain Python, and the inputs the renumbering tests run: rhs built so that a kernel which
ordered anything by device state id would answer differently from the reference.

TEST INFRASTRUCTURE ONLY.  `bfs_perm` / `band` / `device_ids` restate the C++ rule from the
blob alone; `tie_rhs` is a layered rhs in which most strings have several co-optimal paths,
each with its own olabel sequence; `mutant_best` is a 1-best search that breaks ties by a
state numbering, i.e. the bug the tests are built to catch.  tests/test_renumber_model.py
checks the inputs against the oracle and this model (never against the library);
tests/test_gpu_renumber.py runs them through every engine.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import oracle_ffi as O

STATE_DTYPE = np.dtype([("off", "<u4"), ("n", "<u4"), ("fin", "<f8")])


# ---------------------------------------------------------------------------------------
# the blob, as the device copy is built from it
# ---------------------------------------------------------------------------------------

def as_blob(f) -> bytes:
    return f if isinstance(f, (bytes, bytearray)) else O.freeze(f)


def frozen(f):
    """(start, per-state list of (ilabel, olabel, weight, nextstate)) in frozen span order:
    fromMutable's (ilabel, olabel, weight, nextstate) sort, read back from the blob."""
    blob = as_blob(f)
    hdr = np.frombuffer(blob, "<u4", 6)
    ns, na, start = int(hdr[2]), int(hdr[3]), int(hdr[4])
    st = np.frombuffer(blob, STATE_DTYPE, ns, 24)
    arcs = np.frombuffer(blob, O.ARC_DTYPE, na, 24 + 16 * ns)
    out = []
    for s in range(ns):
        a = arcs[int(st["off"][s]):int(st["off"][s]) + int(st["n"][s])]
        out.append([(int(x["il"]), int(x["ol"]), float(x["w"]), int(x["next"])) for x in a])
    return start, out


def bfs_perm(f):
    """old id -> new id: breadth first from the start state, arcs in frozen span order,
    unreachable states last in id order.  None where the C++ code builds no permutation
    whatever the mode (fewer than two states, no start state)."""
    start, arcs = frozen(f)
    ns = len(arcs)
    if ns < 2 or start >= ns:
        return None
    perm = [None] * ns
    queue = []

    def visit(s):
        if perm[s] is None:
            perm[s] = len(queue)
            queue.append(s)

    visit(start)
    q = 0
    while q < len(queue):
        for _, _, _, t in arcs[queue[q]]:
            visit(t)
        q += 1
    for s in range(ns):
        visit(s)
    return perm


def band(f, perm=None):
    """(jump_fwd, jump_back) of the rhs under `perm` (None: the blob's own ids)."""
    _, arcs = frozen(f)
    jf = jb = 0
    for s, al in enumerate(arcs):
        ps = s if perm is None else perm[s]
        for _, _, _, t in al:
            pt = t if perm is None else perm[t]
            if pt >= ps:
                jf = max(jf, pt - ps)
            else:
                jb = max(jb, ps - pt)
    return jf, jb


def auto_renumbers(f) -> bool:
    """Auto mode (FSTAMD_RENUMBER unset): only when the id band is above 64 and
    breadth-first ids shrink it at least 4x."""
    perm = bfs_perm(f)
    if perm is None:
        return False
    jf, jb = band(f)
    if jf + jb <= 64:
        return False
    nf, nb = band(f, perm)
    return (nf + nb) * 4 <= jf + jb


def device_ids(f, mode):
    """(perm or None, (jump_fwd, jump_back)) of the device copy under FSTAMD_RENUMBER =
    `mode` ("0", "1", or None for unset)."""
    perm = bfs_perm(f)
    if mode == "0" or perm is None or (mode is None and not auto_renumbers(f)):
        return None, band(f)
    return perm, band(f, perm)


def moved(perm) -> int:
    return 0 if perm is None else sum(1 for i, p in enumerate(perm) if i != p)


# ---------------------------------------------------------------------------------------
# inputs built for ties
# ---------------------------------------------------------------------------------------

def scattered(f: O.Fst, seed) -> O.Fst:
    """The same FST under a random permutation of its state ids."""
    perm = np.random.default_rng(seed).permutation(f.num_states)
    g = O.Fst(start=int(perm[f.start]), finals=[0.0] * f.num_states,
              arcs=[[] for _ in range(f.num_states)])
    for s, fw in enumerate(f.finals):
        g.finals[int(perm[s])] = fw
    for s, al in enumerate(f.arcs):
        g.arcs[int(perm[s])] = [(a, b, w, int(perm[d])) for (a, b, w, d) in al]
    return g


def tie_rhs(rng, T, W, labels, fan, wmax, eps, split=False) -> O.Fst:
    """State 0, then T layers of W states (layer t = ids 1 + (t - 1) W ...).  Every state
    but the last layer's has, for each ilabel, `fan` arcs to distinct states of the next
    layer with integer weights 0..wmax and pairwise distinct olabels (1..8), so every path
    has its own olabel sequence and frozen order never depends on nextstate.  Two thirds of
    the states are final, weight 0.  eps > 0: one state in three also has an epsilon-input
    arc, olabel 9, weight 0..wmax, that moves `eps` layers on (1: the rhs stays layered;
    2: breadth-first levels stop being layers).  split: the arcs of the k-th label go to
    the k-th part of the next layer only, so every state has in-arcs of one label (the pull
    tiers' direct layout, which the 4-B records and the packed cells need)."""
    part = W // len(labels) if split else W
    assert fan <= part and fan <= 8
    f = O.Fst()
    for _ in range(1 + T * W):
        f.add_state(0.0 if rng.random() < 2 / 3 else math.inf)
    f.start = 0

    def layer(t):
        return [0] if t == 0 else list(range(1 + (t - 1) * W, 1 + t * W))

    for t in range(T):
        nxt = layer(t + 1)
        for s in layer(t):
            for k, il in enumerate(labels):
                tg = rng.choice(part, fan, replace=False) + (k * part if split else 0)
                ol = rng.choice(8, fan, replace=False) + 1
                for j in range(fan):
                    f.add_arc(s, int(il), int(ol[j]), float(rng.integers(0, wmax + 1)), nxt[int(tg[j])])
            if eps and rng.random() < 1 / 3:
                far = layer(min(T, t + eps))
                f.add_arc(s, 0, 9, float(rng.integers(0, wmax + 1)), far[int(rng.integers(len(far)))])
    return f


def shifted(f: O.Fst, dw) -> O.Fst:
    """Every arc weight + dw (0.5: dyadic; 0.1: neither an integer nor dyadic)."""
    return O.Fst(start=f.start, finals=list(f.finals),
                 arcs=[[(a, b, w + dw, d) for (a, b, w, d) in al] for al in f.arcs])


def mutant_best(f, seq, ident):
    """A plain Viterbi 1-best of `seq` through an epsilon-free rhs that breaks every tie
    towards the smaller ident[state]: between two best arcs into one state the one from the
    smaller-ident source (then the earlier arc), between two best final states the
    smaller-ident one.  Returns (olabel sequence or None, number of co-optimal paths)."""
    start, arcs = frozen(f)
    blob = as_blob(f)
    ns = len(arcs)
    fin = np.frombuffer(blob, STATE_DTYPE, ns, 24)["fin"] if ns else []
    if start >= ns:
        return None, 0
    cur = {start: (0.0, 1, ())}  # state -> (cost, co-optimal prefixes, olabels)
    for x in seq:
        nxt = {}
        for s in sorted(cur, key=lambda q: ident[q]):
            c, n, path = cur[s]
            for il, ol, w, t in arcs[s]:
                assert il != 0
                if il != x:
                    continue
                d = c + w
                if t not in nxt or d < nxt[t][0]:
                    nxt[t] = (d, n, path + (ol,))
                elif d == nxt[t][0]:
                    nxt[t] = (d, nxt[t][1] + n, nxt[t][2])
        cur = nxt
    best, count = None, 0
    for s in sorted(cur, key=lambda q: ident[q]):
        c, n, path = cur[s]
        if math.isinf(fin[s]):
            continue
        d = c + float(fin[s])
        if best is None or d < best[0]:
            best, count = (d, path), n
        elif d == best[0]:
            count += n
    return (None, 0) if best is None else (list(best[1]), count)


# ---------------------------------------------------------------------------------------
# the cases of test_gpu_renumber.py
# ---------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    name: str
    cls: str          # "A" the band is lost, "B" the band is gained, "C" cyclic
    fst: O.Fst
    blob: bytes
    seqs: tuple
    eps: bool         # the rhs has input epsilons
    tie: bool         # an epsilon-free tie_rhs: the co-optimal and mutant shares apply


def rand_seqs(seed, labels, count, max_len, min_len=0):
    rng = np.random.default_rng(seed)
    seqs = [[int(rng.choice(labels)) for _ in range(int(rng.integers(min_len, max_len + 1)))]
            for _ in range(count - 2)]
    return seqs + [[], [int(labels[0])] * max_len]


def cyclic_rhs():
    """Class C: cycles, epsilons, weights 0..3, four labels on nearly every state."""
    from test_gpu_parity import random_rhs
    return random_rhs(np.random.default_rng(1012), 40, 480, 3, eps=True, wmax=3)


BYTE_LABELS = (98, 99)  # b"a", b"b" as the text entry's labels (byte + 1)


def _build():
    from test_gpu_edge_labels import marker_rhs, marker_seqs
    out = []

    def add(name, cls, f, seqs, tie=False):
        blob = O.freeze(f)
        eps = any(a[0] == 0 for al in f.arcs for a in al)
        out.append(Case(name, cls, f, blob, tuple(tuple(s) for s in seqs), eps, tie))

    add("A-marker-eps", "A", marker_rhs(True), marker_seqs())
    add("A-marker-noeps", "A", marker_rhs(False), marker_seqs())
    add("A-tie-eps", "A", tie_rhs(np.random.default_rng(31), 14, 4, (1, 2), 3, 1, 2),
        rand_seqs(32, (1, 2), 64, 13))
    # (strings of three labels or more: a shorter one has too few paths to tie)
    base = tie_rhs(np.random.default_rng(50), 14, 4, (1, 2), 3, 1, 0)
    seqs = rand_seqs(52, (1, 2), 64, 13, 3)
    add("B-tie", "B", scattered(base, 51), seqs, tie=True)
    add("B-tie-half", "B", scattered(shifted(base, 0.5), 51), seqs, tie=True)
    add("B-tie-tenth", "B", scattered(shifted(base, 0.1), 51), seqs, tie=True)
    wide = tie_rhs(np.random.default_rng(60), 14, 6, (1, 2), 3, 1, 0, split=True)
    add("B-split", "B", scattered(wide, 61), seqs, tie=True)
    add("B-split-half", "B", scattered(shifted(wide, 0.5), 61), seqs, tie=True)
    add("B-split-tenth", "B", scattered(shifted(wide, 0.1), 61), seqs, tie=True)
    add("B-tie-bytes", "B",
        scattered(tie_rhs(np.random.default_rng(41), 14, 4, BYTE_LABELS, 3, 1, 0), 42),
        rand_seqs(43, BYTE_LABELS, 64, 13, 3), tie=True)
    add("B-tie-eps", "B", scattered(tie_rhs(np.random.default_rng(22), 14, 4, (1, 2), 3, 1, 1), 23),
        rand_seqs(24, (1, 2), 64, 13))
    add("B-eps-dense", "B", scattered(O.gen("eps_dense", 64, 12), 5),
        [[1] * (i % 16) for i in range(32)])
    add("B-ambiguous", "B", scattered(O.gen("ambiguous", 256, 12), 5),
        [[1] * (i % 16) for i in range(32)])
    add("C-cyclic", "C", cyclic_rhs(), rand_seqs(1013, (1, 2, 3), 64, 5))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


def small_lhs():
    """Ten small random lhs (epsilons, cycles) for the single calls and fst_compose_frozen,
    64 for the lhs batch entry."""
    from test_gpu_parity import random_rhs
    rng = np.random.default_rng(3100)
    return [random_rhs(rng, int(rng.integers(1, 8)), int(rng.integers(2, 20)), 3, eps=True)
            for _ in range(64)]


def no_start_rhs() -> O.Fst:
    return O.Fst(finals=[0.0, 0.0, math.inf], arcs=[[(1, 1, 0.0, 1)], [(1, 2, 1.0, 2)], []])


def one_state_rhs() -> O.Fst:
    return O.Fst(start=0, finals=[0.5], arcs=[[(1, 7, 0.25, 0), (1, 8, 0.25, 0), (0, 3, 1.0, 0)]])
