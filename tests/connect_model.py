"""connect (trim) as the reference defines it (src/ops/connect.zig:17-124), restated in numpy
for the tests of FST_LATTICE_CONNECT and fst_connect_lhs_batch.  Written from the description
of the operation, not from the library's kernels:

  - no start or no states: the empty FST;
  - accessible = forward closure of the start; coaccessible = backward closure of the final
    states, final meaning the weight is not +-inf (so -inf is not final and NaN is);
  - kept = accessible and coaccessible, new id = rank among the kept states in increasing old
    id; the start not kept: the empty FST;
  - a kept state's final weight is copied bit for bit when final, else +inf;
  - its arcs are the old arcs whose target is kept, in the old order, targets renumbered,
    labels and weights copied bit for bit.
"""
from dataclasses import dataclass

import numpy as np

NO_STATE = 0xFFFFFFFF


@dataclass
class Trimmed:
    start: int           # NO_STATE for the empty FST
    finals: np.ndarray   # f64 [n]
    off: np.ndarray      # u64 [n + 1] arc offsets local to the item
    il: np.ndarray       # u32 [a]
    ol: np.ndarray
    w: np.ndarray        # f64 [a]
    next: np.ndarray     # u32 [a]
    states_in: int = 0
    arcs_in: int = 0


def _empty(n, a):
    return Trimmed(NO_STATE, np.zeros(0, np.float64), np.zeros(1, np.uint64),
                   np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float64),
                   np.zeros(0, np.uint32), n, a)


def _closure(seeds, off, nbr, n):
    """The states reachable from `seeds` over the CSR (off, nbr)."""
    seen = np.zeros(n, bool)
    seen[seeds] = True
    stack = [int(s) for s in seeds]
    while stack:
        s = stack.pop()
        for t in nbr[off[s]:off[s + 1]].tolist():
            if not seen[t]:
                seen[t] = True
                stack.append(t)
    return seen


def connect(start, finals, off, il, ol, w, nxt) -> Trimmed:
    """connect of one FST given as CSR arrays (off: n + 1 local arc offsets)."""
    finals = np.ascontiguousarray(finals, np.float64)
    off = np.ascontiguousarray(off).astype(np.int64)
    off = off - off[0] if len(off) else np.zeros(1, np.int64)
    il, ol = np.ascontiguousarray(il, np.uint32), np.ascontiguousarray(ol, np.uint32)
    w, nxt = np.ascontiguousarray(w, np.float64), np.ascontiguousarray(nxt, np.uint32)
    n, a = len(finals), len(nxt)
    if start is None or int(start) == NO_STATE or n == 0:
        return _empty(n, a)
    start = int(start)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    tgt = nxt.astype(np.int64)
    accessible = _closure([start], off, tgt, n)
    order = np.argsort(tgt, kind="stable")           # the reverse CSR: arcs by target
    roff = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))])
    is_final = ~np.isinf(finals)
    coaccessible = _closure(np.flatnonzero(is_final), roff, src[order], n)
    kept = accessible & coaccessible
    if not kept[start]:
        return _empty(n, a)
    new_id = np.cumsum(kept) - 1
    keep_arc = kept[src] & kept[tgt]
    out_fin = finals[kept].copy()
    out_fin[~is_final[kept]] = np.inf
    deg = np.bincount(new_id[src[keep_arc]], minlength=int(kept.sum()))
    out_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    return Trimmed(int(new_id[start]), out_fin, out_off, il[keep_arc], ol[keep_arc],
                   w[keep_arc], new_id[tgt[keep_arc]].astype(np.uint32), n, a)


def connect_lists(start, finals, arcs) -> Trimmed:
    """connect of (start, finals, arcs per state as (il, ol, w, next) lists)."""
    off = np.concatenate([[0], np.cumsum([len(al) for al in arcs])]).astype(np.uint64)
    flat = [x for al in arcs for x in al]
    col = lambda k, dt: np.array([x[k] for x in flat], dt)
    return connect(start, finals, off, col(0, np.uint32), col(1, np.uint32), col(2, np.float64),
                   col(3, np.uint32))


def connect_csr(c) -> Trimmed:
    """connect of an oracle_ffi.Csr (O.compose_csr's result)."""
    start = c.start if len(c.finals) else NO_STATE
    return connect(start, c.finals, c.off, c.arcs["il"], c.arcs["ol"], c.arcs["w"],
                   c.arcs["next"])


def to_lists(t: Trimmed):
    """(start, finals, arcs per state) of a Trimmed, weights as bit patterns."""
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()
    arcs = []
    for s in range(len(t.finals)):
        b, e = int(t.off[s]), int(t.off[s + 1])
        arcs.append(list(zip(t.il[b:e].tolist(), t.ol[b:e].tolist(), bits(t.w[b:e]),
                             t.next[b:e].tolist())))
    return t.start, bits(t.finals), arcs
