"""Beam pruning as include/fst_batch.h defines it (fst_prune_lhs_batch), restated twice for the
tests.  Written from the header's comment, not from the library's kernels.

(a) prune(): numpy.  F and B by plain relaxation of every arc until nothing changes, then the
    cut on f64 values, then connect_model.connect of the item with the kept arcs and finals:
      F(start) = 0.0, F(dst) = min(F(dst), F(src) + w);
      B(s) = final(s) if final else +inf, B(src) = min(B(src), w + B(dst));
      best = min over final t of F(t) + final(t); limit = best + beam;
      arc kept iff (F(src) + w) + B(dst) is not +inf and <= limit;
      a final weight kept iff F(s) + final(s) is not +inf and <= limit.
(b) prune_brute(): small acyclic items whose sums are exact (weights that are small integers or
    halves).  Every complete path is enumerated with its total by the definition's folds; an
    arc is kept iff it lies on a path of total <= limit, a final weight iff the path that ends
    there does.
Both return (status, Trimmed): status 0 (OK) or 5 (UNSUPPORTED, with the empty FST).
"""
import math

import numpy as np

import connect_model as CM

OK, UNSUPPORTED = 0, 5
INF = math.inf
NO_STATE = CM.NO_STATE


def _arrays(start, finals, arcs):
    off = np.concatenate([[0], np.cumsum([len(al) for al in arcs])]).astype(np.int64)
    flat = [x for al in arcs for x in al]
    col = lambda k, dt: np.array([x[k] for x in flat], dt)
    return (np.array(finals, np.float64), off, col(0, np.uint32), col(1, np.uint32),
            col(2, np.float64), col(3, np.uint32))


def _precheck(start, finals, w):
    """None to go on, or the (status, Trimmed) of rules 1 and 2."""
    n, a = len(finals), len(w)
    if start is None or int(start) == NO_STATE or n == 0:
        return OK, CM._empty(n, a)
    if np.isnan(finals).any() or np.isnan(w).any() or (w < 0.0).any():
        return UNSUPPORTED, CM._empty(n, a)
    return None


def distances(start, finals, off, w, nxt):
    """(F, B) by relaxing every arc until nothing changes."""
    n = len(finals)
    F = [INF] * n
    F[start] = 0.0
    B = [f if not math.isinf(f) else INF for f in finals.tolist()]
    src = np.repeat(np.arange(n), np.diff(off)).tolist()
    arcs = list(zip(src, nxt.tolist(), w.tolist()))
    for _ in range(n * len(arcs) + 2):
        changed = False
        for s, t, x in arcs:
            f = F[s] + x
            if f < F[t]:
                F[t] = f
                changed = True
            b = x + B[t]
            if b < B[s]:
                B[s] = b
                changed = True
        if not changed:
            return np.array(F, np.float64), np.array(B, np.float64)
    raise AssertionError("the relaxation did not settle")


def prune(start, finals, arcs, beam, dist=None):
    """Model (a) of one item given as (start, finals, arcs per state as (il, ol, w, next)).
    dist: a dict that keeps the item's distances from one beam to the next."""
    finals, off, il, ol, w, nxt = _arrays(start, finals, arcs)
    pre = _precheck(start, finals, w)
    if pre is not None:
        return pre
    n, a = len(finals), len(w)
    start = int(start)
    dist = {} if dist is None else dist
    if "FB" not in dist:
        dist["FB"] = distances(start, finals, off, w, nxt)
    F, B = dist["FB"]
    is_final = ~np.isinf(finals)
    with np.errstate(invalid="ignore", over="ignore"):
        tot = F + finals
        best = tot[is_final].min() if is_final.any() else INF
        if best == INF:
            return OK, CM._empty(n, a)
        limit = best + beam
        src = np.repeat(np.arange(n), np.diff(off))
        T = (F[src] + w) + B[nxt.astype(np.int64)]
        keep_arc = ~np.isinf(T) & (T <= limit)
        keep_fin = is_final & ~np.isinf(tot) & (tot <= limit)
    cut_finals = np.where(keep_fin, finals, INF)
    deg = np.bincount(src[keep_arc], minlength=n)
    cut_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    t = CM.connect(start, cut_finals, cut_off, il[keep_arc], ol[keep_arc], w[keep_arc],
                   nxt[keep_arc])
    t.states_in, t.arcs_in = n, a
    return OK, t


def prune_brute(start, finals, arcs, beam):
    """Model (b): every complete path of a small acyclic item with exact sums."""
    finals, off, il, ol, w, nxt = _arrays(start, finals, arcs)
    pre = _precheck(start, finals, w)
    if pre is not None:
        return pre
    n, a = len(finals), len(w)
    start = int(start)
    is_final = ~np.isinf(finals)
    paths = []  # (total, arc indices, final state)

    def walk(s, g, used):
        if is_final[s]:
            paths.append((g + finals[s], tuple(used), s))
        for k in range(int(off[s]), int(off[s + 1])):
            if math.isinf(w[k]):
                continue        # an arc of weight +inf is never part of a path
            assert len(used) < n, "prune_brute is for acyclic items"
            walk(int(nxt[k]), g + w[k], used + [k])

    walk(start, 0.0, [])
    paths = [p for p in paths if not math.isinf(p[0])]
    if not paths:
        return OK, CM._empty(n, a)
    limit = min(p[0] for p in paths) + beam
    keep_arc = np.zeros(a, bool)
    keep_fin = np.zeros(n, bool)
    for total, used, t in paths:
        if total <= limit:
            keep_arc[list(used)] = True
            keep_fin[t] = True
    src = np.repeat(np.arange(n), np.diff(off))
    cut_finals = np.where(keep_fin, finals, INF)
    deg = np.bincount(src[keep_arc], minlength=n)
    cut_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    t = CM.connect(start, cut_finals, cut_off, il[keep_arc], ol[keep_arc], w[keep_arc],
                   nxt[keep_arc])
    t.states_in, t.arcs_in = n, a
    return OK, t


def prune_batch(fsts, beam, cache=None):
    """Model (a) of a list of items, as the arrays of the library's result:
    dict(status, start, state_offsets, arc_offsets, finals, il, ol, w, next).  cache: a list of
    one dict per item, kept by the caller across beams (the distances do not depend on it)."""
    status, start, so, ao = [], [], [0], [0]
    fin, il, ol, w, nx = [], [], [], [], []
    for i, (st, finals, arcs) in enumerate(fsts):
        s, t = prune(st, finals, arcs, beam, cache[i] if cache is not None else None)
        status.append(s)
        start.append(t.start)
        base = ao[-1]
        ao.extend((t.off[1:].astype(np.int64) + base).tolist())
        so.append(so[-1] + len(t.finals))
        fin.append(t.finals)
        il.append(t.il)
        ol.append(t.ol)
        w.append(t.w)
        nx.append(t.next)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return dict(status=np.array(status, np.int32), start=np.array(start, np.uint32),
                state_offsets=np.array(so, np.uint64), arc_offsets=np.array(ao, np.uint64),
                finals=cat(fin, np.float64), il=cat(il, np.uint32), ol=cat(ol, np.uint32),
                w=cat(w, np.float64), next=cat(nx, np.uint32))


def assert_batch_equal(got, exp, what=""):
    """A LatticeBatch against prune_batch's dict, bit for bit."""
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    assert got.status.tolist() == exp["status"].tolist(), what
    assert got.start.tolist() == exp["start"].tolist(), what
    assert got.state_offsets.tolist() == exp["state_offsets"].tolist(), what
    assert got.arc_offsets.tolist() == exp["arc_offsets"].tolist(), what
    assert np.array_equal(bits(got.final_weights), bits(exp["finals"])), what
    assert np.array_equal(got.ilabels, exp["il"]), what
    assert np.array_equal(got.olabels, exp["ol"]), what
    assert np.array_equal(bits(got.weights), bits(exp["w"])), what
    assert np.array_equal(got.nextstates, exp["next"]), what
