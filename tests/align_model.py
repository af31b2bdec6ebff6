"""The alignment of include/fst_batch.h (FstAlignedTextResult), restated from per-stage paths.

A path is (ilabels, olabels); `align` takes one string's paths, stage by stage, and returns
(begin, end) per symbol of the last stage's output."""


def stage_map(il, ol):
    """(b, e, N) of one path: per non-epsilon olabel the consumed-input interval of its arc."""
    b, e, n = [], [], 0
    for i, o in zip(il, ol):
        step = int(i != 0)
        if o != 0:
            b.append(n)
            e.append(n + step)
        n += step
    return b, e, n


def compose(B, E, b, e, n1):
    """Stage s's (b, e) through the running map (B, E) of stage s-1's M output symbols."""
    M = len(B)
    lo = [B[x] if x < M else n1 for x in b]
    return lo, [E[x] if y > x else l for x, y, l in zip(b, e, lo)]


def align(paths):
    B, E, n1 = stage_map(*paths[0])
    for il, ol in paths[1:]:
        b, e, _ = stage_map(il, ol)
        B, E = compose(B, E, b, e, n1)
    return B, E
