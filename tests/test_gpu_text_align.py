"""GPU tests of the aligned text entry: fst_normalize_text_aligned_batch (bytes in, bytes out,
plus the input span of every output byte) and the device pieces fst_device_path_alignment /
fst_device_compose_alignment.

The expected maps come from the CPU oracle's paths, stage by stage (O.batch_run with the
projection of test_gpu_configs.oracle_pipeline), through tests/align_model.py; text, offsets,
statuses and weights must equal fst_normalize_text_batch's on the same inputs bit for bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import libfst_amd as F
from libfst_amd import fst as FF
import oracle_ffi as O
from align_model import align, compose, stage_map
from test_gpu_configs import oracle_pipeline
from test_gpu_parity import EAGER, LAZY, bits
from test_gpu_text import COPY_DELETE, config4, lab, rhs_blob, to_labels
from test_text_api import python_text

pytestmark = pytest.mark.gpu

OK, EMPTY, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED
INF = math.inf


def expected(blobs, texts, sem):
    """(texts, status, total weights, [(begin, end) per string], [arcs of the stage-1 path])
    from the oracle's paths of every stage."""
    labels, offsets = to_labels(texts)
    stages = [oracle_pipeline(blobs[:k + 1], labels, offsets, sem)[0] for k in range(len(blobs))]
    ref, exp = oracle_pipeline(blobs, labels, offsets, sem)
    r = F.BatchResult(status=exp, offsets=ref.offsets, ilabels=ref.ilabels, olabels=ref.olabels,
                      weights=ref.weights, finals=ref.finals)
    out, status, tw = python_text(r)
    maps = []
    for i in range(len(texts)):
        if status[i] != OK:
            maps.append(([], []))
            continue
        cut = lambda s: (int(s.offsets[i]), int(s.offsets[i + 1]))
        maps.append(align([(s.ilabels[cut(s)[0]:cut(s)[1]].tolist(),
                            s.olabels[cut(s)[0]:cut(s)[1]].tolist()) for s in stages]))
    arcs = [int(stages[0].offsets[i + 1]) - int(stages[0].offsets[i]) for i in range(len(texts))]
    return out, status, tw, maps, arcs


def invariants(got, texts):
    b, e = got.in_begin.astype(np.int64), got.in_end.astype(np.int64)
    assert len(b) == len(e) == len(got.text)
    assert np.all(b <= e)
    for i, t in enumerate(texts):
        a, z = int(got.offsets[i]), int(got.offsets[i + 1])
        assert np.all(e[a:z] <= len(t)), i
        assert np.all(e[a:max(z - 1, a)] <= b[a + 1:max(z, a + 1)]), i


def same_text(a, b):
    for x, y in ((a.status, b.status), (a.offsets, b.offsets), (a.text, b.text),
                 (a.total_weight, b.total_weight)):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def same_all(a, b):
    same_text(a, b)
    assert a.in_begin.tobytes() == b.in_begin.tobytes()
    assert a.in_end.tobytes() == b.in_end.tobytes()


def check_aligned(blobs, texts, sem, want=None, **kw):
    stages = [F.Fst.from_bytes(b) for b in blobs]
    got = F.normalize_text_aligned_batch(stages, texts, sem, **kw)
    out, status, tw, maps, _ = want or expected(blobs, texts, sem)
    assert np.array_equal(got.status, status), np.nonzero(got.status != status)[0][:10]
    assert got.texts() == out
    assert np.array_equal(bits(got.total_weight), bits(tw))
    same_text(got, F.normalize_text_batch(stages, texts, sem, **kw))
    invariants(got, texts)
    for i, (b, e) in enumerate(maps):
        a, z = int(got.offsets[i]), int(got.offsets[i + 1])
        assert got.in_begin[a:z].tolist() == b, (i, texts[i])
        assert got.in_end[a:z].tolist() == e, (i, texts[i])
    return got


# ---- 1. one stage: copies, deletions and insertions across the 64-arc passes ------------

# COPY_DELETE ('a', 'x' copied, 'd' deleted) plus 'i' -> "i!": i:i, then an input-epsilon arc
# that emits '!' (two arcs for one byte)
COPY_DELETE_INSERT = COPY_DELETE + [(0, lab("i"), lab("i"), 0.4, 1), (1, 0, lab("!"), 0.6, 0)]


def pass_edge_texts():
    rng = np.random.default_rng(3)
    texts = []
    for P in (0, 1, 63, 64, 65, 127, 128, 129, 200):     # arcs of the path
        texts.append(b"x" * P)
        texts.append(bytes(rng.choice(list(b"adx"), P).tolist()))
        k = P // 5                                         # k insertions: P - 2k other arcs
        s = [ord("i")] * k + rng.choice(list(b"adx"), P - 2 * k).tolist()
        texts.append(bytes(rng.permutation(s).tolist()))
    for P in (129, 200):
        tail = b"x" * (P - 65)
        texts += [b"x" * 63 + b"dd" + tail,               # deletions on arcs 63 and 64
                  b"x" * 63 + b"xx" + tail,               # copies
                  b"x" * 62 + b"i" + b"x" + tail[1:],      # the insertion on arc 63
                  b"x" * 63 + b"i" + tail,                 # ... on arc 64 (P + 1 arcs)
                  b"d" * 62 + b"i" + b"d" * 70]            # the only bytes come from arcs 62, 63
    texts += [b"d" * 130, b"i" * 100, b"i"]
    return texts


@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_one_stage_pass_edges(sem):
    blob = rhs_blob(COPY_DELETE_INSERT, finals=(0.2, INF))
    texts = pass_edge_texts()
    want = expected([blob], texts, sem)
    assert all(s == OK for s in want[1])
    assert {0, 1, 63, 64, 65, 127, 128, 129, 200} <= set(want[4])
    got = check_aligned([blob], texts, sem, want)
    i = texts.index(b"d" * 62 + b"i" + b"d" * 70)
    assert got.texts()[i] == b"i!" and got.spans(i) == [(62, 63, 0, 1), (63, 63, 1, 2)]


def test_copy_only_rhs_is_the_identity():
    blob = rhs_blob([(0, lab(c), lab(c), 0.25, 0) for c in "ax"])
    texts = [b"", b"a", b"ax" * 32, b"x" * 65, b"a" * 200, b"xa"]
    for sem in (LAZY, EAGER):
        got = check_aligned([blob], texts, sem)
        for i, t in enumerate(texts):
            a, z = int(got.offsets[i]), int(got.offsets[i + 1])
            assert got.in_begin[a:z].tolist() == list(range(len(t)))
            assert got.in_end[a:z].tolist() == list(range(1, len(t) + 1))
            assert got.spans(i) == ([(0, len(t), 0, len(t))] if t else [])


# ---- 2. two stages: tagger -> verbalizer -------------------------------------------------

@functools.lru_cache(maxsize=None)
def config4_aligned(sem):
    blobs, texts, _ = config4(sem)
    return blobs, texts, expected(list(blobs), texts, sem)


@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_tagger_verbalizer_aligned(sem):
    blobs, texts, want = config4_aligned(sem)
    assert len(texts) == 305 and b"" in texts and b"##" in texts and b"7" in texts
    got = check_aligned(list(blobs), texts, sem, want)
    assert (want[1] == OK).sum() > 0.9 * len(texts) - 5
    i = texts.index(b"7")
    a, z = int(got.offsets[i]), int(got.offsets[i + 1])
    assert got.texts()[i] == b"seven"
    # every byte's interval lies inside the one input byte: 0 <= begin <= end <= 1.  (By the
    # definition the five bytes carry [1, 1): the tagger gives "#h" and the verbalizer emits the
    # word on input-epsilon arcs after both symbols are consumed, b == M; check_aligned above
    # compared exactly that with the model.)
    assert np.all(got.in_begin[a:z] <= got.in_end[a:z]) and np.all(got.in_end[a:z] <= 1)
    assert want[3][i] == ([1] * 5, [1] * 5)
    i = texts.index(b"##")   # fails at stage 1: no bytes, no entries
    assert got.status[i] == EMPTY and got.offsets[i] == got.offsets[i + 1]
    # the maps say something: some string has a rewritten digit between copied letters
    assert any(len(got.spans(k)) >= 3 for k in range(len(texts)))


# ---- 3. three stages: M == 0 and b == M ---------------------------------------------------

def three_stages():
    s1 = rhs_blob(COPY_DELETE + [(0, lab("q"), lab("a"), 0.4, 1), (1, 0, lab("a"), 0.6, 0)],
                  finals=(0.2, INF))                                  # q -> "aa"
    s2 = rhs_blob([(0, lab("a"), lab("a"), 0.1, 0), (0, lab("x"), 0, 0.3, 0)])   # x deleted
    # 'a' copied; the path ends on two input-epsilon arcs taken once the input is exhausted
    s3 = rhs_blob([(0, lab("a"), lab("a"), 0.1, 0), (0, 0, lab("!"), 0.5, 1),
                   (1, 0, lab("?"), 0.5, 2)], finals=(INF, INF, 0.0))
    return [s1, s2, s3]


def test_three_stages_empty_middle_and_trailing_insertions():
    blobs = three_stages()
    rng = np.random.default_rng(8)
    texts = [b"", b"x", b"xxdx", b"d", b"a", b"q", b"axqda", b"z", b"xq", b"x" * 70, b"ax" * 40]
    texts += [bytes(rng.choice(list(b"axdq"), int(n)).tolist()) for n in rng.integers(1, 70, 20)]
    for sem in (LAZY, EAGER):
        want = expected(blobs, texts, sem)
        got = check_aligned(blobs, texts, sem, want)
        assert got.texts()[:8] == [b"!?", b"!?", b"!?", b"!?", b"a!?", b"aa!?", b"aaaa!?", b""]
        assert got.status[7] == EMPTY
        # M == 0 (stage 2 gave nothing): both bytes sit at N1, the end of the input
        assert got.spans(2) == [(4, 4, 0, 2)] and got.spans(0) == [(0, 0, 0, 2)]
        # b == M: the trailing bytes sit at N1 behind the mapped ones
        assert got.spans(5) == [(0, 1, 0, 1), (1, 1, 1, 4)]
        assert got.spans(6)[-1] == (5, 5, 4, 6)


# ---- 4. shards ---------------------------------------------------------------------------

@pytest.mark.parametrize("stream", ["0", None])
def test_shards_give_identical_bytes(monkeypatch, stream):
    if stream is None:
        monkeypatch.delenv("FSTAMD_STREAM", raising=False)
    else:
        monkeypatch.setenv("FSTAMD_STREAM", stream)
    blobs, texts, want = config4_aligned(LAZY)
    stages = [F.Fst.from_bytes(b) for b in blobs]
    plain = F.normalize_text_aligned_batch(stages, texts, LAZY)
    one = check_aligned(list(blobs), texts, LAZY, want, devices=[0], shards=1)
    three = check_aligned(list(blobs), texts, LAZY, want, devices=[0], shards=3)
    same_all(one, plain)
    same_all(three, one)
    # one stage, which the text entry streams unless told not to: the aligned entry never does
    blob = rhs_blob(COPY_DELETE, finals=(0.2,))
    rng = np.random.default_rng(5)
    short = [bytes(rng.choice(list(b"adx"), int(n)).tolist()) for n in rng.integers(0, 90, 64)]
    w1 = expected([blob], short, LAZY)
    same_all(check_aligned([blob], short, LAZY, w1, devices=[0], shards=3),
             check_aligned([blob], short, LAZY, w1))


# ---- 5. the device pieces ----------------------------------------------------------------

GUARD = 0xEEEEEEEE


def device_batch(paths):
    """An FstDeviceBatch from [(status, ilabels, olabels)], laid out back to front with gaps
    (the gaps hold non-byte labels: never read).  Returns (desc, tensors kept alive)."""
    dev = torch.device("cuda", 0)
    n = len(paths)
    poff, pos = [0] * n, 3
    for i in reversed(range(n)):
        poff[i] = pos
        pos += len(paths[i][1]) + (i % 3)
    cap = pos + 5
    il = np.full(cap, 300, np.uint32)
    ol = np.full(cap, 300, np.uint32)
    for i, p in enumerate(paths):
        il[poff[i]:poff[i] + len(p[1])] = p[1]
        ol[poff[i]:poff[i] + len(p[2])] = p[2]
    t = lambda a, dt: torch.as_tensor(np.asarray(a).astype(dt), device=dev)
    keep = [t([p[0] for p in paths], np.int32), t([len(p[1]) for p in paths], np.int32),
            t(poff, np.int64), t(np.zeros(n), np.float64), t(il.view(np.int32), np.int32),
            t(ol.view(np.int32), np.int32), t(np.full(cap, 0.5), np.float64),
            torch.zeros(1, dtype=torch.int64, device=dev)]
    desc = FF.FstDeviceBatch(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                             keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(),
                             keep[6].data_ptr(), cap, keep[7].data_ptr(), 0)
    return desc, keep


def hand_paths():
    rng = np.random.default_rng(9)
    paths = []
    for L in [0, 1, 5, 63, 64, 65, 127, 128, 129, 200, 7, 3, 2, 1, 0, 70]:
        il, ol = rng.integers(0, 257, L), rng.integers(0, 257, L)
        il[rng.random(L) < 0.4] = 0
        ol[rng.random(L) < 0.4] = 0
        paths.append((OK, il.tolist(), ol.tolist()))
    paths[10] = (OK, [5, 6, 7, 0, 1, 2, 3], [5, 257, 6, 0, 1, 2, 3])      # a non-byte label
    paths[11] = (EMPTY, [], [])
    paths[12] = (F.FST_PATH_CYCLE, [9, 9], [9, 9])                        # a failed string's arcs
    paths[15] = (OK, [0] * 60 + [4] * 10, [0] * 66 + [256, 1, 0, 98])     # bytes from pass 2 on
    return paths


def path_alignment(desc, n, off, capacity, guard=16):
    dev = torch.device("cuda", 0)
    mk = lambda: torch.full((capacity + guard,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
    b, e = mk(), mk()
    cons = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rc = F.lib().fst_device_path_alignment(C.byref(desc), n, C.c_void_p(off.data_ptr()),
                                           C.c_void_p(b.data_ptr()), C.c_void_p(e.data_ptr()),
                                           capacity, C.c_void_p(cons.data_ptr()), None)
    assert rc == FF.FST_OK
    torch.cuda.synchronize()
    return (b.cpu().numpy().view(np.uint32), e.cpu().numpy().view(np.uint32), cons.cpu().numpy())


def test_device_path_alignment_at_text_and_projection_offsets():
    dev = torch.device("cuda", 0)
    paths = hand_paths()
    n = len(paths)
    desc, keep = device_batch(paths)
    good = [p[0] == OK and all(x <= 256 for x in p[2]) for p in paths]
    maps = [stage_map(p[1], p[2]) if g else ([], [], 0) for p, g in zip(paths, good)]
    # (a) at the offsets of fst_device_emit_text
    toff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    tw = torch.zeros(n, dtype=torch.float64, device=dev)
    total = FF._u64(0)
    assert F.lib().fst_device_emit_text(C.byref(desc), n, None, 0, C.c_void_p(toff.data_ptr()),
                                        C.c_void_p(st.data_ptr()), C.c_void_p(tw.data_ptr()),
                                        C.byref(total), None) == FF.FST_OK
    need = int(total.value)
    wb = np.asarray([x for m in maps for x in m[0]], np.uint32)
    we = np.asarray([x for m in maps for x in m[1]], np.uint32)
    assert need == len(wb) and st.cpu().numpy()[10] == UNSUPPORTED
    for capacity in (need, need - 1, need - 37, 0):
        b, e, cons = path_alignment(desc, n, toff, capacity)
        assert np.array_equal(b[:capacity], wb[:capacity])
        assert np.array_equal(e[:capacity], we[:capacity])
        assert np.all(b[capacity:] == GUARD) and np.all(e[capacity:] == GUARD)   # nothing past it
        assert cons.tolist() == [m[2] for m in maps]
    # (b) at the offsets of fst_device_project_output: a failed string owns one dead label
    plab = torch.zeros(need + n, dtype=torch.int32, device=dev)
    poff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    pst = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ml = FF._u32(0)
    assert F.lib().fst_device_project_output(C.byref(desc), n, C.c_void_p(plab.data_ptr()),
                                             C.c_void_p(poff.data_ptr()),
                                             C.c_void_p(pst.data_ptr()), C.byref(ml),
                                             None) == FF.FST_OK
    off = poff.cpu().numpy()
    ptotal = int(off[-1])
    assert ptotal == need + good.count(False)
    for capacity in (ptotal, ptotal - 1):
        b, e, cons = path_alignment(desc, n, poff, capacity)
        for i, m in enumerate(maps):
            a, z = int(off[i]), min(int(off[i + 1]), capacity)
            wbi, wei = (m[0], m[1]) if good[i] else ([0], [0])
            k = max(z - a, 0)
            assert b[a:a + k].tolist() == wbi[:k] and e[a:a + k].tolist() == wei[:k], i
        assert np.all(b[capacity:] == GUARD) and np.all(e[capacity:] == GUARD)
        assert cons.tolist() == [m[2] for m in maps]
    del keep


def test_device_compose_alignment():
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    inner, outer, n1 = [], [], []
    for M, Q in [(0, 0), (0, 3), (1, 0), (1, 5), (5, 1), (64, 64), (65, 130), (130, 65), (7, 200)]:
        # a running map of M symbols over N1 bytes, then (b, e) of Q symbols into them
        N1 = int(rng.integers(M, 2 * M + 3))
        B = np.sort(rng.integers(0, N1 + 1, M))
        E = np.minimum(B + rng.integers(0, 2, M), np.append(B[1:], N1)) if M else B
        b = np.sort(rng.integers(0, M + 1, Q))           # b == M among them
        e = np.where(b < M, b + rng.integers(0, 2, Q), b)
        inner.append((B.tolist(), E.tolist()))
        outer.append((b.tolist(), e.tolist()))
        n1.append(N1)
    assert any(M in b for (b, _), (M, _) in zip(outer, [(len(x[0]), 0) for x in inner]))
    csr = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    flat = lambda parts: np.asarray([x for p in parts for x in p], np.int64).astype(np.int32)
    t = lambda a: torch.as_tensor(a, device=dev)
    ooff, ioff = t(csr([o[0] for o in outer])), t(csr([i[0] for i in inner]))
    ob, oe = t(flat([o[0] for o in outer])), t(flat([o[1] for o in outer]))
    ib, ie = t(flat([i[0] for i in inner])), t(flat([i[1] for i in inner]))
    cons = t(np.asarray(n1, np.int32))
    want = [compose(i[0], i[1], o[0], o[1], n) for i, o, n in zip(inner, outer, n1)]
    wb, we = flat([w[0] for w in want]), flat([w[1] for w in want])
    total = len(wb)
    P = lambda x: C.c_void_p(x.data_ptr())
    for capacity in (total, total - 1):
        rb = torch.full((total + 8,), -7, dtype=torch.int32, device=dev)
        re = torch.full((total + 8,), -7, dtype=torch.int32, device=dev)
        assert F.lib().fst_device_compose_alignment(len(n1), P(ooff), P(ob), P(oe), P(ioff), P(ib),
                                                    P(ie), P(cons), P(rb), P(re), capacity,
                                                    None) == FF.FST_OK
        torch.cuda.synchronize()
        rb, re = rb.cpu().numpy(), re.cpu().numpy()
        assert np.array_equal(rb[:capacity], wb[:capacity])
        assert np.array_equal(re[:capacity], we[:capacity])
        assert np.all(rb[capacity:] == -7) and np.all(re[capacity:] == -7)
    # in place: the outer arrays receive the result
    assert F.lib().fst_device_compose_alignment(len(n1), P(ooff), P(ob), P(oe), P(ioff), P(ib),
                                                P(ie), P(cons), P(ob), P(oe), total,
                                                None) == FF.FST_OK
    torch.cuda.synchronize()
    assert np.array_equal(ob.cpu().numpy(), wb) and np.array_equal(oe.cpu().numpy(), we)


# ---- 6. many strings per wave: the grid-stride loops of both kernels ---------------------
# The launchers give every string a wave of its own up to 32 per CU, so the cases above never
# send a wave on to a second string.  FSTAMD_ALIGN_GRID caps both grids (1: one wave takes
# every string in turn, 3: strings i, i + 3, ...); the last test has more strings than waves
# without the cap.  What a wave carried from one string into the next (the output cursor, the
# input base, the ownership verdict) would show in every map after its first.

def label_stage_maps(stages, texts, sem):
    """(begin, end) per string from the label entry's own paths, stage by stage with the
    projection on the host, through align_model; ([], []) where a stage fails."""
    labels, offsets = to_labels(texts)
    n = len(texts)
    alive = np.ones(n, bool)
    paths = [[] for _ in range(n)]
    for s in stages:
        r = F.compose_frozen_shortest_path_batch(s, labels, offsets, 1, sem)
        off = r.offsets.astype(np.int64)
        il, ol = r.ilabels.tolist(), r.olabels.tolist()
        seqs = []
        for i in range(n):
            p = (il[off[i]:off[i + 1]], ol[off[i]:off[i + 1]])
            alive[i] &= r.status[i] == OK and all(x <= 256 for x in p[1])
            paths[i].append(p)
            seqs.append([x for x in p[1] if x] if alive[i] else [0xFFFFFFFF])
        labels = np.asarray([x for q in seqs for x in q], np.uint32)
        offsets = np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).astype(np.uint64)
    return [align(paths[i]) if alive[i] else ([], []) for i in range(n)]


def maps_of(got):
    out = []
    for i in range(len(got.status)):
        a, z = int(got.offsets[i]), int(got.offsets[i + 1])
        out.append((got.in_begin[a:z].tolist(), got.in_end[a:z].tolist()))
    return out


@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_capped_grid_one_and_two_stages(monkeypatch, grid, sem):
    monkeypatch.delenv("FSTAMD_ALIGN_GRID", raising=False)
    blob = rhs_blob(COPY_DELETE_INSERT, finals=(0.2, INF))
    texts1 = pass_edge_texts()
    want1 = expected([blob], texts1, sem)
    blobs, texts2, want2 = config4_aligned(sem)
    free1 = check_aligned([blob], texts1, sem, want1)
    free2 = check_aligned(list(blobs), texts2, sem, want2)
    monkeypatch.setenv("FSTAMD_ALIGN_GRID", grid)
    # one stage: the model, the host conversion of the label entry's paths, three shards
    one = check_aligned([blob], texts1, sem, want1)
    same_all(one, free1)
    stage = F.Fst.from_bytes(blob)
    labels, offsets = to_labels(texts1)
    same_all(one, F.batch_result_to_aligned_text(
        F.compose_frozen_shortest_path_batch(stage, labels, offsets, 1, sem)))
    same_all(one, check_aligned([blob], texts1, sem, want1, devices=[0], shards=3))
    # two stages: the compose kernel strides too
    two = check_aligned(list(blobs), texts2, sem, want2)
    same_all(two, free2)
    same_all(two, check_aligned(list(blobs), texts2, sem, want2, devices=[0], shards=3))
    stages = [F.Fst.from_bytes(b) for b in blobs]
    assert maps_of(two) == label_stage_maps(stages, texts2, sem)


@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_more_strings_than_waves(monkeypatch, sem):
    monkeypatch.delenv("FSTAMD_ALIGN_GRID", raising=False)
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 32
    n = waves + 333          # the first 333 waves take a second string
    rng = np.random.default_rng(21)
    # one stage: short strings of copies, deletions and insertions
    texts = [bytes(rng.choice(list(b"adxi"), int(k)).tolist()) for k in rng.integers(0, 7, n)]
    texts[waves] = b"d" * 62 + b"i" + b"d" * 70      # a second string that spans three passes
    stage = F.Fst.from_bytes(rhs_blob(COPY_DELETE_INSERT, finals=(0.2, INF)))
    got = F.normalize_text_aligned_batch([stage], texts, sem)
    invariants(got, texts)
    same_text(got, F.normalize_text_batch([stage], texts, sem))
    labels, offsets = to_labels(texts)
    same_all(got, F.batch_result_to_aligned_text(
        F.compose_frozen_shortest_path_batch(stage, labels, offsets, 1, sem)))
    assert maps_of(got) == label_stage_maps([stage], texts, sem)
    assert got.spans(waves) == [(62, 63, 0, 1), (63, 63, 1, 2)]
    same_all(got, F.normalize_text_aligned_batch([stage], texts, sem, devices=[0], shards=3))
    # two stages: letters and digits through tagger -> verbalizer, "#" fails stage 1
    blobs, _, _ = config4_aligned(sem)
    stages = [F.Fst.from_bytes(b) for b in blobs]
    texts = [bytes(rng.choice(list(b"ab 07#"), int(k), p=[.25, .25, .1, .17, .17, .06]).tolist())
             for k in rng.integers(0, 6, n)]
    got = F.normalize_text_aligned_batch(stages, texts, sem)
    invariants(got, texts)
    same_text(got, F.normalize_text_batch(stages, texts, sem))
    maps = label_stage_maps(stages, texts, sem)
    assert maps_of(got) == maps
    assert sum(1 for m in maps[waves:] if m[0]) > 100 and (got.status[waves:] != OK).sum() > 10
    same_all(got, F.normalize_text_aligned_batch(stages, texts, sem, devices=[0], shards=3))
