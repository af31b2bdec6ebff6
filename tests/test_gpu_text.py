"""GPU tests of the text entries: fst_normalize_text_batch (bytes in, bytes out), the device
pieces fst_device_compile_text / fst_device_emit_text, and their agreement with the oracle.

Every case compares the text entry with values derived from the CPU oracle (O.batch_run /
oracle_pipeline, then the projection and the left fold in Python, test_text_api.python_text)
and with the host conversion of the label entry's result on the same inputs; the hand-built
device batches are compared with the same Python projection."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import libfst_amd as F
from libfst_amd import fst as FF
from libfst_amd import synthetic as SY
import oracle_ffi as O
from test_gpu_configs import oracle_fst, oracle_pipeline
from test_gpu_parity import EAGER, LAZY, bits
from test_text_api import python_text

pytestmark = pytest.mark.gpu

OK, EMPTY, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED
INF = math.inf


def to_labels(texts):
    data, offsets = FF.text_csr(texts)
    return data.astype(np.uint32) + 1, offsets


def expected(blobs, texts, sem):
    """(texts, status, total weights) from the oracle's paths."""
    labels, offsets = to_labels(texts)
    ref, exp = oracle_pipeline(blobs, labels, offsets, sem)
    r = F.BatchResult(status=exp, offsets=ref.offsets, ilabels=ref.ilabels, olabels=ref.olabels,
                      weights=ref.weights, finals=ref.finals)
    return python_text(r)


def same(got, want):
    texts, status, tw = want
    assert np.array_equal(got.status, status), np.nonzero(got.status != status)[0][:10]
    assert got.texts() == texts
    assert np.array_equal(bits(got.total_weight), bits(tw))
    assert int(got.offsets[0]) == 0 and int(got.offsets[-1]) == len(got.text)
    assert got.text.tobytes() == b"".join(texts)


def check_text(blobs, texts, sem, want=None, **kw):
    stages = [F.Fst.from_bytes(b) for b in blobs]
    got = F.normalize_text_batch(stages, texts, sem, **kw)
    want = want or expected(blobs, texts, sem)
    same(got, want)
    labels, offsets = to_labels(texts)
    same(F.batch_result_to_text(F.pipeline_batch(stages, labels, offsets, 1, sem)), want)
    return got, want


def rhs_blob(arcs, finals=(0.0,)):
    """A frozen rhs from (src, il, ol, w, next) arcs."""
    f = O.Fst()
    for fw in finals:
        f.add_state(fw)
    f.start = 0
    for a in arcs:
        f.add_arc(*a)
    return O.freeze(f)


def lab(ch):
    return ord(ch) + 1


# ---- 1. two stages, both semantics ------------------------------------------------------

def shifted(spec, dw):
    ns, start, finals, arcs = spec
    return (ns, start, [f + dw if f != INF else f for f in finals],
            [[(il, ol, w + dw, nx) for (il, ol, w, nx) in al] for al in arcs])


@functools.lru_cache(maxsize=None)
def config4(sem, dw=0.0):
    blobs = (O.freeze(oracle_fst(shifted(SY.tagger(), dw))),
             O.freeze(oracle_fst(shifted(SY.verbalizer(), dw))))
    rng = np.random.default_rng(4)
    texts = [t.encode() for t in SY.utterances(rng, 300) + ["", "a", "7", "##", "call 911"]]
    return blobs, texts, expected(blobs, texts, sem)


@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_tagger_verbalizer_text(sem):
    blobs, texts, want = config4(sem)
    got, _ = check_text(blobs, texts, sem, want)
    assert (want[1] == OK).sum() > 0.9 * len(texts) - 5
    assert got.texts()[texts.index(b"7")] == b"seven"
    i = texts.index(b"##")   # the tagger has no arc for '#': stage 1's status is reported
    assert got.status[i] == EMPTY and got.total_weight[i] == INF


# ---- 2. one stage, the running base across 64-arc passes --------------------------------

# 'a' and 'x' are copied, 'd' is deleted (an epsilon output at that path position); the
# weights are no dyadic rationals, so the fold's order shows in the total
COPY_DELETE = [(0, lab("a"), lab("a"), 0.1, 0), (0, lab("x"), lab("x"), 0.7, 0),
               (0, lab("d"), 0, 0.3, 0)]


def test_one_stage_pass_boundaries():
    blob = rhs_blob(COPY_DELETE, finals=(0.2,))
    rng = np.random.default_rng(2)
    texts = []
    for L in (0, 1, 63, 64, 65, 128, 129, 200):
        texts.append(bytes(rng.choice(list(b"adx"), L).tolist()))
        texts.append(b"a" * L)
    texts += [b"d" * 70 + b"xa" * 3,          # the first output byte falls in the second pass
              b"d" * 130 + b"a",               # ... in the third
              b"d" * 130, b"d" * 64, b"d",     # every output epsilon
              b"a" * 63 + b"d" + b"x" * 64 + b"d" * 64 + b"a"]
    for sem in (LAZY, EAGER):
        got, want = check_text([blob], texts, sem)
        assert want[0][-6] == b"xaxaxa" and want[0][-4] == b"" and all(s == OK for s in want[1])


# ---- 3. neighbours share dwords ----------------------------------------------------------

def test_neighbouring_strings_keep_their_bytes():
    blob = rhs_blob(COPY_DELETE)
    texts = []
    for i in range(257):
        s = [ord("a") if i % 2 else ord("x")] * (i % 8) + [ord("d")] * (i * 3 % 5)
        texts.append(bytes(np.random.default_rng(i).permutation(s).tolist()))
    got, want = check_text([blob], texts, LAZY)
    assert [len(t) for t in got.texts()] == [i % 8 for i in range(257)]
    assert got.text.tobytes() == b"".join(want[0])


# ---- 4. widen ----------------------------------------------------------------------------

GUARD = 0x5A5A5A5A


def widen_on_device(data, offsets, shift):
    """fst_device_compile_text on `data` placed `shift` bytes into a device buffer; returns the
    whole label buffer (guards before and after the range the call may write)."""
    dev = torch.device("cuda", 0)
    buf = torch.zeros(len(data) + 8, dtype=torch.uint8, device=dev)
    txt = buf[shift:shift + len(data)]
    txt.copy_(torch.as_tensor(data))
    off = torch.as_tensor(offsets.astype(np.int64), device=dev)
    pad = 64
    labels = torch.full((len(data) + 2 * pad,), GUARD, dtype=torch.int32, device=dev)
    rc = F.lib().fst_device_compile_text(C.c_void_p(txt.data_ptr()), C.c_void_p(off.data_ptr()),
                                         len(offsets) - 1,
                                         C.c_void_p(labels.data_ptr() + 4 * pad), None)
    assert rc == FF.FST_OK
    torch.cuda.synchronize()
    return labels.cpu().numpy().view(np.uint32), pad


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_widen_every_alignment(shift):
    rng = np.random.default_rng(40 + shift)
    # (the three 1-byte strings at the end: dropping 0..3 of them ends the range at every
    # residue mod 4, so the bytes after the last whole dword number 0, 1, 2 and 3)
    lens = np.concatenate([np.arange(10), rng.integers(0, 10, 38), [1, 1, 1]])
    total = int(lens.sum())
    if total % 4 == 0:
        lens[10] += 1
        total += 1
    data = rng.integers(0, 256, total).astype(np.uint8)
    data[:4] = [0, 255, 0, 255]
    data[-2:] = [255, 0]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert {int(o) % 4 for o in offsets} == {0, 1, 2, 3} and total % 4 != 0
    tails = set()
    for first in (0, 3):     # the range may also start inside the buffer
        for drop in (0, 1, 2, 3):
            off = offsets[first:len(offsets) - drop]
            lo, hi = int(off[0]), int(off[-1])
            head = min((4 - (shift + lo) % 4) % 4, hi - lo)   # (the buffer itself is aligned)
            tails.add((hi - lo - head) % 4)
            out, pad = widen_on_device(data, off, shift)
            assert np.array_equal(out[pad + lo:pad + hi], data[lo:hi].astype(np.uint32) + 1)
            assert np.all(out[:pad + lo] == GUARD) and np.all(out[pad + hi:] == GUARD)
    assert tails == {0, 1, 2, 3}


def test_widen_more_dwords_than_threads():
    rng = np.random.default_rng(44)
    total = (3 << 20) + 5       # the grid strides over its dwords more than once
    data = rng.integers(0, 256, total).astype(np.uint8)
    offsets = np.asarray([0, 5, 5, total], np.uint64)
    out, pad = widen_on_device(data, offsets, 1)     # 3 bytes before the first dword, 2 after
    assert np.array_equal(out[pad:pad + total], data.astype(np.uint32) + 1)
    assert np.all(out[:pad] == GUARD) and np.all(out[pad + total:] == GUARD)


# ---- 5. non-byte labels and failures -----------------------------------------------------

def test_non_byte_labels_and_failures():
    odd = rhs_blob([(0, lab("a"), lab("a"), 0.5, 0), (0, lab("b"), 257, 0.5, 0),
                    (0, lab("c"), 0xFFFFFFFF, 0.5, 0)])
    copy = rhs_blob([(0, lab(c), lab(c), 0.25, 0) for c in "abc"])
    texts = [b"aa", b"ab", b"ca", b"ae", b"", b"aaa"]
    for sem in (LAZY, EAGER):
        # the last stage emits the labels: UNSUPPORTED, no bytes, +inf; "ae" has no path
        got, _ = check_text([odd], texts, sem)
        assert list(got.status) == [OK, UNSUPPORTED, UNSUPPORTED, EMPTY, OK, OK]
        assert got.texts() == [b"aa", b"", b"", b"", b"", b"aaa"]
        assert np.all(np.isinf(got.total_weight[1:4]))
        got, _ = check_text([copy, odd], texts, sem)
        assert list(got.status) == [OK, UNSUPPORTED, UNSUPPORTED, EMPTY, OK, OK]
        # stage 1 fails: its status is the string's, whatever stage 2 makes of the dead input
        got, _ = check_text([odd, copy], texts, sem)
        assert list(got.status) == [OK, UNSUPPORTED, UNSUPPORTED, EMPTY, OK, OK]
        assert got.texts() == [b"aa", b"", b"", b"", b"", b"aaa"]


# ---- 6. the device emission on its own, and its capacity check ---------------------------

def device_emit(paths, capacity, guard=16):
    """fst_device_emit_text on a hand-built stage: `paths` = [(status, olabels, weights, final)],
    laid out in the arena back to front with gaps.  Returns (text buffer with `guard` bytes
    past the capacity, offsets, status, total weights, total bytes)."""
    dev = torch.device("cuda", 0)
    n = len(paths)
    poff, pos = [0] * n, 3
    for i in reversed(range(n)):
        poff[i] = pos
        pos += len(paths[i][1]) + (i % 3)
    cap = pos + 5
    ol = np.full(cap, 300, np.uint32)      # the gaps hold non-byte labels: never read
    w = np.full(cap, np.nan)
    for i, p in enumerate(paths):
        ol[poff[i]:poff[i] + len(p[1])] = p[1]
        w[poff[i]:poff[i] + len(p[1])] = p[2]
    t = lambda a, dt: torch.as_tensor(np.asarray(a).astype(dt), device=dev)
    status = t([p[0] for p in paths], np.int32)
    plen = t([len(p[1]) for p in paths], np.int32)
    poff_d = t(poff, np.int64)
    fin = t([p[3] for p in paths], np.float64)
    ol_d, w_d = t(ol.view(np.int32), np.int32), t(w, np.float64)
    il_d = torch.zeros(cap, dtype=torch.int32, device=dev)
    cur = torch.zeros(1, dtype=torch.int64, device=dev)
    desc = FF.FstDeviceBatch(status.data_ptr(), plen.data_ptr(), poff_d.data_ptr(), fin.data_ptr(),
                             il_d.data_ptr(), ol_d.data_ptr(), w_d.data_ptr(), cap,
                             cur.data_ptr(), 0)
    text = torch.full((capacity + guard,), 0xEE, dtype=torch.uint8, device=dev)
    toff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    tw = torch.zeros(n, dtype=torch.float64, device=dev)
    total = FF._u64(0)
    rc = F.lib().fst_device_emit_text(C.byref(desc), n, C.c_void_p(text.data_ptr()), capacity,
                                      C.c_void_p(toff.data_ptr()), C.c_void_p(st.data_ptr()),
                                      C.c_void_p(tw.data_ptr()), C.byref(total), None)
    assert rc == FF.FST_OK
    torch.cuda.synchronize()
    return (text.cpu().numpy(), toff.cpu().numpy().astype(np.uint64), st.cpu().numpy(),
            tw.cpu().numpy(), int(total.value))


def hand_paths():
    rng = np.random.default_rng(6)
    paths = []
    for i, L in enumerate([0, 1, 5, 63, 64, 65, 127, 128, 129, 200, 7, 3, 2, 1, 0, 70]):
        ol = rng.integers(0, 257, L)
        ol[rng.random(L) < 0.4] = 0
        paths.append((OK, ol.tolist(), rng.random(L).tolist(), float(rng.random())))
    paths[10] = (OK, [5, 257, 6, 0, 1, 2, 3], [0.1] * 7, 0.0)        # a non-byte label
    paths[11] = (EMPTY, [], [], INF)
    paths[12] = (F.FST_PATH_CYCLE, [9, 9], [0.1, 0.1], 0.0)          # a failed string's arcs
    paths[15] = (OK, [0] * 66 + [256, 1, 0, 98], [0.1] * 70, 0.7)    # bytes from pass 2 on
    return paths


def test_device_emit_and_capacity():
    paths = hand_paths()
    r = F.BatchResult(status=np.asarray([p[0] for p in paths], np.int32),
                      offsets=np.concatenate([[0], np.cumsum([len(p[1]) for p in paths])]).astype(np.uint64),
                      ilabels=np.zeros(0, np.uint32),
                      olabels=np.asarray([x for p in paths for x in p[1]], np.uint32),
                      weights=np.asarray([x for p in paths for x in p[2]], np.float64),
                      finals=np.asarray([p[3] for p in paths], np.float64))
    texts, status, tw = python_text(r)
    whole = np.frombuffer(b"".join(texts), np.uint8)
    need = len(whole)
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    assert status[10] == UNSUPPORTED and texts[15] == b"\xff\x00a"
    for capacity in (need, need - 1, need - 37, 3, 0):
        text, toff, st, w, total = device_emit(paths, capacity)
        assert total == need                       # the needed total, whatever the capacity
        assert np.array_equal(text[:capacity], whole[:capacity])
        assert np.all(text[capacity:] == 0xEE)     # nothing at or past the capacity
        assert np.array_equal(toff, off) and np.array_equal(st, status)
        assert np.array_equal(bits(w), bits(tw))


# ---- 7. shards ---------------------------------------------------------------------------

def test_shards_give_identical_bytes():
    blobs, texts, want = config4(LAZY)
    stages = [F.Fst.from_bytes(b) for b in blobs]
    one = F.normalize_text_batch(stages, texts, LAZY, devices=[0], shards=1)
    three = F.normalize_text_batch(stages, texts, LAZY, devices=[0], shards=3)
    same(one, want)
    same(three, want)
    assert np.array_equal(one.offsets, three.offsets)
    assert one.text.tobytes() == three.text.tobytes()


# ---- 8. weights that are no dyadic rationals ---------------------------------------------

@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_total_weight_fold_with_non_dyadic_weights(sem):
    blobs, texts, want = config4(sem, 0.1)
    check_text(blobs, texts, sem, want)
    ok = want[1] == OK
    assert ok.sum() > 0.9 * len(texts) - 5
    # the case is not vacuous: some total differs from its pairwise (tree) sum
    labels, offsets = to_labels(texts)
    ref, _ = oracle_pipeline(blobs, labels, offsets, sem)
    tree = lambda x: 0.0 if len(x) == 0 else float(x[0]) if len(x) == 1 else \
        tree(x[:len(x) // 2]) + tree(x[len(x) // 2:])
    differs = sum(tree(ref.weights[int(ref.offsets[i]):int(ref.offsets[i + 1])]) + ref.finals[i]
                  != want[2][i] for i in np.nonzero(ok)[0])
    assert differs > 0


# ---- 9. hygiene --------------------------------------------------------------------------

def test_empty_batch_pool_reuse_and_idle_coalescer():
    blobs, texts, want = config4(LAZY)
    stages = [F.Fst.from_bytes(b) for b in blobs]
    none = F.normalize_text_batch(stages, [], LAZY)
    assert len(none.status) == 0 and list(none.offsets) == [0] and none.texts() == []
    a = F.normalize_text_batch(stages, texts, LAZY)
    first = (a.status.copy(), a.offsets.copy(), a.text.copy(), a.total_weight.copy())
    del a                                           # its pinned blocks go back to the pool
    b = F.normalize_text_batch(stages, texts, LAZY)
    for x, y in zip(first, (b.status, b.offsets, b.text, b.total_weight)):
        assert x.tobytes() == y.tobytes()
    same(b, want)
    # a (uint8 array, offsets) pair is the same input
    c = F.normalize_text_batch(stages, FF.text_csr(texts), LAZY)
    assert c.text.tobytes() == b.text.tobytes()
    assert F.coalescer_state(0) == (0, 0)
