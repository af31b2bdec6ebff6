"""GPU tests of the streamed route of fst_normalize_text_batch (c_api.cpp run_streamed in text
mode): one stage whose rhs has no input epsilon and starts with a pull tier.  The bytes go up
in parts under the pull kernels, which read them as labels (byte + 1) and write every
finished string's text into its fixed slot of the pinned result from the chase epilogue
(kernels/device_common.hpp emit_text_paths); strings the pull tier hands on are finished by
the later tiers and emitted by text_fixup_kernel; the host closes the short slots up.

Every case takes its expected values from the CPU oracle (test_gpu_text.expected: the oracle's
paths, then the projection and the left fold in Python) and compares three producers of this
build with them and with each other, byte for byte and bit for bit: the streamed text route,
the text entry with FSTAMD_STREAM=0 (the sharded route) and fst_batch_result_to_text of the
label entry's result.

The rhs is a ring of 48 states, every weight a non-dyadic decimal (0.1, 0.3, 0.7, final 0.2):
  'a' : two arcs, olabel 'a' weight 0.1 to s + 1 and olabel 'A' weight 0.3 to s + 2 (a choice:
        what follows may only be accepted from one of the two);
  'd' : olabel 0 (an output epsilon), 0.3, to s + 1;
  'x' : olabel 'x', 0.7, to s + 1;
  'z' : olabel 256 (the byte 0xFF, legal), 0.1, to s + 1 -- even states only;
  'n' : olabel 257 (no byte), 0.1, to s + 1 -- states 3, 17, 31, 45 only.
'd' moves one state at a time, so b"ddd" + b"n" must take a 257 arc and b"d" + b"z" dies."""
import functools

import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
from test_gpu_parity import EAGER, LAZY, bits, expected_status
from test_gpu_text import lab, rhs_blob, same, to_labels
from test_text_api import python_text
import test_gpu_text as TG

pytestmark = pytest.mark.gpu

OK, EMPTY, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED
S = 48


@functools.lru_cache(maxsize=None)
def ring_blob():
    f = O.Fst()
    for _ in range(S):
        f.add_state(0.2)
    f.start = 0
    for s in range(S):
        n1, n2 = (s + 1) % S, (s + 2) % S
        f.add_arc(s, lab("a"), lab("a"), 0.1, n1)
        f.add_arc(s, lab("a"), lab("A"), 0.3, n2)
        f.add_arc(s, lab("d"), 0, 0.3, n1)
        f.add_arc(s, lab("x"), lab("x"), 0.7, n1)
        if s % 2 == 0:
            f.add_arc(s, lab("z"), 256, 0.1, n1)
        elif s % 14 == 3:
            f.add_arc(s, lab("n"), 257, 0.1, n1)
    return O.freeze(f)


@functools.lru_cache(maxsize=None)
def metric_blob():
    return O.freeze(O.gen("ambiguous", 4096, 12))


@functools.lru_cache(maxsize=None)
def stage(which):
    if which == "ring":
        return F.Fst.from_bytes(ring_blob())
    return F.Fst.bench_transducer(F.BENCH_AMBIGUOUS, 4096, 12)


def blob_of(which):
    return ring_blob() if which == "ring" else metric_blob()


def expected(blobs, texts, sem):
    """test_gpu_text.expected for one stage, the oracle on 8 threads: (texts, status, total
    weights) from the oracle's paths."""
    (blob,) = blobs
    labels, offsets = to_labels(texts)
    ref = O.batch_run(blob, labels, offsets, 0 if sem == LAZY else 1, 1, 8)
    r = F.BatchResult(status=expected_status(ref), offsets=ref.offsets, ilabels=ref.ilabels,
                      olabels=ref.olabels, weights=ref.weights, finals=ref.finals)
    return python_text(r)


def identical(a, b):
    assert np.array_equal(a.status, b.status), np.nonzero(a.status != b.status)[0][:10]
    assert np.array_equal(a.offsets, b.offsets)
    assert a.text.tobytes() == b.text.tobytes()
    assert np.array_equal(bits(a.total_weight), bits(b.total_weight))


def shard_log(err):
    return [ln.split() for ln in err.splitlines() if ln.startswith("[libfst_amd shard]")]


def three_producers(which, texts, sem, monkeypatch, **kw):
    """(streamed text result, FSTAMD_STREAM=0 text result, converted label result)."""
    st = stage(which)
    got = F.normalize_text_batch([st], texts, sem, **kw)
    with monkeypatch.context() as m:
        m.setenv("FSTAMD_STREAM", "0")
        plain = F.normalize_text_batch([st], texts, sem, **kw)
    labels, offsets = to_labels(texts)
    conv = F.batch_result_to_text(F.compose_frozen_shortest_path_batch(st, labels, offsets, 1, sem))
    identical(got, plain)
    identical(got, conv)
    return got, plain, conv


def check(which, texts, sem, monkeypatch, want=None, **kw):
    want = want or expected([blob_of(which)], texts, sem)
    got, plain, conv = three_producers(which, texts, sem, monkeypatch, **kw)
    for r in (got, plain, conv):
        same(r, want)
    return got, want


# ---- 1. the route ------------------------------------------------------------------------

def route_of(stages, texts, sem, capfd, monkeypatch):
    capfd.readouterr()
    with monkeypatch.context() as m:
        m.setenv("FSTAMD_SHARD_LOG", "1")
        got = F.normalize_text_batch(stages, texts, sem)
    plan = shard_log(capfd.readouterr().err)
    assert len(plan) == 1, plan
    return plan[0][-1], got


@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_route(sem, capfd, monkeypatch):
    texts = [b"aax", b"", b"ddz", b"adxa" * 9]
    # the ring and the metric rhs: one stage, no input epsilon, a pull tier first
    route, got = route_of([stage("ring")], texts, sem, capfd, monkeypatch)
    assert route == "streamed-text"
    want = expected([ring_blob()], texts, sem)
    same(got, want)
    check("ring", texts, sem, monkeypatch, want)      # ... and the other two producers
    mtexts = [bytes([0] * 64), bytes([0, 1] * 20), b"", bytes([2, 0])]
    route, got = route_of([stage("metric")], mtexts, sem, capfd, monkeypatch)
    assert route == "streamed-text"
    mwant = expected([metric_blob()], mtexts, sem)
    same(got, mwant)
    check("metric", mtexts, sem, monkeypatch, mwant)
    # FSTAMD_STREAM=0, two stages, an rhs with an input epsilon: the sharded route
    with monkeypatch.context() as m:
        m.setenv("FSTAMD_STREAM", "0")
        route, got = route_of([stage("ring")], texts, sem, capfd, monkeypatch)
    assert route == "sharded"
    same(got, want)
    blobs, ctexts, cwant = TG.config4(sem)
    route, got = route_of([F.Fst.from_bytes(b) for b in blobs], ctexts, sem, capfd, monkeypatch)
    assert route == "sharded"
    same(got, cwant)
    TG.check_text(blobs, ctexts, sem, cwant)          # (the label entry's converted result too)
    eps = rhs_blob([(0, 0, lab("e"), 0.1, 1), (0, lab("a"), lab("a"), 0.1, 0),
                    (1, lab("a"), lab("b"), 0.3, 1)], finals=(0.7, 0.2))
    etexts = [b"aaa", b"", b"ab"]
    route, got = route_of([F.Fst.from_bytes(eps)], etexts, sem, capfd, monkeypatch)
    assert route == "sharded"
    ewant = expected([eps], etexts, sem)
    same(got, ewant)
    TG.check_text([eps], etexts, sem, ewant)


# ---- 2. emission edges, one part ---------------------------------------------------------

def edge_texts():
    rng = np.random.default_rng(2)
    texts = []
    for L in (0, 1, 63, 64, 65, 128, 129, 200):
        texts.append(bytes(rng.choice(list(b"adx"), L).tolist()))
        texts.append(b"a" * L)
    texts += [b"d", b"d" * 64, b"d" * 130,     # every output an epsilon: 1, 64, 130 arcs
              b"d" * 70 + b"xa" * 3,           # the first output byte falls in the second pass
              b"d" * 130 + b"a",               # ... in the third
              b"ddz" + b"a" * 5 + b"z",        # the byte 0xFF (and a choice: z needs an even state)
              b"a" * 63 + b"d" + b"x" * 64 + b"d" * 64 + b"a"]
    for i in range(257):                       # neighbours share dwords: 0..7 bytes each
        s = [ord("a") if i % 2 else ord("x")] * (i % 8) + [ord("d")] * (i * 3 % 5)
        texts.append(bytes(np.random.default_rng(i).permutation(s).tolist()))
    return texts


@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_emission_edges(sem, monkeypatch):
    texts = edge_texts()
    got, want = check("ring", texts, sem, monkeypatch)
    assert all(s == OK for s in want[1])
    assert want[0][19] == b"xaxaxa" and want[0][20] == b"a" and want[0][16:19] == [b"", b"", b""]
    assert b"\xff" in want[0][21]
    assert [len(t) for t in got.texts()[-257:]] == [i % 8 for i in range(257)]
    assert got.text.tobytes() == b"".join(want[0])
    assert int(got.offsets[0]) == 0 and int(got.offsets[-1]) == len(got.text)
    # full and partial chase batches (16 jobs a chase)
    for n in (1, 15, 16, 17, 33):
        sub = texts[3:3 + n]
        check("ring", sub, sem, monkeypatch, (want[0][3:3 + n], want[1][3:3 + n], want[2][3:3 + n]))


# ---- 3. several strings per wave ---------------------------------------------------------

@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_many_strings_per_wave(sem, monkeypatch):
    # three waves take all 300 strings: every emission but a wave's last runs with a full
    # chase batch and later strings' jobs pending behind it
    monkeypatch.setenv("FSTAMD_P_GRID", "3")
    monkeypatch.setenv("FSTAMD_LP_GRID", "3")
    rng = np.random.default_rng(33)
    texts = [bytes(rng.choice(list(b"aaaddxxz"), int(rng.integers(0, 90))).tolist())
             for _ in range(300)]
    got, want = check("ring", texts, sem, monkeypatch)
    assert (want[1] == OK).sum() > 100 and (want[1] == EMPTY).sum() > 5


# ---- 4. statuses -------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_statuses_and_compaction(sem, monkeypatch):
    texts = [b"aa", b"dddn", b"ax", b"aqa", b"xdx", b"dz", b"", b"dddnaa", b"ddz", b"n", b"xx"]
    got, want = check("ring", texts, sem, monkeypatch)
    assert list(got.status) == [OK, UNSUPPORTED, OK, EMPTY, OK, EMPTY, OK, UNSUPPORTED, OK, EMPTY, OK]
    assert got.texts() == [b"aa", b"", b"ax", b"", b"xx", b"", b"", b"", b"\xff", b"", b"xx"]
    bad = got.status != OK
    assert np.all(np.isinf(got.total_weight[bad])) and np.all(np.isfinite(got.total_weight[~bad]))
    # the gaps are closed: the offsets are the prefix sum of the OK strings' byte counts
    assert list(got.offsets) == [0, 2, 2, 4, 4, 6, 6, 6, 6, 7, 7, 9]


# ---- 5. fold order -----------------------------------------------------------------------

@pytest.mark.parametrize("sem", [LAZY, EAGER])
def test_fold_order(sem, monkeypatch):
    texts = [b"a" * 10 + b"x", b"x" + b"a" * 10]
    got, want = check("ring", texts, sem, monkeypatch)
    fold = 0.0
    for w in [0.1] * 10 + [0.7]:
        fold += w
    assert bits(got.total_weight[0]) == bits(np.float64(fold + 0.2))
    # the case is not vacuous: the same weights in another order round differently
    assert bits(got.total_weight[0]) != bits(got.total_weight[1])
    assert np.array_equal(bits(got.total_weight), bits(want[2]))


# ---- 6. several parts --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def big_batch(which):
    rng = np.random.default_rng(606 if which == "ring" else 607)
    num = 40000 if which == "ring" else 42000   # (the metric batch has few long strings)
    lens = rng.integers(80, 130, num)
    texts = []
    for i, L in enumerate(lens):
        if which == "ring":
            q = rng.choice(list(b"aaaaddxxxz"), L).astype(np.uint8)
        else:
            q = np.where(rng.random(L) < 0.9, 0, 1).astype(np.uint8)
        kind = i % 97
        if kind == 5:
            q = q[:0]                                        # the empty string
        elif kind == 11:
            q[int(rng.integers(0, L))] = ord("q") if which == "ring" else 2   # no rhs arc
        elif kind == 17 and which == "ring":                 # long: 900 bytes
            q = rng.choice(list(b"adx"), 900).astype(np.uint8)
        elif kind == 17 and (i // 97) % 128 == 0:            # (4 of them: the lazy later tiers
            q = np.zeros(900, np.uint8)                      # take ~0.3 s for each)
        elif kind == 23 and which == "ring":
            q[:4] = list(b"dddn")                            # must take an olabel-257 arc
        texts.append(q.tobytes())
    assert sum(len(t) for t in texts) >= (1 << 22) and num >= (1 << 15)
    return texts


@functools.lru_cache(maxsize=None)
def big_sample(which, sem):
    texts = big_batch(which)
    num = len(texts)
    rng = np.random.default_rng(1 + sem)
    special = [i for i in range(num) if i % 97 in (5, 11, 17, 23)]
    # every 14th special string (they alternate between two kinds), some of the others and
    # four of the 900-byte ones (all there are on the metric rhs)
    picked = special[::14] + special[1::42]
    picked += [i for i in special if len(texts[i]) == 900][:4]
    idx = np.unique(np.concatenate([rng.choice(num, 150, replace=False), np.asarray(picked),
                                    [0, num - 1]])).astype(np.int64)
    return idx, expected([blob_of(which)], [texts[i] for i in idx], sem)


@pytest.mark.parametrize("sem", [EAGER, LAZY])
@pytest.mark.parametrize("cuts", ["", "8,45,230"])
@pytest.mark.parametrize("which", ["ring", "metric"])
def test_several_parts(which, cuts, sem, monkeypatch, capfd):
    texts = big_batch(which)
    if cuts:
        monkeypatch.setenv("FSTAMD_STREAM_CUTS", cuts)
    monkeypatch.setenv("FSTAMD_SHARD_LOG", "1")
    capfd.readouterr()
    got, plain, conv = three_producers(which, texts, sem, monkeypatch)
    err = capfd.readouterr().err
    assert [p[-1] for p in shard_log(err)] == ["streamed-text", "sharded", "streamed"], err[-1500:]
    stream = [ln.split() for ln in err.splitlines() if ln.startswith("[libfst_amd stream]")]
    assert int(stream[0][7]) == (4 if cuts else 3), stream      # the parts of the text call
    if which == "metric":   # the 900-byte strings outgrow the pull tier's back slab there
        assert int(stream[0][-1]) >= 4, stream
    idx, want = big_sample(which, sem)
    wtexts, wstatus, wtw = want
    all_texts = got.texts()
    assert np.array_equal(got.status[idx], wstatus)
    assert [all_texts[i] for i in idx] == wtexts
    assert np.array_equal(bits(got.total_weight[idx]), bits(wtw))
    kinds = {int(s) for s in wstatus}
    assert kinds >= ({OK, EMPTY, UNSUPPORTED} if which == "ring" else {OK, EMPTY})
    assert int(got.offsets[0]) == 0 and int(got.offsets[-1]) == len(got.text)


# ---- 6b. strings the pull tier hands on, on the ring --------------------------------------

def test_handed_on_strings_with_a_non_byte_label(monkeypatch, capfd):
    # the lazy pull hands on every string of more than 4095 bytes (kLpMaxLen): the later
    # tiers finish them in the arena's slots and text_fixup_kernel emits them -- one with a
    # forced olabel-257 arc (its byte count comes back as "not bytes": UNSUPPORTED, no bytes),
    # one whose only bytes come after 4100 output epsilons, one plain, one with no path.
    # (Eager tier P hands nothing on for this rhs at any length a test could afford; the
    # metric rhs's 900-byte strings in test_several_parts are its handed-on case.)
    long = 4100
    texts = [b"ax", b"dddn" + b"a" * long, b"d" * long + b"xa", b"", b"a" * long,
             b"a" * long + b"q", b"dddnx", b"x" * 9]
    monkeypatch.setenv("FSTAMD_SHARD_LOG", "1")
    capfd.readouterr()
    got, want = check("ring", texts, LAZY, monkeypatch)
    err = capfd.readouterr().err
    stream = [ln.split() for ln in err.splitlines() if ln.startswith("[libfst_amd stream]")]
    assert int(stream[0][-1]) == 4, stream     # the four long ones, nothing else
    assert list(got.status) == [OK, UNSUPPORTED, OK, OK, OK, EMPTY, UNSUPPORTED, OK]
    assert got.texts() == [b"ax", b"", b"xa", b"", b"a" * long, b"", b"", b"x" * 9]
    assert np.isinf(got.total_weight[1]) and np.isfinite(got.total_weight[2])


# ---- 7. shards on one GPU ----------------------------------------------------------------

@pytest.mark.parametrize("sem", [EAGER, LAZY])
def test_shards_on_one_gpu(sem, monkeypatch, capfd):
    rng = np.random.default_rng(70 + sem)
    texts = [bytes(rng.choice(list(b"aaaddxxz"), int(rng.integers(0, 70))).tolist())
             for _ in range(1500)]
    texts[7] = b"dddn" + texts[7]
    texts[700] = b"q"
    one, want = check("ring", texts, sem, monkeypatch)
    for shards in (2, 3):
        capfd.readouterr()
        with monkeypatch.context() as m:
            m.setenv("FSTAMD_SHARD_LOG", "1")
            many = F.normalize_text_batch([stage("ring")], texts, sem, devices=[0], shards=shards)
        plan = shard_log(capfd.readouterr().err)
        assert len(plan) == shards and all(p[-1] == "streamed-text" for p in plan), plan
        spans = [tuple(int(x) for x in p[6].split("..")) for p in plan]
        assert spans[0][0] == 0 and spans[-1][1] == len(texts)
        assert all(spans[j][1] == spans[j + 1][0] for j in range(shards - 1))
        identical(many, one)
        same(many, want)


# ---- 8. error path -----------------------------------------------------------------------

@pytest.mark.parametrize("sem", [EAGER, LAZY])
def test_failure_drains_its_streams(sem, monkeypatch):
    # FSTAMD_FAULT_INJECT=stream_after_pull: the call fails once the parts' kernels and the
    # downloads were queued; its buffers and result pages go back to the pools only after
    # every stream has drained, so the next calls (they reuse those blocks) are right
    rng = np.random.default_rng(80 + sem)
    texts = [bytes(rng.choice(list(b"aaaddxxz"), int(rng.integers(0, 70))).tolist())
             for _ in range(1200)]
    want = expected([ring_blob()], texts, sem)
    monkeypatch.setenv("FSTAMD_FAULT_INJECT", "stream_after_pull")
    with pytest.raises(RuntimeError):
        F.normalize_text_batch([stage("ring")], texts, sem)
    monkeypatch.delenv("FSTAMD_FAULT_INJECT")
    for _ in range(2):
        check("ring", texts, sem, monkeypatch, want)
    assert F.coalescer_state(0) == (0, 0)


# ---- 9. the label entry's streamed route is untouched ------------------------------------

@pytest.mark.parametrize("sem", [EAGER, LAZY])
def test_label_entry_untouched(sem, monkeypatch, capfd):
    rhs = stage("metric")
    rng = np.random.default_rng(90 + sem)
    num = 1 << 16
    lab2d = np.where(rng.random((num, 64)) < 0.9, 1, 2).astype(np.uint32)
    labels, offsets = lab2d.ravel(), np.arange(0, (num + 1) * 64, 64, dtype=np.uint64)
    monkeypatch.setenv("FSTAMD_SHARD_LOG", "1")
    capfd.readouterr()
    got = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem)
    assert [p[-1] for p in shard_log(capfd.readouterr().err)] == ["streamed"]
    monkeypatch.setenv("FSTAMD_STREAM", "0")
    ref = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem)
    for a, b in ((got.status, ref.status), (got.offsets, ref.offsets), (got.ilabels, ref.ilabels),
                 (got.olabels, ref.olabels), (bits(got.weights), bits(ref.weights)),
                 (bits(got.finals), bits(ref.finals))):
        assert np.array_equal(a, b)
    # a sample against the oracle, through the text projection of both
    idx = np.unique(np.concatenate([rng.choice(num, 60, replace=False), [0, num - 1]]))
    texts = [(lab2d[i] - 1).astype(np.uint8).tobytes() for i in idx]
    wtexts, wstatus, wtw = expected([metric_blob()], texts, sem)
    conv = F.batch_result_to_text(got)
    all_texts = conv.texts()
    assert np.array_equal(conv.status[idx], wstatus)
    assert [all_texts[i] for i in idx] == wtexts
    assert np.array_equal(bits(conv.total_weight[idx]), bits(wtw))
