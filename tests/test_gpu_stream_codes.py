"""The streamed batch's weight codes (batch_streamed.cpp, code_pull.hip): on an rhs whose tier P
records hold the arc weight as a byte (RK 2..6) the pull tier sends one byte per arc to a
pinned staging block, and host threads expand each finished part's codes into the result's
f64 weights after that part's completion event.  FSTAMD_STREAM_CODES: 0 = the f64 copy-out,
1 = every part coded, 2 = all but the last.

Every case compares the whole result byte for byte with the same call under
FSTAMD_STREAM_CODES=0, compares >= 512 strings (every special one among them) with the
oracle, and asserts the route from FSTAMD_ROUTE_LOG's `stream: weight codes on|off` line.
"""
import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O
from test_gpu_parity import EAGER, LAZY, bits, expected_status, load_blob

pytestmark = pytest.mark.gpu

TAG = "[libfst_amd route] stream: weight codes "


def routes(err):
    """[(on|off, mode, parts)] of the calls logged in `err`"""
    out = []
    for ln in err.splitlines():
        if ln.startswith(TAG):
            w = ln[len(TAG):].replace(",", "").split()  # on mode 1 parts 3
            out.append((w[0], int(w[2]), int(w[4])))
    return out


def same_result(a, b):
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.offsets, b.offsets)
    assert np.array_equal(a.ilabels, b.ilabels)
    assert np.array_equal(a.olabels, b.olabels)
    assert np.array_equal(bits(a.weights), bits(b.weights))
    assert np.array_equal(bits(a.finals), bits(b.finals))


def oracle_sample(blob, labels, offsets, sem, idx):
    base = int(offsets[0])
    sub = [labels[int(offsets[i]) - base:int(offsets[i + 1]) - base] for i in idx]
    so = np.concatenate([[0], np.cumsum([len(q) for q in sub])]).astype(np.uint64)
    sl = np.concatenate(sub).astype(np.uint32)
    return O.batch_run(blob, sl, so, 0 if sem == LAZY else 1, 1, 8)


def compare_sample(got, ref, idx):
    exp = expected_status(ref)
    assert np.array_equal(got.status[idx], exp)
    for j, i in enumerate(idx):
        a0, a1 = int(got.offsets[i]), int(got.offsets[i + 1])
        if exp[j] != F.FST_PATH_OK:
            assert a1 == a0  # compacted out
            continue
        b0, b1 = int(ref.offsets[j]), int(ref.offsets[j + 1])
        assert np.array_equal(got.ilabels[a0:a1], ref.ilabels[b0:b1]), i
        assert np.array_equal(got.olabels[a0:a1], ref.olabels[b0:b1]), i
        assert np.array_equal(bits(got.weights[a0:a1]), bits(ref.weights[b0:b1])), i
        assert bits(got.finals[i]) == bits(ref.finals[j]), i


def run_logged(capfd, rhs, labels, offsets, sem=EAGER, **kw):
    capfd.readouterr()
    got = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem, **kw)
    return got, routes(capfd.readouterr().err)


def coded_vs_plain(monkeypatch, capfd, rhs, labels, offsets, want, sem=EAGER, **kw):
    """The call as the environment stands (route asserted: `want`, a list of (on|off, mode,
    parts) or of on|off alone), then under FSTAMD_STREAM_CODES=0 (off): equal bytes."""
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    got, r = run_logged(capfd, rhs, labels, offsets, sem, **kw)
    assert (r if isinstance(want[0], tuple) else [x[0] for x in r]) == want, r
    with monkeypatch.context() as m:
        m.setenv("FSTAMD_STREAM_CODES", "0")
        plain, r0 = run_logged(capfd, rhs, labels, offsets, sem, **kw)
    assert r0 and all(x[0] == "off" and x[1] == 0 for x in r0), r0
    same_result(got, plain)
    return got


# ---- record kinds: the ambiguous chain at T = 256 (weights 0..3) with its weights remapped ----
def chain(weight_of):
    f = O.gen("ambiguous", 256, 12)
    a = 0
    for s, al in enumerate(f.arcs):
        for k, (il, ol, w, nx) in enumerate(al):
            al[k] = (il, ol, float(weight_of(w, a)), nx)
            a += 1
    return O.freeze(f)


KINDS = {
    # name: (weights, environment, codes)
    "rk6": (lambda w, a: w, {}, "on"),
    "rk3": (lambda w, a: w, {"FSTAMD_NO_PACK": "1"}, "on"),
    "rk2": (lambda w, a: w, {"FSTAMD_NO_REC4": "1"}, "on"),
    "scale2": (lambda w, a: w + 0.5, {}, "on"),
    "scale256": (lambda w, a: (w + 1 + a % 4) / 256.0, {}, "on"),
    "rk4": (lambda w, a: w + 0.1, {}, "on"),
    "rk5": (lambda w, a: w + 0.1 + (a % 50) * 0.013, {}, "on"),       # 200 distinct weights
    "rk1_wide": (lambda w, a: w * 100.0, {}, "off"),                  # weights up to 300
    "rk0_many": (lambda w, a: w + 0.1 + (a % 300) * 0.001, {}, "off"),  # > 256, non-dyadic
}


@pytest.fixture(scope="module")
def mixed_strings():
    """2,000 strings of lengths 0..130 (every slot residue mod 4, 16 and 64), mostly 1s; a
    few hold the dead label 2 (no path: compacted out)"""
    rng = np.random.default_rng(2026)
    lens = rng.integers(0, 131, 2000)
    lens[:4] = [0, 1, 130, 64]
    seqs = []
    for i, L in enumerate(lens):
        q = np.ones(L, np.uint32)
        if L and i % 41 == 7:
            q[int(rng.integers(0, L))] = 2
        seqs.append(q)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    special = [i for i in range(2000) if i % 41 == 7 or lens[i] == 0][:150]
    idx = np.unique(np.concatenate([rng.choice(2000, 520, replace=False), special, [0, 1999]]))
    return np.concatenate(seqs).astype(np.uint32), offsets, idx.astype(np.int64)


@pytest.mark.parametrize("kind", list(KINDS))
def test_record_kinds(kind, mixed_strings, monkeypatch, capfd):
    weight_of, env, want = KINDS[kind]
    labels, offsets, idx = mixed_strings
    blob = chain(weight_of)
    rhs = load_blob(blob)
    monkeypatch.setenv("FSTAMD_P_GRID", "8")  # 8 waves: every chase with up to 16 jobs pending
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = coded_vs_plain(monkeypatch, capfd, rhs, labels, offsets, [want])
    assert len(idx) >= 512
    compare_sample(got, oracle_sample(blob, labels, offsets, EAGER, idx), idx)


def test_lazy_semantics_keep_the_f64_copy_out(mixed_strings, monkeypatch, capfd):
    labels, offsets, idx = mixed_strings
    blob = chain(lambda w, a: w)
    got = coded_vs_plain(monkeypatch, capfd, load_blob(blob), labels, offsets, ["off"], sem=LAZY)
    compare_sample(got, oracle_sample(blob, labels, offsets, LAZY, idx), idx)


def test_text_entry_keeps_its_emission(monkeypatch, capfd):
    rhs = F.Fst.bench_transducer(F.BENCH_AMBIGUOUS, 256, 12)
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    texts = [bytes([0] * L) for L in range(0, 60)]  # (byte 0 = label 1)
    capfd.readouterr()
    a = F.normalize_text_batch([rhs], texts, EAGER)
    r = routes(capfd.readouterr().err)
    assert r and all(x[0] == "off" for x in r), r
    monkeypatch.setenv("FSTAMD_STREAM_CODES", "0")
    b = F.normalize_text_batch([rhs], texts, EAGER)
    assert np.array_equal(a.status, b.status) and np.array_equal(a.offsets, b.offsets)
    assert np.array_equal(a.text, b.text)
    assert np.array_equal(bits(a.total_weight), bits(b.total_weight))


# ---- parts: 33,000 strings x 128 labels, the smallest batch the part rule splits ----
@pytest.fixture(scope="module")
def chain256():
    return F.Fst.bench_transducer(F.BENCH_AMBIGUOUS, 256, 12), O.freeze(O.gen("ambiguous", 256, 12))


@pytest.fixture(scope="module")
def split_batch(chain256):
    rng = np.random.default_rng(33000)
    lab = np.ones((33000, 128), np.uint32)
    dead = np.arange(13, 33000, 61)  # the dead label: no path, in every part
    lab[dead, rng.integers(0, 128, len(dead))] = 2
    offsets = np.arange(0, 33001 * 128, 128, dtype=np.uint64)
    idx = np.unique(np.concatenate([rng.choice(33000, 400, replace=False), dead[::4],
                                    [0, 32999]])).astype(np.int64)
    assert len(idx) >= 512
    return lab.ravel(), offsets, idx, oracle_sample(chain256[1], lab.ravel(), offsets, EAGER, idx)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("cuts,parts", [("500", 2), ("23,163", 3), ("60,200,500,850", 5)])
def test_parts(chain256, split_batch, cuts, parts, mode, monkeypatch, capfd):
    labels, offsets, idx, ref = split_batch
    monkeypatch.setenv("FSTAMD_STREAM_CUTS", cuts)
    monkeypatch.setenv("FSTAMD_STREAM_CODES", str(mode))
    got = coded_vs_plain(monkeypatch, capfd, chain256[0], labels, offsets, [("on", mode, parts)])
    compare_sample(got, ref, idx)


def test_default_cuts_and_mode(chain256, split_batch, monkeypatch, capfd):
    labels, offsets, idx, ref = split_batch
    got = coded_vs_plain(monkeypatch, capfd, chain256[0], labels, offsets, ["on"])
    compare_sample(got, ref, idx)


def test_first_offset_not_zero(chain256, split_batch, monkeypatch, capfd):
    labels, offsets, idx, ref = split_batch
    shifted = np.concatenate([np.full(5, 2, np.uint32), labels])
    monkeypatch.setenv("FSTAMD_STREAM_CUTS", "23,163")
    got = coded_vs_plain(monkeypatch, capfd, chain256[0], shifted, offsets + np.uint64(5),
                         [("on", 1, 3)])
    compare_sample(got, ref, idx)


def test_three_shards_on_one_gpu(chain256, monkeypatch, capfd):
    # lengths 120..136: the shards' first labels fall on odd offsets, so their slices of the
    # result start off every alignment the copy-out and the expander care about
    rhs, blob = chain256
    rng = np.random.default_rng(333)
    lens = rng.integers(120, 137, 33000)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    labels = np.ones(int(offsets[-1]), np.uint32)
    dead = np.arange(5, 33000, 67)
    labels[offsets[dead].astype(np.int64) + 3] = 2
    got = coded_vs_plain(monkeypatch, capfd, rhs, labels, offsets, ["on"] * 3, devices=[0],
                         shards=3)
    idx = np.unique(np.concatenate([rng.choice(33000, 420, replace=False), dead[::4],
                                    [0, 10999, 11000, 21999, 22000, 32999]])).astype(np.int64)
    assert len(idx) >= 512
    compare_sample(got, oracle_sample(blob, labels, offsets, EAGER, idx), idx)


# ---- fix-ups: strings the pull tier hands on, finished by the later tiers as f64 ----
@pytest.fixture(scope="module")
def fixup_batch():
    rhs = F.Fst.bench_transducer(F.BENCH_AMBIGUOUS, 1024, 12)
    blob = O.freeze(O.gen("ambiguous", 1024, 12))
    rng = np.random.default_rng(9001)
    num = 38000
    lens = rng.integers(100, 131, num)
    seqs = []
    for i, L in enumerate(lens):
        q = np.ones(L, np.uint32)
        kind = i % 389
        if kind == 5:
            q[int(rng.integers(0, L))] = 0   # label 0: the pull tier hands it on
        elif kind == 11:
            q[int(rng.integers(0, L))] = 3   # no rhs arc: no path
        elif kind == 17:
            q = q[:0]                        # the empty string
        elif kind == 23 and i % 4 == 3:
            q = np.ones(900, np.uint32)      # beyond the pull tier's window
        seqs.append(q)
    offsets = np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).astype(np.uint64)
    labels = np.concatenate(seqs).astype(np.uint32)
    special = [i for i in range(num) if i % 389 in (5, 11, 17) or (i % 389 == 23 and i % 4 == 3)]
    idx = np.unique(np.concatenate([rng.choice(num, 260, replace=False), special,
                                    [0, num - 1]])).astype(np.int64)
    assert len(idx) >= 512 and offsets[-1] >= (1 << 22)
    return rhs, labels, offsets, idx, oracle_sample(blob, labels, offsets, EAGER, idx)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("few", [None, "0"])
def test_fixups(fixup_batch, few, mode, monkeypatch, capfd):
    # few = 0: the bulk fix-up downloads the whole f64 arena, which holds no pull-tier weight
    # of a coded part -- it must not clobber what the expanders wrote
    rhs, labels, offsets, idx, ref = fixup_batch
    if few is not None:
        monkeypatch.setenv("FSTAMD_STREAM_FIX_FEW", few)
    monkeypatch.setenv("FSTAMD_STREAM_CODES", str(mode))
    got = coded_vs_plain(monkeypatch, capfd, rhs, labels, offsets, ["on"])
    compare_sample(got, ref, idx)


# ---- a failing call with expanders in flight ----
def test_error_after_pull_with_expanders_in_flight(chain256, split_batch, monkeypatch, capfd):
    labels, offsets, idx, ref = split_batch
    monkeypatch.setenv("FSTAMD_ROUTE_LOG", "1")
    monkeypatch.setenv("FSTAMD_FAULT_INJECT", "stream_after_pull")
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        F.compose_frozen_shortest_path_batch(chain256[0], labels, offsets, 1, EAGER)
    assert [x[0] for x in routes(capfd.readouterr().err)] == ["on"]
    monkeypatch.delenv("FSTAMD_FAULT_INJECT")
    for _ in range(2):  # the pooled staging block and arenas serve the next calls
        got, r = run_logged(capfd, chain256[0], labels, offsets)
        assert [x[0] for x in r] == ["on"]
        compare_sample(got, ref, idx)
