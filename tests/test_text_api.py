"""CPU tests of the text entries (include/fst_batch.h): the five symbols exist and the header
compiles, and the host conversion fst_batch_result_to_text follows the reference's
printOutputString (src/string.zig:60-97) and its left-fold total weight -- on hand-built
results and against the oracle's own print_string.  No GPU is used here; the device
emission is checked against the same conversion in test_gpu_text.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import libfst_amd as F
from libfst_amd import fst as FF
from libfst_amd import synthetic as SY
import oracle_ffi as O
from test_gpu_configs import oracle_fst
from test_gpu_parity import bits, expected_status

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_SYMBOLS = ["fst_normalize_text_batch", "fst_text_result_free", "fst_device_compile_text",
                "fst_device_emit_text", "fst_batch_result_to_text"]
OK, EMPTY, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED


def test_library_exports_the_text_symbols():
    L = F.lib()
    header = open(os.path.join(REPO, "include", "fst_batch.h")).read()
    for n in TEXT_SYMBOLS:
        assert hasattr(L, n), n
        assert n in FF.SIGNATURES, n
        assert n + "(" in header, n
    assert "FstTextResult" in header


def test_header_compiles_and_declares_the_text_entries(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "use_text.c"
    src.write_text(
        '#include "fst_batch.h"\n'
        "void* use_text[] = {\n" + "".join(f"    (void*)&{n},\n" for n in TEXT_SYMBOLS) + "};\n"
        "unsigned long use_size = sizeof(FstTextResult);\n")
    r = subprocess.run([hipcc, "-x", "c++", "-I", os.path.join(REPO, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use_text.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def batch(paths):
    """A BatchResult from [(status, olabels, weights, final)]."""
    lens = [len(p[1]) for p in paths]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ol = np.asarray([x for p in paths for x in p[1]], np.uint32)
    w = np.asarray([x for p in paths for x in p[2]], np.float64)
    return F.BatchResult(status=np.asarray([p[0] for p in paths], np.int32), offsets=off,
                         ilabels=np.zeros(len(ol), np.uint32), olabels=ol, weights=w,
                         finals=np.asarray([p[3] for p in paths], np.float64))


def fold(weights, final):
    """dist along the path, then times(dist, final) (shortest-path.zig:72)."""
    d = 0.0
    for w in weights:
        d = d + float(w)
    return d + float(final)


def python_text(r):
    """The projection and the fold in Python: (texts, status, total weights)."""
    texts, status, tw = [], [], []
    for i in range(len(r.status)):
        a, b = int(r.offsets[i]), int(r.offsets[i + 1])
        st, out, w = int(r.status[i]), b"", math.inf
        if st == OK:
            ol = [int(x) for x in r.olabels[a:b]]
            if any(x > 256 for x in ol):
                st = UNSUPPORTED
            else:
                out = bytes(x - 1 for x in ol if x)
                w = fold(r.weights[a:b], r.finals[i])
        texts.append(out)
        status.append(st)
        tw.append(w)
    return texts, np.asarray(status, np.int32), np.asarray(tw, np.float64)


def test_epsilons_dropped_and_byte_range():
    t = F.batch_result_to_text(batch([
        (OK, [0, 105, 0, 0, 106, 0], [0.5] * 6, 0.25),   # epsilons at the ends and inside
        (OK, [256, 1, 256], [1.0, 2.0, 3.0], 0.0),        # label 256 -> 0xFF, label 1 -> 0x00
        (OK, [0, 0, 0], [0.0] * 3, 1.0),                  # every output epsilon
    ]))
    assert t.texts() == [b"hi", b"\xff\x00\xff", b""]
    assert list(t.status) == [OK, OK, OK]
    assert list(t.offsets) == [0, 2, 5, 5]
    assert t.text.tobytes() == b"hi\xff\x00\xff"
    assert list(t.total_weight) == [3.25, 6.0, 1.0]


@pytest.mark.parametrize("bad", [257, 0xFFFFFFFF])
def test_non_byte_label_is_unsupported(bad):
    t = F.batch_result_to_text(batch([(OK, [98], [1.0], 0.0), (OK, [98, bad, 99], [1.0] * 3, 0.0),
                                      (OK, [100], [2.0], 0.0)]))
    assert list(t.status) == [OK, UNSUPPORTED, OK]
    assert t.texts() == [b"a", b"", b"c"]
    assert list(t.offsets) == [0, 1, 1, 2]
    assert t.total_weight[1] == math.inf and t.total_weight[2] == 2.0


def test_failed_status_passes_through():
    # a non-OK string has no bytes and +inf, whatever its (ignored) path range holds
    t = F.batch_result_to_text(batch([(EMPTY, [], [], math.inf), (F.FST_PATH_CYCLE, [98], [1.0], 0.0),
                                      (OK, [99], [1.5], 0.5)]))
    assert list(t.status) == [EMPTY, F.FST_PATH_CYCLE, OK]
    assert t.texts() == [b"", b"", b"b"]
    assert t.total_weight[0] == math.inf and t.total_weight[1] == math.inf
    assert t.total_weight[2] == 2.0


def test_zero_length_path_keeps_the_final_weight():
    t = F.batch_result_to_text(batch([(OK, [], [], 0.75)]))
    assert list(t.status) == [OK] and t.texts() == [b""]
    assert list(t.offsets) == [0, 0]
    assert bits(t.total_weight)[0] == bits([0.75])[0]


def test_total_weight_is_the_left_fold():
    ws = [0.1] * 10 + [0.7]
    pairwise = lambda x: x[0] if len(x) == 1 else pairwise(x[:len(x) // 2]) + pairwise(x[len(x) // 2:])
    assert fold(ws, 0.0) != pairwise(ws) + 0.0      # the case tells the two apart
    t = F.batch_result_to_text(batch([(OK, [98] * 11, ws, 0.0), (OK, [98] * 11, ws, 0.3)]))
    assert bits(t.total_weight)[0] == bits([fold(ws, 0.0)])[0]
    assert bits(t.total_weight)[1] == bits([fold(ws, 0.3)])[0]
    assert bits(t.total_weight)[0] != bits([pairwise(ws)])[0]


def test_no_strings_and_bad_arguments():
    t = F.batch_result_to_text(batch([]))
    assert len(t.status) == 0 and list(t.offsets) == [0] and t.texts() == []
    L = F.lib()
    res = FF.FstTextResult()
    assert L.fst_batch_result_to_text(None, res) == FF.FST_INVALID_ARG
    st = np.zeros(1, np.int32)
    off = np.asarray([4, 2], np.uint64)   # decreasing
    fin = np.zeros(1, np.float64)
    P = FF.C.POINTER
    cast = lambda a, ct: FF.C.cast(a.ctypes.data, P(ct))
    src = FF.FstBatchResult(1, cast(st, FF.C.c_int32), cast(off, FF.C.c_uint64), None, None, None,
                            cast(fin, FF.C.c_double), 0)
    res.num_strings = 7
    assert L.fst_batch_result_to_text(src, res) == FF.FST_INVALID_ARG
    assert res.num_strings == 0 and not res.text   # zeroed once the arguments were checked
    # the text entry checks its arguments before it needs a device
    h = (FF.C.c_uint64 * 1)(F.FST_INVALID_HANDLE)
    zero = np.zeros(1, np.uint64)
    assert L.fst_normalize_text_batch(h, 1, None, zero.ctypes.data, 0, None, res) == FF.FST_INVALID_ARG
    assert L.fst_normalize_text_batch(h, 0, None, zero.ctypes.data, 0, None, res) == FF.FST_INVALID_ARG
    L.fst_text_result_free(res)   # an empty result: a no-op


@pytest.mark.parametrize("sem", [0, 1])
def test_host_conversion_matches_oracle_print_string(sem):
    """printOutputString of the oracle's own 1-best chain, utterance by utterance, against the
    host conversion of the oracle's batch result."""
    blob = O.freeze(oracle_fst(SY.tagger()))
    rng = np.random.default_rng(17)
    texts = SY.utterances(rng, 50) + ["", "7", "#", "ab#", "A"]   # the last three have no path
    labels, offsets = SY.to_labels(texts)
    ref = O.batch_run(blob, labels, offsets, sem, 1)
    r = F.BatchResult(status=expected_status(ref), offsets=ref.offsets, ilabels=ref.ilabels,
                      olabels=ref.olabels, weights=ref.weights, finals=ref.finals)
    t = F.batch_result_to_text(r)
    got = t.texts()
    dead = 0
    for i, s in enumerate(texts):
        lhs = O.compile_string(s.encode())
        if sem == 0:
            rc, best = O.compose_shortest_path(lhs, blob, 1)
        else:
            rc, lat = O.compose(lhs, blob)
            assert rc == O.OR_OK
            rc, best = O.shortest_path(lat, 1)
        assert rc == O.OR_OK
        want = O.print_string(best, tape=1)
        if want is None:
            dead += 1
            assert t.status[i] != OK and got[i] == b"" and t.total_weight[i] == math.inf, (i, s)
        else:
            assert t.status[i] == OK and got[i] == want, (i, s)
            ch = O.chain(best)
            assert bits(t.total_weight)[i] == bits([fold(ch[2], ch[3])])[0], (i, s)
    assert dead == 3
    py_texts, py_status, py_tw = python_text(r)
    assert got == py_texts and np.array_equal(t.status, py_status)
    assert np.array_equal(bits(t.total_weight), bits(py_tw))
