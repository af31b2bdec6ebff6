"""CPU tests of the aligned text entries (include/fst_batch.h, FstAlignedTextResult): the symbols
exist, the header compiles and the ctypes mirror has the header's layout, the entry checks its
arguments as fst_normalize_text_batch does, and the host conversion
fst_batch_result_to_aligned_text follows the definition as tests/align_model.py restates it.
No GPU is used here; the device kernels are checked against the same model in
test_gpu_text_align.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import libfst_amd as F
from libfst_amd import fst as FF
import oracle_ffi as O
from align_model import align, compose, stage_map
from test_text_api import python_text

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_SYMBOLS = ["fst_normalize_text_aligned_batch", "fst_aligned_text_result_free",
                 "fst_device_path_alignment", "fst_device_compose_alignment",
                 "fst_batch_result_to_aligned_text"]
OK, EMPTY, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED


def hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_library_exports_the_alignment_symbols():
    L = F.lib()
    header = open(os.path.join(REPO, "include", "fst_batch.h")).read()
    for n in ALIGN_SYMBOLS:
        assert hasattr(L, n), n
        assert n in FF.SIGNATURES, n
        assert n + "(" in header, n
    assert "FstAlignedTextResult" in header
    for n in ("AlignedTextResult", "normalize_text_aligned_batch", "batch_result_to_aligned_text"):
        assert hasattr(F, n), n


def test_header_compiles_and_the_mirror_has_its_layout(tmp_path):
    """Every field of the ctypes mirror at the header's offset, checked by the compiler."""
    checks = [f"static_assert(sizeof(FstAlignedTextResult) == {C.sizeof(FF.FstAlignedTextResult)}, "
              '"size");\n']
    for name, _ in FF.FstAlignedTextResult._fields_:
        off = getattr(FF.FstAlignedTextResult, name).offset
        checks.append(f'static_assert(offsetof(FstAlignedTextResult, {name}) == {off}, "{name}");\n')
    # the text result is a prefix of it, field for field
    for name, _ in FF.FstTextResult._fields_:
        checks.append(f"static_assert(offsetof(FstAlignedTextResult, {name}) == "
                      f'offsetof(FstTextResult, {name}), "prefix {name}");\n')
    assert [n for n, _ in FF.FstAlignedTextResult._fields_][-2:] == ["in_begin", "in_end"]
    src = tmp_path / "use_align.cpp"
    src.write_text('#include <cstddef>\n#include "fst_batch.h"\n' + "".join(checks) +
                   "void* use_align[] = {\n" +
                   "".join(f"    (void*)&{n},\n" for n in ALIGN_SYMBOLS) + "};\n")
    r = subprocess.run([hipcc(), "-x", "c++", "-I", os.path.join(REPO, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use_align.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the host conversion against the model ----------------------------------------------

def batch(paths):
    """A BatchResult from [(status, ilabels, olabels)] (weights 0.5 per arc, final 0.25)."""
    lens = [len(p[1]) for p in paths]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    flat = lambda k: np.asarray([x for p in paths for x in p[k]], np.uint32)
    return F.BatchResult(status=np.asarray([p[0] for p in paths], np.int32), offsets=off,
                         ilabels=flat(1), olabels=flat(2), weights=np.full(int(off[-1]), 0.5),
                         finals=np.full(len(paths), 0.25))


def model(r):
    """(begin, end) per string from the model, [] for every string python_text reports not OK."""
    _, status, _ = python_text(r)
    out = []
    for i, st in enumerate(status):
        a, z = int(r.offsets[i]), int(r.offsets[i + 1])
        out.append(align([(r.ilabels[a:z].tolist(), r.olabels[a:z].tolist())]) if st == OK
                   else ([], []))
    return out


def check(paths):
    r = batch(paths)
    t = F.batch_result_to_aligned_text(r)
    plain = F.batch_result_to_text(r)
    for x, y in ((t.status, plain.status), (t.offsets, plain.offsets), (t.text, plain.text),
                 (t.total_weight, plain.total_weight)):
        assert x.tobytes() == y.tobytes()
    assert len(t.in_begin) == len(t.in_end) == len(t.text)
    for i, (b, e) in enumerate(model(r)):
        a, z = int(t.offsets[i]), int(t.offsets[i + 1])
        assert t.in_begin[a:z].tolist() == b and t.in_end[a:z].tolist() == e, i
    return t


def test_model_on_known_answers():
    assert stage_map([], []) == ([], [], 0)
    # x:y, eps:y, x:eps, x:y
    assert stage_map([5, 0, 6, 7], [9, 8, 0, 7]) == ([0, 1, 2], [1, 1, 3], 3)
    # stage 2 maps its two consumed symbols and inserts once its input is exhausted (b == M)
    assert compose([0, 0], [1, 1], [0, 1, 2], [1, 2, 2], 1) == ([0, 0, 1], [1, 1, 1])
    # M == 0: everything is an insertion at N1
    assert compose([], [], [0, 0], [0, 0], 4) == ([4, 4], [4, 4])
    # five symbols from one consumed byte: the consuming arc's is [0, 1), the eps:y arcs after
    # it sit at the boundary behind it; a copying second stage keeps the map
    tag = ([56, 0, 0, 0, 0], [116, 102, 119, 102, 111])
    assert align([tag, ([116, 102, 119, 102, 111],) * 2]) == ([0, 1, 1, 1, 1], [1] * 5)
    # synthetic's cascade on "7": 7:# eps:h, then #:eps h:eps and five eps:y arcs (b == M)
    assert align([([56, 0], [36, 105]), ([36, 105] + [0] * 5, [0, 0, 116, 102, 119, 102, 111])]) \
        == ([1] * 5, [1] * 5)


def test_zero_arcs_and_all_epsilon_outputs():
    t = check([(OK, [], []), (OK, [5, 6, 7], [0, 0, 0]), (OK, [5], [6])])
    assert list(t.offsets) == [0, 0, 0, 1]
    assert t.in_begin.tolist() == [0] and t.in_end.tolist() == [1]


def test_input_epsilon_insertions_before_between_and_after():
    t = check([(OK, [0, 0, 5, 0, 6, 7, 0, 0], [40, 41, 5, 42, 0, 7, 43, 44])])
    assert t.in_begin.tolist() == [0, 0, 0, 1, 2, 3, 3]
    assert t.in_end.tolist() == [0, 0, 1, 1, 3, 3, 3]
    assert t.spans(0) == [(0, 0, 0, 2), (0, 1, 2, 3), (1, 1, 3, 4), (2, 3, 4, 5), (3, 3, 5, 7)]


def test_non_ok_string_between_ok_ones():
    t = check([(OK, [5, 6], [5, 6]), (EMPTY, [], []), (F.FST_PATH_CYCLE, [9, 9], [9, 9]),
               (OK, [0, 7], [8, 7])])
    assert list(t.offsets) == [0, 2, 2, 2, 4]
    assert t.in_begin.tolist() == [0, 1, 0, 0] and t.in_end.tolist() == [1, 2, 0, 1]
    assert t.spans(0) == [(0, 2, 0, 2)] and t.spans(1) == [] and t.spans(3) == [(0, 0, 0, 1), (0, 1, 1, 2)]


@pytest.mark.parametrize("bad", [257, 0xFFFFFFFF])
def test_olabel_above_256_has_no_entries(bad):
    t = check([(OK, [5], [5]), (OK, [5, 6, 7], [5, bad, 7]), (OK, [0, 6], [6, 6])])
    assert list(t.status) == [OK, UNSUPPORTED, OK]
    assert list(t.offsets) == [0, 1, 1, 3]
    assert t.in_begin.tolist() == [0, 0, 0] and t.in_end.tolist() == [1, 0, 1]


def test_spans_merge_rewrites_and_copies():
    # "a7b" -> "asevenb": 'a' and 's' advance with the input (one copied run), "even" comes
    # from eps:y arcs at one boundary (one run with one interval), 'b' is a copy again
    t = check([(OK, [98, 56, 0, 0, 0, 0, 99], [98, 116, 102, 119, 102, 111, 99])])
    assert t.texts() == [b"asevenb"]
    assert t.spans(0) == [(0, 2, 0, 2), (2, 2, 2, 6), (2, 3, 6, 7)]
    # copied text is one segment, a deletion splits it
    t = check([(OK, [5, 6, 7, 8, 9], [5, 6, 0, 8, 9])])
    assert t.spans(0) == [(0, 2, 0, 2), (3, 5, 2, 4)]


def test_random_paths_follow_the_model():
    rng = np.random.default_rng(11)
    paths = []
    for L in (0, 1, 2, 63, 64, 65, 130):
        il = rng.integers(0, 257, L)
        il[rng.random(L) < 0.3] = 0
        ol = rng.integers(0, 257, L)
        ol[rng.random(L) < 0.3] = 0
        paths.append((OK, il.tolist(), ol.tolist()))
    t = check(paths)
    b, e = t.in_begin.astype(np.int64), t.in_end.astype(np.int64)
    assert np.all(b <= e)
    for i in range(len(paths)):
        a, z = int(t.offsets[i]), int(t.offsets[i + 1])
        assert np.all(e[a:z - 1] <= b[a + 1:z]) if z > a else True
        assert np.all(e[a:z] <= sum(x != 0 for x in paths[i][1]))


# ---- arguments and the empty result ------------------------------------------------------

def poisoned(cls):
    r = cls()
    C.memset(C.byref(r), 0x5A, C.sizeof(r))
    return r


def test_host_conversion_bad_arguments_and_no_strings():
    t = F.batch_result_to_aligned_text(batch([]))
    assert len(t.status) == 0 and list(t.offsets) == [0] and t.texts() == []
    assert len(t.in_begin) == 0 and len(t.in_end) == 0
    L = F.lib()
    res = poisoned(FF.FstAlignedTextResult)
    assert L.fst_batch_result_to_aligned_text(None, res) == FF.FST_INVALID_ARG
    src = FF.FstBatchResult()
    assert L.fst_batch_result_to_aligned_text(src, None) == FF.FST_INVALID_ARG
    st, fin = np.zeros(1, np.int32), np.zeros(1, np.float64)
    cast = lambda a, ct: C.cast(a.ctypes.data, C.POINTER(ct))
    off = np.asarray([4, 2], np.uint64)   # decreasing
    src = FF.FstBatchResult(1, cast(st, C.c_int32), cast(off, C.c_uint64), None, None, None,
                            cast(fin, C.c_double), 0)
    assert L.fst_batch_result_to_aligned_text(src, res) == FF.FST_INVALID_ARG
    assert bytes(res) == bytes(C.sizeof(res))   # zeroed once the arguments were checked
    # arcs but no ilabels: the map needs them
    off = np.asarray([0, 1], np.uint64)
    ol, w = np.ones(1, np.uint32), np.ones(1, np.float64)
    src = FF.FstBatchResult(1, cast(st, C.c_int32), cast(off, C.c_uint64), None,
                            cast(ol, C.c_uint32), cast(w, C.c_double), cast(fin, C.c_double), 1)
    res = poisoned(FF.FstAlignedTextResult)
    assert L.fst_batch_result_to_aligned_text(src, res) == FF.FST_INVALID_ARG
    assert bytes(res) == bytes(C.sizeof(res))
    L.fst_aligned_text_result_free(res)   # an empty result: a no-op
    L.fst_aligned_text_result_free(None)


def entry_calls():
    """(name, stages, num_stages, text, offsets, num_strings, opts) of every rejected call."""
    f = O.Fst()
    f.add_state(0.0)
    f.start = 0
    f.add_arc(0, 98, 98, 0.0, 0)
    good = F.Fst.from_bytes(O.freeze(f))
    hs = (C.c_uint64 * 2)(good.h, good.h)
    stale = (C.c_uint64 * 2)(good.h, F.FST_INVALID_HANDLE)
    text = np.frombuffer(b"aaaa", np.uint8)
    off = np.asarray([0, 2, 4], np.uint64)
    down = np.asarray([0, 3, 2], np.uint64)
    flags = FF.FstBatchOptions(-1, 0, 2, 0, 0)   # an unknown flag
    P = lambda a: a.ctypes.data
    return good, [
        ("no stages", None, 1, P(text), P(off), 2, None),
        ("zero stages", hs, 0, P(text), P(off), 2, None),
        ("no offsets", hs, 1, P(text), None, 2, None),
        ("no text for bytes", hs, 1, None, P(off), 2, None),
        ("decreasing offsets", hs, 1, P(text), P(down), 2, None),
        ("unknown flags", hs, 1, P(text), P(off), 2, C.pointer(flags)),
        ("stale handle", stale, 2, P(text), P(off), 2, None),
        ("stale handle, no strings", stale, 2, P(text), P(off), 0, None),
    ], (hs, stale, text, off, down, flags)


def test_entry_checks_its_arguments_as_the_text_entry_does():
    L = F.lib()
    good, calls, keep = entry_calls()
    assert L.fst_normalize_text_aligned_batch(keep[0], 1, None, keep[3].ctypes.data, 2, None,
                                              None) == FF.FST_INVALID_ARG
    n_text = C.sizeof(FF.FstTextResult)
    zeroed = 0
    for name, *args in calls:
        a = poisoned(FF.FstAlignedTextResult)
        t = poisoned(FF.FstTextResult)
        assert L.fst_normalize_text_aligned_batch(*args, a) == FF.FST_INVALID_ARG, name
        assert L.fst_normalize_text_batch(*args, t) == FF.FST_INVALID_ARG, name
        # *out zeroed exactly where the text entry zeroes its own
        assert bytes(a)[:n_text] == bytes(t), name
        if bytes(t) == bytes(n_text):
            assert bytes(a) == bytes(C.sizeof(a)), name
            zeroed += 1
        else:
            assert bytes(a) == b"\x5a" * C.sizeof(a), name
    assert zeroed == 4   # every check after the null-pointer ones


def test_no_strings_is_the_empty_ok_result():
    L = F.lib()
    good, _, keep = entry_calls()
    res = poisoned(FF.FstAlignedTextResult)
    zero = np.zeros(1, np.uint64)
    assert L.fst_normalize_text_aligned_batch(keep[0], 2, None, zero.ctypes.data, 0, None,
                                              res) == FF.FST_OK
    assert res.num_strings == 0 and res.total_bytes == 0 and res.text_offsets[0] == 0
    assert res.status and res.text and res.total_weight and res.in_begin and res.in_end
    L.fst_aligned_text_result_free(res)
    assert bytes(res) == bytes(C.sizeof(res))   # freed: zeroed, a second free is a no-op
    L.fst_aligned_text_result_free(res)
    r = F.normalize_text_aligned_batch([good], [])
    assert len(r.status) == 0 and list(r.offsets) == [0] and len(r.in_begin) == 0
