"""Python host mirror of libfst's C ABI for the frozen-compose hot path.

Thin ctypes binding of libfst_amd.so (include/fst.h + include/fst_batch.h).  Names,
argument meaning and error behaviour follow the reference C API
(ontypehq/libfst src/c-api.zig): handles are u64, FST_INVALID_HANDLE signals
failure, n-shortest accepts only n in {0, 1}.  All compose / shortest-path work runs
in the HIP kernels of libfst_amd.so; if the library or a GPU is missing these calls
raise instead of computing anything on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# LIBFST_AMD_LIB: an alternate build of the same library (A/B runs of kernel variants).
LIB_PATH = os.environ.get("LIBFST_AMD_LIB") or os.path.join(PKG_DIR, "libfst_amd.so")

FST_NO_STATE = 0xFFFFFFFF
FST_EPSILON = 0
FST_INVALID_HANDLE = 0xFFFFFFFFFFFFFFFF

FST_OK, FST_OOM, FST_INVALID_ARG, FST_INVALID_STATE, FST_IO_ERROR = range(5)
FST_SEM_LAZY, FST_SEM_EAGER = 0, 1
(FST_PATH_OK, FST_PATH_EMPTY, FST_PATH_ERROR_N, FST_PATH_CYCLE, FST_PATH_OVERFLOW,
 FST_PATH_UNSUPPORTED, FST_PATH_OUTPUT_FULL, FST_PATH_INTERNAL) = range(8)

BENCH_AMBIGUOUS, BENCH_EPS_DENSE, BENCH_BRANCHING = 0, 1, 2


class FstArc(C.Structure):
    _fields_ = [("ilabel", C.c_uint32), ("olabel", C.c_uint32), ("weight", C.c_double),
                ("nextstate", C.c_uint32)]


class FstBatchResult(C.Structure):
    _fields_ = [("num_strings", C.c_uint32), ("status", C.POINTER(C.c_int32)),
                ("path_offsets", C.POINTER(C.c_uint64)), ("ilabels", C.POINTER(C.c_uint32)),
                ("olabels", C.POINTER(C.c_uint32)), ("weights", C.POINTER(C.c_double)),
                ("final_weights", C.POINTER(C.c_double)), ("total_arcs", C.c_uint64)]


class FstTextResult(C.Structure):
    _fields_ = [("num_strings", C.c_uint32), ("status", C.POINTER(C.c_int32)),
                ("text_offsets", C.POINTER(C.c_uint64)), ("text", C.POINTER(C.c_uint8)),
                ("total_weight", C.POINTER(C.c_double)), ("total_bytes", C.c_uint64)]


class FstAlignedTextResult(C.Structure):
    _fields_ = FstTextResult._fields_ + [("in_begin", C.POINTER(C.c_uint32)),
                                         ("in_end", C.POINTER(C.c_uint32))]


FST_BATCH_DEVICES = 1


class FstBatchOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("semantics", C.c_uint32), ("flags", C.c_uint32),
                ("num_shards", C.c_uint32), ("device_mask", C.c_uint64)]


def batch_options(device=-1, semantics=FST_SEM_LAZY, devices=None, shards=0) -> FstBatchOptions:
    """FstBatchOptions; `devices` (a list of HIP ordinals) shards the batch over them
    (FST_BATCH_DEVICES), `shards` > len(devices) runs several shards per device."""
    if devices is None and not shards:
        return FstBatchOptions(device, semantics, 0, 0, 0)
    devs = list(devices) if devices is not None else [max(device, 0)]
    mask = 0
    for d in devs:
        mask |= 1 << int(d)
    return FstBatchOptions(device, semantics, FST_BATCH_DEVICES, int(shards), mask)


class FstLhsBatch(C.Structure):
    _fields_ = [("num_fsts", C.c_uint32), ("state_offsets", C.c_void_p), ("start", C.c_void_p),
                ("final_weights", C.c_void_p), ("arc_offsets", C.c_void_p),
                ("ilabels", C.c_void_p), ("olabels", C.c_void_p), ("weights", C.c_void_p),
                ("nextstates", C.c_void_p)]


class FstDeviceBatch(C.Structure):
    _fields_ = [("status", C.c_void_p), ("path_len", C.c_void_p), ("path_offset", C.c_void_p),
                ("final_weight", C.c_void_p), ("ilabels", C.c_void_p), ("olabels", C.c_void_p),
                ("weights", C.c_void_p), ("arc_capacity", C.c_uint64), ("arc_cursor", C.c_void_p),
                ("work", C.c_void_p)]


FST_LATTICE_PROJECT_OUTPUT = 1
FST_LATTICE_CONNECT = 4  # (bit 1 is not assigned)
FST_NBEST_MAX = 16


class FstLatticeBatch(C.Structure):
    _fields_ = [("fsts", FstLhsBatch), ("status", C.POINTER(C.c_int32)),
                ("total_states", C.c_uint64), ("total_arcs", C.c_uint64)]


class FstDeviceLattices(C.Structure):
    _fields_ = [("status", C.c_void_p), ("state_offsets", C.c_void_p), ("start", C.c_void_p),
                ("final_weights", C.c_void_p), ("arc_offsets", C.c_void_p),
                ("ilabels", C.c_void_p), ("olabels", C.c_void_p), ("weights", C.c_void_p),
                ("nextstates", C.c_void_p), ("state_capacity", C.c_uint64),
                ("arc_capacity", C.c_uint64)]


class FstPosteriorResult(C.Structure):
    _fields_ = [("num_fsts", C.c_uint32), ("status", C.POINTER(C.c_int32)),
                ("total", C.POINTER(C.c_double)), ("alpha", C.POINTER(C.c_double)),
                ("beta", C.POINTER(C.c_double)), ("arc_cost", C.POINTER(C.c_double)),
                ("total_states", C.c_uint64), ("total_arcs", C.c_uint64)]


class FstDevicePosteriors(C.Structure):
    _fields_ = [("status", C.c_void_p), ("total", C.c_void_p), ("alpha", C.c_void_p),
                ("beta", C.c_void_p), ("arc_cost", C.c_void_p)]


class FstLaunchStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("launches", C.c_uint32), ("engine", C.c_uint32),
                ("grid", C.c_uint32)]


# Every symbol include/fst.h and include/fst_batch.h declare, with its ctypes signature.
_u32, _u64, _f64, _i32, _P = C.c_uint32, C.c_uint64, C.c_double, C.c_int32, C.c_void_p
SIGNATURES = {
    "fst_mutable_new": (_u64, []),
    "fst_mutable_clone": (_u64, [_u64]),
    "fst_mutable_free": (None, [_u64]),
    "fst_mutable_add_state": (_u32, [_u64]),
    "fst_mutable_set_start": (C.c_int, [_u64, _u32]),
    "fst_mutable_set_final": (C.c_int, [_u64, _u32, _f64]),
    "fst_mutable_add_arc": (C.c_int, [_u64, _u32, _u32, _u32, _f64, _u32]),
    "fst_mutable_start": (_u32, [_u64]),
    "fst_mutable_num_states": (_u32, [_u64]),
    "fst_mutable_num_arcs": (_u32, [_u64, _u32]),
    "fst_mutable_final_weight": (_f64, [_u64, _u32]),
    "fst_mutable_get_arcs": (_u32, [_u64, _u32, C.POINTER(FstArc), _u32]),
    "fst_freeze": (_u64, [_u64]),
    "fst_free": (None, [_u64]),
    "fst_start": (_u32, [_u64]),
    "fst_num_states": (_u32, [_u64]),
    "fst_num_arcs": (_u32, [_u64, _u32]),
    "fst_final_weight": (_f64, [_u64, _u32]),
    "fst_get_arcs": (_u32, [_u64, _u32, C.POINTER(FstArc), _u32]),
    "fst_load": (_u64, [C.c_char_p]),
    "fst_save": (C.c_int, [_u64, C.c_char_p]),
    "fst_compose_frozen": (_u64, [_u64, _u64]),
    "fst_compose_frozen_shortest_path": (_u64, [_u64, _u64, _u32]),
    "fst_shortest_path": (_u64, [_u64, _u32]),
    "fst_compile_string": (_u64, [C.c_char_p, _u32]),
    "fst_print_string": (_i32, [_u64, C.c_char_p, _u32]),
    "fst_print_output_string": (_i32, [_u64, C.c_char_p, _u32]),
    "fst_teardown": (None, []),
    "fst_compose_frozen_shortest_path_batch": (
        C.c_int, [_u64, _P, _P, _u32, _u32, C.POINTER(FstBatchOptions), C.POINTER(FstBatchResult)]),
    "fst_batch_result_free": (None, [C.POINTER(FstBatchResult)]),
    "fst_compose_frozen_shortest_path_lhs_batch": (
        C.c_int, [_u64, C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstBatchResult)]),
    "fst_compose_frozen_shortest_path_handles_batch": (
        C.c_int, [_u64, _P, _u32, _u32, C.POINTER(FstBatchOptions), C.POINTER(FstBatchResult)]),
    "fst_pipeline_lhs_batch": (
        C.c_int, [_P, _u32, C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstBatchResult)]),
    "fst_normalize_lhs_batch": (
        C.c_int, [_P, _u32, C.POINTER(FstLhsBatch), C.POINTER(FstBatchOptions),
                  C.POINTER(FstTextResult)]),
    "fst_device_compose_shortest_path_lhs": (
        C.c_int, [_u64, C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstDeviceBatch), _P]),
    "fst_device_shortest_path_lhs": (
        C.c_int, [C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstDeviceBatch), _P]),
    "fst_device_compose_shortest_path": (
        C.c_int, [_u64, _P, _P, _u32, _u32, _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstDeviceBatch), _P]),
    "fst_compose_frozen_batch": (
        C.c_int, [_u64, _P, _P, _u32, _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstLatticeBatch)]),
    "fst_compose_frozen_lhs_batch": (
        C.c_int, [_u64, C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstLatticeBatch)]),
    "fst_lattice_batch_free": (None, [C.POINTER(FstLatticeBatch)]),
    "fst_connect_lhs_batch": (
        C.c_int, [C.POINTER(FstLhsBatch), C.POINTER(FstBatchOptions),
                  C.POINTER(FstLatticeBatch)]),
    "fst_prune_lhs_batch": (
        C.c_int, [C.POINTER(FstLhsBatch), _f64, C.POINTER(FstBatchOptions),
                  C.POINTER(FstLatticeBatch)]),
    "fst_device_prune_lhs": (
        C.c_int, [C.POINTER(FstLhsBatch), _f64, C.POINTER(FstBatchOptions),
                  C.POINTER(FstDeviceLattices), C.POINTER(_u64), _P]),
    "fst_posterior_lhs_batch": (
        C.c_int, [C.POINTER(FstLhsBatch), C.POINTER(FstBatchOptions),
                  C.POINTER(FstPosteriorResult)]),
    "fst_posterior_result_free": (None, [C.POINTER(FstPosteriorResult)]),
    "fst_device_posterior_lhs": (
        C.c_int, [C.POINTER(FstLhsBatch), C.POINTER(FstBatchOptions),
                  C.POINTER(FstDevicePosteriors), _P]),
    "fst_batch_result_path_costs": (C.c_int, [C.POINTER(FstBatchResult), _u32, _P, _u32, _P]),
    "fst_shortest_path_lhs_batch": (
        C.c_int, [C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstBatchResult)]),
    "fst_nbest_lhs_batch": (
        C.c_int, [C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstBatchResult)]),
    "fst_device_nbest_lhs": (
        C.c_int, [C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstDeviceBatch), _P]),
    "fst_nbest_unique_lhs_batch": (
        C.c_int, [C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstBatchResult)]),
    "fst_device_nbest_unique_lhs": (
        C.c_int, [C.POINTER(FstLhsBatch), _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstDeviceBatch), _P]),
    "fst_device_compose_frozen": (
        C.c_int, [_u64, _P, _P, _u32, _u32, _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstDeviceLattices), C.POINTER(_u64), _P]),
    "fst_device_prepare": (C.c_int, [_u64, _i32]),
    "fst_device_adopt_blob": (_u64, [_P, _u64, _i32, _P]),
    "fst_last_launch_stats": (C.c_int, [C.POINTER(FstLaunchStats)]),
    "fst_bench_transducer": (_u64, [_u32, _u32, _u32]),
    "fst_bench_transducer_wt": (_u64, [_u32, _u32, _u32, _u32]),
    "fst_batch_load": (_u64, [C.c_char_p]),
    "fst_batch_load_bytes": (_u64, [C.c_void_p, C.c_uint64]),
    "fst_weight_type": (C.c_int32, [_u64]),
    "fst_read_text": (_u64, [C.c_char_p]),
    "fst_chain_cost": (_f64, [_u64, _u64]),
    "fst_debug_coalescer_state": (C.c_int32, [C.c_int32, C.POINTER(_u32)]),
    "fst_load_att": (_u64, [C.c_char_p, _u32]),
    "fst_device_project_output": (C.c_int, [C.c_void_p, _u32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(_u32), C.c_void_p]),
    "fst_pipeline_batch": (C.c_int, [C.c_void_p, _u32, C.c_void_p, C.c_void_p, _u32, _u32,
                                     C.c_void_p, C.c_void_p]),
    "fst_normalize_text_batch": (C.c_int, [C.c_void_p, _u32, C.c_void_p, C.c_void_p, _u32,
                                           C.POINTER(FstBatchOptions), C.POINTER(FstTextResult)]),
    "fst_text_result_free": (None, [C.POINTER(FstTextResult)]),
    "fst_device_compile_text": (C.c_int, [C.c_void_p, C.c_void_p, _u32, C.c_void_p, C.c_void_p]),
    "fst_device_emit_text": (C.c_int, [C.POINTER(FstDeviceBatch), _u32, C.c_void_p, _u64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_u64),
                                       C.c_void_p]),
    "fst_batch_result_to_text": (C.c_int, [C.POINTER(FstBatchResult), C.POINTER(FstTextResult)]),
    "fst_normalize_text_aligned_batch": (
        C.c_int, [C.c_void_p, _u32, C.c_void_p, C.c_void_p, _u32, C.POINTER(FstBatchOptions),
                  C.POINTER(FstAlignedTextResult)]),
    "fst_aligned_text_result_free": (None, [C.POINTER(FstAlignedTextResult)]),
    "fst_device_path_alignment": (C.c_int, [C.POINTER(FstDeviceBatch), _u32, _P, _P, _P, _u64, _P,
                                            _P]),
    "fst_device_compose_alignment": (C.c_int, [_u32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _u64,
                                               _P]),
    "fst_batch_result_to_aligned_text": (C.c_int, [C.POINTER(FstBatchResult),
                                                   C.POINTER(FstAlignedTextResult)]),
    "fst_debug_text_compact": (_u64, [_u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "fst_debug_expand_weight_codes": (None, [C.c_void_p, _u64, C.c_void_p, C.c_void_p]),
    "fst_debug_stream_part_cuts": (_u32, [C.c_void_p, _u32, C.c_void_p, _u32, C.c_void_p]),
}

_lib = None


def lib():
    """Load libfst_amd.so (built by __graft_entry__.build()); raise if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it first (python -c 'import __graft_entry__ as g; "
                "g.build()'); libfst_amd has no CPU fallback")
        # One HIP runtime per process: torch ships its own libamdhip64 (same soname
        # libamdhip64.so.7, but torch links it by the bare name), so if this library
        # loaded /opt/rocm's copy first, a later `import torch` would bring a second
        # runtime and one of the two would see no device.  Loading torch first makes
        # our DT_NEEDED resolve to the copy torch already holds.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class MutableFst:
    """Owning wrapper of an FstMutableHandle (src/c-api.zig:437-503)."""

    def __init__(self, handle=None):
        self.h = lib().fst_mutable_new() if handle is None else handle
        if self.h == FST_INVALID_HANDLE:
            raise RuntimeError("invalid mutable handle")

    def __del__(self):
        if getattr(self, "h", FST_INVALID_HANDLE) != FST_INVALID_HANDLE and _lib is not None:
            _lib.fst_mutable_free(self.h)
            self.h = FST_INVALID_HANDLE

    def add_state(self):
        return lib().fst_mutable_add_state(self.h)

    def set_start(self, s):
        return lib().fst_mutable_set_start(self.h, s)

    def set_final(self, s, w):
        return lib().fst_mutable_set_final(self.h, s, w)

    def add_arc(self, src, il, ol, w, nxt):
        return lib().fst_mutable_add_arc(self.h, src, il, ol, w, nxt)

    @property
    def start(self):
        return lib().fst_mutable_start(self.h)

    @property
    def num_states(self):
        return lib().fst_mutable_num_states(self.h)

    def final_weight(self, s):
        return lib().fst_mutable_final_weight(self.h, s)

    def arcs(self, s):
        n = lib().fst_mutable_num_arcs(self.h, s)
        buf = (FstArc * max(n, 1))()
        m = lib().fst_mutable_get_arcs(self.h, s, buf, n)
        return [(buf[i].ilabel, buf[i].olabel, buf[i].weight, buf[i].nextstate) for i in range(m)]

    def freeze(self) -> "Fst":
        return Fst(lib().fst_freeze(self.h))

    def print_string(self, output_tape=False):
        buf = C.create_string_buffer(1 << 16)
        fn = lib().fst_print_output_string if output_tape else lib().fst_print_string
        n = fn(self.h, buf, len(buf))
        return None if n < 0 else buf.raw[:n]

    def to_lists(self):
        """(start, finals, arcs-per-state) for comparisons in tests."""
        ns = self.num_states
        return (self.start, [self.final_weight(s) for s in range(ns)],
                [self.arcs(s) for s in range(ns)])

    def to_arrays(self):
        """(start, offsets u64[ns + 1], arcs, finals f64[ns]) with `arcs` a numpy record
        array of FstArc {ilabel, olabel, weight, nextstate}: large results (config 1's
        lattice has 10 M arcs) without Python tuples."""
        L, ns = lib(), self.num_states
        cnt = np.fromiter((L.fst_mutable_num_arcs(self.h, s) for s in range(ns)), np.uint64, ns)
        off = np.zeros(ns + 1, np.uint64)
        np.cumsum(cnt, out=off[1:])
        tot = int(off[-1])
        buf = (FstArc * max(tot, 1))()
        base, sz, ptr = C.addressof(buf), C.sizeof(FstArc), C.POINTER(FstArc)
        for s in np.nonzero(cnt)[0]:
            L.fst_mutable_get_arcs(self.h, int(s), C.cast(base + int(off[s]) * sz, ptr), int(cnt[s]))
        dt = np.dtype([("il", "<u4"), ("ol", "<u4"), ("w", "<f8"), ("next", "<u4"), ("pad", "<u4")])
        arcs = np.frombuffer(buf, dtype=dt, count=tot).copy()
        fin = np.fromiter((L.fst_mutable_final_weight(self.h, s) for s in range(ns)), np.float64, ns)
        return self.start, off, arcs, fin

    @staticmethod
    def read_text(path) -> "MutableFst":
        """fst_read_text: OpenFst AT&T text (src/io/text.zig), labels as written."""
        h = lib().fst_read_text(os.fsencode(path))
        if h == FST_INVALID_HANDLE:
            raise ValueError(f"fst_read_text failed: {path}")
        return MutableFst(h)

    @staticmethod
    def compile_string(data: bytes) -> "MutableFst":
        return MutableFst(lib().fst_compile_string(data, len(data)))


class Fst:
    """Owning wrapper of an FstHandle (frozen FST)."""

    def __init__(self, handle):
        if handle == FST_INVALID_HANDLE:
            raise RuntimeError("invalid frozen handle")
        self.h = handle

    def __del__(self):
        if getattr(self, "h", FST_INVALID_HANDLE) != FST_INVALID_HANDLE and _lib is not None:
            _lib.fst_free(self.h)
            self.h = FST_INVALID_HANDLE

    @property
    def start(self):
        return lib().fst_start(self.h)

    @property
    def num_states(self):
        return lib().fst_num_states(self.h)

    def final_weight(self, s):
        return lib().fst_final_weight(self.h, s)

    def arcs(self, s):
        n = lib().fst_num_arcs(self.h, s)
        buf = (FstArc * max(n, 1))()
        m = lib().fst_get_arcs(self.h, s, buf, n)
        return [(buf[i].ilabel, buf[i].olabel, buf[i].weight, buf[i].nextstate) for i in range(m)]

    def save(self, path):
        return lib().fst_save(self.h, path.encode())

    @staticmethod
    def load(path) -> "Fst":
        return Fst(lib().fst_load(path.encode()))

    @staticmethod
    def load_any(path) -> "Fst":
        """Tropical or Log blob (fst_batch_load: weight type from the header)."""
        return Fst(lib().fst_batch_load(path.encode()))

    @staticmethod
    def load_att(path, shift_byte_labels=True) -> "Fst":
        """fst_load_att: AT&T text -> frozen, with att2lfst's +1 byte-label shift."""
        h = lib().fst_load_att(os.fsencode(path), 1 if shift_byte_labels else 0)
        if h == FST_INVALID_HANDLE:
            raise ValueError(f"fst_load_att failed: {path}")
        return Fst(h)

    @staticmethod
    def from_bytes(blob: bytes) -> "Fst":
        """Tropical or Log blob from memory (fst_batch_load_bytes)."""
        buf = C.create_string_buffer(blob, len(blob))
        return Fst(lib().fst_batch_load_bytes(C.cast(buf, C.c_void_p), len(blob)))

    @property
    def weight_type(self):
        return lib().fst_weight_type(self.h)

    @staticmethod
    def bench_transducer(kind, transducer_len, branches, weight_type=0) -> "Fst":
        return Fst(lib().fst_bench_transducer_wt(kind, transducer_len, branches, weight_type))

    def prepare(self, device=-1):
        rc = lib().fst_device_prepare(self.h, device)
        if rc != FST_OK:
            raise RuntimeError(f"fst_device_prepare failed: {rc}")


def compose_frozen_shortest_path(a: MutableFst, b: Fst, n: int = 1):
    """fst_compose_frozen_shortest_path (src/c-api.zig:744-811); None on FST_INVALID_HANDLE."""
    h = lib().fst_compose_frozen_shortest_path(a.h, b.h, n)
    return None if h == FST_INVALID_HANDLE else MutableFst(h)


def compose_frozen(a: MutableFst, b: Fst):
    h = lib().fst_compose_frozen(a.h, b.h)
    return None if h == FST_INVALID_HANDLE else MutableFst(h)


def shortest_path(a: MutableFst, n: int = 1):
    h = lib().fst_shortest_path(a.h, n)
    return None if h == FST_INVALID_HANDLE else MutableFst(h)


@dataclass
class BatchResult:
    status: np.ndarray
    offsets: np.ndarray
    ilabels: np.ndarray
    olabels: np.ndarray
    weights: np.ndarray
    finals: np.ndarray


def compose_frozen_shortest_path_batch(b: Fst, labels, offsets, n: int = 1,
                                       semantics: int = FST_SEM_LAZY, device: int = -1,
                                       devices=None, shards: int = 0) -> BatchResult:
    """Batched 1-best of many chain acceptors against one frozen rhs (fst_batch.h);
    `devices` / `shards`: cost-balanced shards over several GPUs (FST_BATCH_DEVICES)."""
    L = lib()
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    num = len(offsets) - 1
    opts = batch_options(device, semantics, devices, shards)
    res = FstBatchResult()
    rc = L.fst_compose_frozen_shortest_path_batch(b.h, labels.ctypes.data, offsets.ctypes.data,
                                                  num, n, C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_compose_frozen_shortest_path_batch failed: {rc}")
    return _take_result(res, num)


class LhsBatch:
    """N general lhs FSTs as one concatenated CSR (FstLhsBatch, fst_batch.h): word lattices,
    confusion networks, n-best unions.  State ids (start, nextstates) are local to each lhs;
    a state's arcs keep their order (it decides ties)."""

    def __init__(self, state_offsets, start, final_weights, arc_offsets, ilabels, olabels,
                 weights, nextstates):
        self.state_offsets = np.ascontiguousarray(state_offsets, dtype=np.uint64)
        self.start = np.ascontiguousarray(start, dtype=np.uint32)
        self.final_weights = np.ascontiguousarray(final_weights, dtype=np.float64)
        self.arc_offsets = np.ascontiguousarray(arc_offsets, dtype=np.uint64)
        self.ilabels = np.ascontiguousarray(ilabels, dtype=np.uint32)
        self.olabels = np.ascontiguousarray(olabels, dtype=np.uint32)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.nextstates = np.ascontiguousarray(nextstates, dtype=np.uint32)

    from_arrays = classmethod(lambda cls, *a, **k: cls(*a, **k))

    @classmethod
    def from_fsts(cls, fsts) -> "LhsBatch":
        """From a list of (start, finals, arcs): `start` a state id or None / FST_NO_STATE,
        `finals` one weight per state (inf: not final), `arcs` per state a list of
        (ilabel, olabel, weight, nextstate) -- MutableFst.to_lists()."""
        state_offsets, arc_offsets, start, fin = [0], [0], [], []
        il, ol, w, nx = [], [], [], []
        for st, finals, arcs in fsts:
            assert len(finals) == len(arcs)
            start.append(FST_NO_STATE if st is None else st)
            fin.extend(finals)
            for state_arcs in arcs:
                for a in state_arcs:
                    il.append(a[0])
                    ol.append(a[1])
                    w.append(a[2])
                    nx.append(a[3])
                arc_offsets.append(len(il))
            state_offsets.append(len(fin))
        return cls(state_offsets, start, fin, arc_offsets, il, ol, w, nx)

    def __len__(self):
        return len(self.start)

    def c_struct(self) -> FstLhsBatch:
        return FstLhsBatch(len(self.start), self.state_offsets.ctypes.data, self.start.ctypes.data,
                           self.final_weights.ctypes.data, self.arc_offsets.ctypes.data,
                           self.ilabels.ctypes.data, self.olabels.ctypes.data,
                           self.weights.ctypes.data, self.nextstates.ctypes.data)


def compose_frozen_shortest_path_lhs_batch(b: Fst, lhs: LhsBatch, n: int = 1,
                                           semantics: int = FST_SEM_LAZY, device: int = -1,
                                           devices=None, shards: int = 0) -> BatchResult:
    """Batched 1-best of many general lhs FSTs against one frozen rhs
    (fst_compose_frozen_shortest_path_lhs_batch): per item what the single call returns
    (lazy) or fst_shortest_path(fst_compose_frozen(a_i, b)) (eager), bit for bit."""
    opts = batch_options(device, semantics, devices, shards)
    res = FstBatchResult()
    cs = lhs.c_struct()
    rc = lib().fst_compose_frozen_shortest_path_lhs_batch(b.h, C.byref(cs), n, C.byref(opts),
                                                          C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_compose_frozen_shortest_path_lhs_batch failed: {rc}")
    return _take_result(res, len(lhs))


class _LatticeOwner:
    """Owns one FstLatticeBatch; fst_lattice_batch_free runs once no array views it."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            lib().fst_lattice_batch_free(C.byref(self.res))
        except Exception:  # interpreter shutdown
            pass


class LatticeBatch:
    """The result of compose_frozen_batch / compose_frozen_lhs_batch: N lattices in
    FstLhsBatch's layout as numpy views of the library's pinned arrays (no copy; the arrays
    keep the result alive), and one status per item."""

    def __init__(self, res: FstLatticeBatch):
        num, ns, na = int(res.fsts.num_fsts), int(res.total_states), int(res.total_arcs)
        owner = _LatticeOwner(res)
        self._owner = owner

        def arr(p, cnt, dt, ct):
            if cnt == 0:
                return np.zeros(0, dt)
            buf = (ct * cnt).from_address(C.cast(p, C.c_void_p).value)
            buf._owner = owner  # the view keeps the result alive
            return np.frombuffer(buf, dtype=dt)

        f = res.fsts
        self.status = arr(res.status, num, np.int32, C.c_int32)
        self.state_offsets = arr(f.state_offsets, num + 1, np.uint64, C.c_uint64)
        self.start = arr(f.start, num, np.uint32, C.c_uint32)
        self.final_weights = arr(f.final_weights, ns, np.float64, C.c_double)
        self.arc_offsets = arr(f.arc_offsets, ns + 1, np.uint64, C.c_uint64)
        self.ilabels = arr(f.ilabels, na, np.uint32, C.c_uint32)
        self.olabels = arr(f.olabels, na, np.uint32, C.c_uint32)
        self.weights = arr(f.weights, na, np.float64, C.c_double)
        self.nextstates = arr(f.nextstates, na, np.uint32, C.c_uint32)

    def __len__(self):
        return len(self.status)

    def as_lhs(self) -> LhsBatch:
        """An LhsBatch over the same memory (its arrays are these views, which keep the
        library's result alive): the input of every lhs batch entry."""
        return LhsBatch(self.state_offsets, self.start, self.final_weights, self.arc_offsets,
                        self.ilabels, self.olabels, self.weights, self.nextstates)

    def item(self, i):
        """(start, finals, arcs per state) of item i, as MutableFst.to_lists(); start is
        FST_NO_STATE for an item of zero states."""
        s0, s1 = int(self.state_offsets[i]), int(self.state_offsets[i + 1])
        ao = self.arc_offsets[s0:s1 + 1].astype(np.int64)
        arcs = []
        for s in range(s1 - s0):
            a, z = int(ao[s]), int(ao[s + 1])
            arcs.append(list(zip(self.ilabels[a:z].tolist(), self.olabels[a:z].tolist(),
                                 self.weights[a:z].tolist(), self.nextstates[a:z].tolist())))
        return int(self.start[i]), self.final_weights[s0:s1].tolist(), arcs


def _lattice_flags(project_output: bool, connect: bool) -> int:
    return ((FST_LATTICE_PROJECT_OUTPUT if project_output else 0) |
            (FST_LATTICE_CONNECT if connect else 0))


def compose_frozen_batch(b: Fst, labels, offsets, project_output: bool = False, device: int = -1,
                         devices=None, shards: int = 0, connect: bool = False) -> LatticeBatch:
    """fst_compose_frozen for a batch of chains (fst_compose_frozen_batch): item i is the
    lattice fst_compose_frozen(compile(labels of string i), b) returns, bit for bit; with
    `connect` (FST_LATTICE_CONNECT) its connect: the states that reach a final state."""
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    opts = batch_options(device, FST_SEM_LAZY, devices, shards)
    res = FstLatticeBatch()
    rc = lib().fst_compose_frozen_batch(b.h, labels.ctypes.data, offsets.ctypes.data,
                                        len(offsets) - 1,
                                        _lattice_flags(project_output, connect),
                                        C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_compose_frozen_batch failed: {rc}")
    return LatticeBatch(res)


def compose_frozen_lhs_batch(b: Fst, lhs: LhsBatch, project_output: bool = False,
                             device: int = -1, devices=None, shards: int = 0,
                             connect: bool = False) -> LatticeBatch:
    """The same for a batch of general lhs (fst_compose_frozen_lhs_batch)."""
    opts = batch_options(device, FST_SEM_LAZY, devices, shards)
    res = FstLatticeBatch()
    cs = lhs.c_struct()
    rc = lib().fst_compose_frozen_lhs_batch(b.h, C.byref(cs),
                                            _lattice_flags(project_output, connect),
                                            C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_compose_frozen_lhs_batch failed: {rc}")
    return LatticeBatch(res)


def connect_lhs_batch(lhs: LhsBatch, device: int = -1, devices=None,
                      shards: int = 0) -> LatticeBatch:
    """Connect (trim) of every item of an lhs batch (fst_connect_lhs_batch): the states that are
    reachable from the start and reach a final state, renumbered in their order; every item is
    FST_PATH_OK and NaN weights are copied."""
    opts = batch_options(device, FST_SEM_LAZY, devices, shards)
    res = FstLatticeBatch()
    cs = lhs.c_struct()
    rc = lib().fst_connect_lhs_batch(C.byref(cs), C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_connect_lhs_batch failed: {rc}")
    return LatticeBatch(res)


def prune_lhs_batch(lhs: LhsBatch, beam: float, device: int = -1, devices=None,
                    shards: int = 0) -> LatticeBatch:
    """Beam pruning of every item of an lhs batch (fst_prune_lhs_batch): the arcs and final
    weights on a complete path within `beam` of the item's best one, then connect.  Arc weights
    must be >= 0 (an item with a negative or NaN weight is FST_PATH_UNSUPPORTED and empty);
    beam = inf is connect on items of finite totals."""
    opts = batch_options(device, FST_SEM_LAZY, devices, shards)
    res = FstLatticeBatch()
    cs = lhs.c_struct()
    rc = lib().fst_prune_lhs_batch(C.byref(cs), float(beam), C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_prune_lhs_batch failed: {rc}")
    return LatticeBatch(res)


class _PosteriorOwner:
    """Owns one FstPosteriorResult; fst_posterior_result_free runs once no array views it."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            lib().fst_posterior_result_free(C.byref(self.res))
        except Exception:  # interpreter shutdown
            pass


class PosteriorResult:
    """The result of posterior_lhs_batch, as numpy views of the library's pinned arrays (no copy;
    the arrays keep the result alive): `status` and `total` (-log Z) per item, `alpha` and `beta`
    indexed like the batch's final_weights, `arc_cost` (the arc's -log posterior) like its
    weights.  Every entry of a non-OK item is +inf."""

    def __init__(self, res: FstPosteriorResult):
        num, ns, na = int(res.num_fsts), int(res.total_states), int(res.total_arcs)
        owner = _PosteriorOwner(res)
        self._owner = owner

        def arr(p, cnt, dt, ct):
            if cnt == 0:
                return np.zeros(0, dt)
            buf = (ct * cnt).from_address(C.cast(p, C.c_void_p).value)
            buf._owner = owner  # the view keeps the result alive
            return np.frombuffer(buf, dtype=dt)

        self.status = arr(res.status, num, np.int32, C.c_int32)
        self.total = arr(res.total, num, np.float64, C.c_double)
        self.alpha = arr(res.alpha, ns, np.float64, C.c_double)
        self.beta = arr(res.beta, ns, np.float64, C.c_double)
        self.arc_cost = arr(res.arc_cost, na, np.float64, C.c_double)

    def __len__(self):
        return len(self.status)


def posterior_lhs_batch(lhs: LhsBatch, device: int = -1, devices=None,
                        shards: int = 0) -> PosteriorResult:
    """Arc posteriors of every item of an lhs batch of acyclic items (fst_posterior_lhs_batch;
    the sums and their order are defined in fst_batch.h): forward and backward log-semiring
    sums, the total mass and every arc's -log posterior, in the batch's own layout."""
    opts = batch_options(device, FST_SEM_LAZY, devices, shards)
    res = FstPosteriorResult()
    cs = lhs.c_struct()
    rc = lib().fst_posterior_lhs_batch(C.byref(cs), C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_posterior_lhs_batch failed: {rc}")
    return PosteriorResult(res)


def batch_result_path_costs(result: "BatchResult", per: int, total) -> np.ndarray:
    """-log confidences of an n-best result (fst_batch_result_path_costs): `result` holds `per`
    strings per item, total[i] is item i's -log Z (PosteriorResult.total); out[i * per + k] is
    the k-th path's cost minus the total, +inf for a string that is not OK.  Runs without a GPU."""
    status = np.ascontiguousarray(result.status, dtype=np.int32)
    offsets = np.ascontiguousarray(result.offsets, dtype=np.uint64)
    ilabels = np.ascontiguousarray(result.ilabels, dtype=np.uint32)
    olabels = np.ascontiguousarray(result.olabels, dtype=np.uint32)
    weights = np.ascontiguousarray(result.weights, dtype=np.float64)
    finals = np.ascontiguousarray(result.finals, dtype=np.float64)
    total = np.ascontiguousarray(total, dtype=np.float64)

    def ptr(a, ct):
        return C.cast(a.ctypes.data, C.POINTER(ct))

    src = FstBatchResult(len(status), ptr(status, C.c_int32), ptr(offsets, C.c_uint64),
                         ptr(ilabels, C.c_uint32), ptr(olabels, C.c_uint32),
                         ptr(weights, C.c_double), ptr(finals, C.c_double),
                         int(offsets[-1]) if len(offsets) else 0)
    out = np.empty(max(len(status), 1), dtype=np.float64)
    rc = lib().fst_batch_result_path_costs(C.byref(src), int(per), total.ctypes.data, len(total),
                                           out.ctypes.data)
    if rc != FST_OK:
        raise RuntimeError(f"fst_batch_result_path_costs failed: {rc}")
    return out[:len(status)]


def shortest_path_lhs_batch(lhs: LhsBatch, n: int = 1, device: int = -1, devices=None,
                            shards: int = 0) -> BatchResult:
    """fst_shortest_path of every item of an lhs batch (fst_shortest_path_lhs_batch), with no
    compose: per item what the single call returns, bit for bit, as a status and a 1-best
    chain.  A non-OK item of a LatticeBatch owns no states and comes out EMPTY here: read the
    producer's status first."""
    opts = batch_options(device, FST_SEM_LAZY, devices, shards)
    res = FstBatchResult()
    cs = lhs.c_struct()
    rc = lib().fst_shortest_path_lhs_batch(C.byref(cs), n, C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_shortest_path_lhs_batch failed: {rc}")
    return _take_result(res, len(lhs))


def nbest_lhs_batch(lhs: LhsBatch, n: int, device: int = -1, devices=None,
                    shards: int = 0) -> BatchResult:
    """The n best distinct paths of every item of an lhs batch of acyclic items
    (fst_nbest_lhs_batch; the order is defined in fst_batch.h): a BatchResult of len(lhs) * n
    strings, item i's k-th best at i * n + k, EMPTY past the item's last path."""
    return _nbest("fst_nbest_lhs_batch", lhs, n, device, devices, shards)


def nbest_unique_lhs_batch(lhs: LhsBatch, n: int, device: int = -1, devices=None,
                           shards: int = 0) -> BatchResult:
    """The n best paths with pairwise different output texts (the non-epsilon olabels) of every
    item of an lhs batch of acyclic items (fst_nbest_unique_lhs_batch): nbest_lhs_batch's order
    with every path dropped that prints the text of an earlier one; the same layout."""
    return _nbest("fst_nbest_unique_lhs_batch", lhs, n, device, devices, shards)


def _nbest(entry, lhs, n, device, devices, shards):
    opts = batch_options(device, FST_SEM_LAZY, devices, shards)
    res = FstBatchResult()
    cs = lhs.c_struct()
    rc = getattr(lib(), entry)(C.byref(cs), n, C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"{entry} failed: {rc}")
    return _take_result(res, len(lhs) * n)


def pipeline_lhs_batch(stages, lhs: LhsBatch, n: int = 1, semantics: int = FST_SEM_LAZY,
                       devices=None, shards: int = 0, device: int = -1) -> BatchResult:
    """A pipeline on a general first stage (fst_pipeline_lhs_batch): stage 1 as
    compose_frozen_shortest_path_lhs_batch, every later stage on the previous stage's 1-best
    output tape as pipeline_batch; the last stage's paths."""
    stages = [stages] if isinstance(stages, Fst) else list(stages)
    hs = (C.c_uint64 * max(len(stages), 1))(*[s.h for s in stages])
    opts = batch_options(device, semantics, devices, shards)
    res = FstBatchResult()
    cs = lhs.c_struct()
    rc = lib().fst_pipeline_lhs_batch(hs, len(stages), C.byref(cs), n, C.byref(opts),
                                      C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_pipeline_lhs_batch failed: {rc}")
    return _take_result(res, len(lhs))


def normalize_lhs_batch(stages, lhs: LhsBatch, semantics: int = FST_SEM_LAZY, devices=None,
                        shards: int = 0, device: int = -1) -> TextResult:
    """Lattices in, text out (fst_normalize_lhs_batch): the same pipeline with the last
    stage's 1-best output tape printed on the device, as normalize_text_batch prints it."""
    stages = [stages] if isinstance(stages, Fst) else list(stages)
    hs = (C.c_uint64 * max(len(stages), 1))(*[s.h for s in stages])
    opts = batch_options(device, semantics, devices, shards)
    res = FstTextResult()
    cs = lhs.c_struct()
    rc = lib().fst_normalize_lhs_batch(hs, len(stages), C.byref(cs), C.byref(opts),
                                       C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_normalize_lhs_batch failed: {rc}")
    return _take_text(res)


def compose_frozen_shortest_path_handles_batch(b: Fst, fsts, n: int = 1,
                                               semantics: int = FST_SEM_LAZY, device: int = -1,
                                               devices=None, shards: int = 0) -> BatchResult:
    """The same from a list of MutableFst (each snapshotted under its lock)."""
    hs = (C.c_uint64 * max(len(fsts), 1))(*[f.h for f in fsts])
    opts = batch_options(device, semantics, devices, shards)
    res = FstBatchResult()
    rc = lib().fst_compose_frozen_shortest_path_handles_batch(b.h, hs, len(fsts), n,
                                                              C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_compose_frozen_shortest_path_handles_batch failed: {rc}")
    return _take_result(res, len(fsts))


def pipeline_batch(stages, labels, offsets, n: int = 1, semantics: int = FST_SEM_LAZY,
                   device: int = -1, devices=None, shards: int = 0) -> BatchResult:
    """Multi-stage batch (tagger -> verbalizer ...): each stage's 1-best output tape is the
    next stage's input, projected on the device (fst_pipeline_batch)."""
    L = lib()
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    num = len(offsets) - 1
    hs = (C.c_uint64 * len(stages))(*[s.h for s in stages])
    opts = batch_options(device, semantics, devices, shards)
    res = FstBatchResult()
    rc = L.fst_pipeline_batch(hs, len(stages), labels.ctypes.data, offsets.ctypes.data, num, n,
                              C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_pipeline_batch failed: {rc}")
    return _take_result(res, num)


class _ResultOwner:
    """Owns one FstBatchResult; fst_batch_result_free runs once no array views it."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            lib().fst_batch_result_free(C.byref(self.res))
        except Exception:  # interpreter shutdown
            pass


def _take_result(res, num) -> BatchResult:
    """Numpy views of the library's (pinned) result arrays, no copy: they stay valid while
    any of the arrays lives, then go back to the library's pool."""
    tot = int(res.total_arcs)
    owner = _ResultOwner(res)

    def arr(p, cnt, dt, ct):
        if cnt == 0:
            return np.zeros(0, dt)
        buf = (ct * cnt).from_address(C.cast(p, C.c_void_p).value)
        buf._owner = owner  # the view keeps the result alive
        return np.frombuffer(buf, dtype=dt)

    return BatchResult(status=arr(res.status, num, np.int32, C.c_int32),
                       offsets=arr(res.path_offsets, num + 1, np.uint64, C.c_uint64),
                       ilabels=arr(res.ilabels, tot, np.uint32, C.c_uint32),
                       olabels=arr(res.olabels, tot, np.uint32, C.c_uint32),
                       weights=arr(res.weights, tot, np.float64, C.c_double),
                       finals=arr(res.final_weights, num, np.float64, C.c_double))


@dataclass
class TextResult:
    status: np.ndarray
    offsets: np.ndarray
    text: np.ndarray
    total_weight: np.ndarray

    def texts(self):
        """One `bytes` per string (empty for every string that is not FST_PATH_OK)."""
        raw, off = self.text.tobytes(), self.offsets
        return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


class _TextOwner:
    """Owns one FstTextResult; fst_text_result_free runs once no array views it."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            lib().fst_text_result_free(C.byref(self.res))
        except Exception:  # interpreter shutdown
            pass


def _take_text(res) -> TextResult:
    num, tot = int(res.num_strings), int(res.total_bytes)
    owner = _TextOwner(res)

    def arr(p, cnt, dt, ct):
        if cnt == 0:
            return np.zeros(0, dt)
        buf = (ct * cnt).from_address(C.cast(p, C.c_void_p).value)
        buf._owner = owner  # the view keeps the result alive
        return np.frombuffer(buf, dtype=dt)

    return TextResult(status=arr(res.status, num, np.int32, C.c_int32),
                      offsets=arr(res.text_offsets, num + 1, np.uint64, C.c_uint64),
                      text=arr(res.text, tot, np.uint8, C.c_uint8),
                      total_weight=arr(res.total_weight, num, np.float64, C.c_double))


def text_csr(texts):
    """(uint8 array, uint64 offsets) of a list of `bytes`; a pair of arrays passes through."""
    if isinstance(texts, tuple):
        data, offsets = texts
        return (np.ascontiguousarray(data, dtype=np.uint8),
                np.ascontiguousarray(offsets, dtype=np.uint64))
    offsets = np.zeros(len(texts) + 1, np.uint64)
    if texts:
        np.cumsum([len(t) for t in texts], out=offsets[1:])
    return np.frombuffer(b"".join(texts), dtype=np.uint8), offsets


def normalize_text_batch(stages, texts, semantics: int = FST_SEM_LAZY, devices=None,
                         shards: int = 0, device: int = -1) -> TextResult:
    """Byte strings in, byte strings out (fst_normalize_text_batch): every string is compiled
    (label = byte + 1), run through `stages` (one Fst or a list: tagger -> verbalizer ...) and
    its 1-best output tape printed, all on the device.  `texts`: a list of `bytes`, or a
    (uint8 array, uint64 offsets) pair."""
    stages = [stages] if isinstance(stages, Fst) else list(stages)
    data, offsets = text_csr(texts)
    hs = (C.c_uint64 * max(len(stages), 1))(*[s.h for s in stages])
    opts = batch_options(device, semantics, devices, shards)
    res = FstTextResult()
    rc = lib().fst_normalize_text_batch(hs, len(stages), data.ctypes.data, offsets.ctypes.data,
                                        len(offsets) - 1, C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_normalize_text_batch failed: {rc}")
    return _take_text(res)


def batch_result_to_text(r: BatchResult) -> TextResult:
    """The host conversion of a label result (fst_batch_result_to_text): what
    normalize_text_batch returns for the same paths; runs without a GPU."""
    status = np.ascontiguousarray(r.status, dtype=np.int32)
    offsets = np.ascontiguousarray(r.offsets, dtype=np.uint64)
    ilabels = np.ascontiguousarray(r.ilabels, dtype=np.uint32)
    olabels = np.ascontiguousarray(r.olabels, dtype=np.uint32)
    weights = np.ascontiguousarray(r.weights, dtype=np.float64)
    finals = np.ascontiguousarray(r.finals, dtype=np.float64)

    def ptr(a, ct):
        return C.cast(a.ctypes.data, C.POINTER(ct))

    src = FstBatchResult(len(status), ptr(status, C.c_int32), ptr(offsets, C.c_uint64),
                         ptr(ilabels, C.c_uint32), ptr(olabels, C.c_uint32),
                         ptr(weights, C.c_double), ptr(finals, C.c_double),
                         int(offsets[-1]) if len(offsets) else 0)
    res = FstTextResult()
    rc = lib().fst_batch_result_to_text(C.byref(src), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_batch_result_to_text failed: {rc}")
    return _take_text(res)


@dataclass
class AlignedTextResult(TextResult):
    """TextResult plus, per output byte, the half-open interval [in_begin, in_end) of the
    string's own input bytes it came from (include/fst_batch.h, FstAlignedTextResult)."""
    in_begin: np.ndarray
    in_end: np.ndarray

    def spans(self, i):
        """String i as (in_lo, in_hi, out_lo, out_hi) segments, all relative to the string.
        Consecutive output bytes join one segment when they carry one and the same input
        interval (insertions at one boundary: in synthetic's cascade the five bytes of "seven"
        all carry the empty interval [1, 1) behind the "7", since they are emitted on
        input-epsilon arcs), or when they are copied text: one-byte intervals that advance
        with the output."""
        a, z = int(self.offsets[i]), int(self.offsets[i + 1])
        segs = []  # [in_lo, in_hi, out_lo, out_hi, kind]; kind None: one byte so far
        for j in range(a, z):
            b, e, o = int(self.in_begin[j]), int(self.in_end[j]), j - a
            if segs:
                s = segs[-1]
                if (b, e) == (s[0], s[1]) and s[4] in (None, "same"):
                    s[3], s[4] = o + 1, "same"
                    continue
                if (e == b + 1 and b == s[1] and s[1] - s[0] == s[3] - s[2]
                        and s[4] in (None, "copy")):
                    s[1], s[3], s[4] = e, o + 1, "copy"
                    continue
            segs.append([b, e, o, o + 1, None])
        return [tuple(s[:4]) for s in segs]


class _AlignedOwner:
    """Owns one FstAlignedTextResult; freed once no array views it."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            lib().fst_aligned_text_result_free(C.byref(self.res))
        except Exception:  # interpreter shutdown
            pass


def _take_aligned(res) -> AlignedTextResult:
    num, tot = int(res.num_strings), int(res.total_bytes)
    owner = _AlignedOwner(res)

    def arr(p, cnt, dt, ct):
        if cnt == 0:
            return np.zeros(0, dt)
        buf = (ct * cnt).from_address(C.cast(p, C.c_void_p).value)
        buf._owner = owner  # the view keeps the result alive
        return np.frombuffer(buf, dtype=dt)

    return AlignedTextResult(status=arr(res.status, num, np.int32, C.c_int32),
                             offsets=arr(res.text_offsets, num + 1, np.uint64, C.c_uint64),
                             text=arr(res.text, tot, np.uint8, C.c_uint8),
                             total_weight=arr(res.total_weight, num, np.float64, C.c_double),
                             in_begin=arr(res.in_begin, tot, np.uint32, C.c_uint32),
                             in_end=arr(res.in_end, tot, np.uint32, C.c_uint32))


def normalize_text_aligned_batch(stages, texts, semantics: int = FST_SEM_LAZY, devices=None,
                                 shards: int = 0, device: int = -1) -> AlignedTextResult:
    """normalize_text_batch plus the input span of every output byte
    (fst_normalize_text_aligned_batch): the same text, offsets, statuses and weights, and
    in_begin / in_end per output byte, computed on the device from every stage's 1-best path."""
    stages = [stages] if isinstance(stages, Fst) else list(stages)
    data, offsets = text_csr(texts)
    hs = (C.c_uint64 * max(len(stages), 1))(*[s.h for s in stages])
    opts = batch_options(device, semantics, devices, shards)
    res = FstAlignedTextResult()
    rc = lib().fst_normalize_text_aligned_batch(hs, len(stages), data.ctypes.data,
                                                offsets.ctypes.data, len(offsets) - 1,
                                                C.byref(opts), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_normalize_text_aligned_batch failed: {rc}")
    return _take_aligned(res)


def batch_result_to_aligned_text(r: BatchResult) -> AlignedTextResult:
    """The host conversion of a one-stage label result (fst_batch_result_to_aligned_text): what
    normalize_text_aligned_batch returns for the same paths; runs without a GPU."""
    status = np.ascontiguousarray(r.status, dtype=np.int32)
    offsets = np.ascontiguousarray(r.offsets, dtype=np.uint64)
    ilabels = np.ascontiguousarray(r.ilabels, dtype=np.uint32)
    olabels = np.ascontiguousarray(r.olabels, dtype=np.uint32)
    weights = np.ascontiguousarray(r.weights, dtype=np.float64)
    finals = np.ascontiguousarray(r.finals, dtype=np.float64)

    def ptr(a, ct):
        return C.cast(a.ctypes.data, C.POINTER(ct))

    src = FstBatchResult(len(status), ptr(status, C.c_int32), ptr(offsets, C.c_uint64),
                         ptr(ilabels, C.c_uint32), ptr(olabels, C.c_uint32),
                         ptr(weights, C.c_double), ptr(finals, C.c_double),
                         int(offsets[-1]) if len(offsets) else 0)
    res = FstAlignedTextResult()
    rc = lib().fst_batch_result_to_aligned_text(C.byref(src), C.byref(res))
    if rc != FST_OK:
        raise RuntimeError(f"fst_batch_result_to_aligned_text failed: {rc}")
    return _take_aligned(res)


def debug_text_compact(slots, nbytes, status, total_weight, text):
    """The streamed text route's host compaction (fst_debug_text_compact) on copies of the
    arrays: (offsets, status, total_weight, text, total bytes).  Runs without a GPU."""
    offsets = np.array(slots, dtype=np.uint64)
    nbytes = np.ascontiguousarray(nbytes, dtype=np.uint32)
    status = np.array(status, dtype=np.int32)
    total_weight = np.array(total_weight, dtype=np.float64)
    text = np.array(text, dtype=np.uint8)
    assert len(offsets) == len(status) + 1 == len(nbytes) + 1 == len(total_weight) + 1
    total = lib().fst_debug_text_compact(len(status), offsets.ctypes.data, nbytes.ctypes.data,
                                         status.ctypes.data, total_weight.ctypes.data,
                                         text.ctypes.data)
    return offsets, status, total_weight, text, int(total)


def debug_expand_weight_codes(codes, table, dst):
    """The streamed batch's host expander (fst_debug_expand_weight_codes): dst[i] =
    table[codes[i]], written in place into `dst` (a float64 array view of len(codes)
    elements, any 8-byte aligned start).  Runs without a GPU."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.float64)
    assert table.shape == (256,) and dst.dtype == np.float64 and dst.flags.c_contiguous
    assert dst.shape == codes.shape and dst.flags.writeable
    lib().fst_debug_expand_weight_codes(codes.ctypes.data, codes.size, table.ctypes.data,
                                        dst.ctypes.data)


def debug_stream_part_cuts(offsets, per_mille):
    """The streamed batch's part planner (fst_debug_stream_part_cuts): the string boundaries
    [0, .., num] of the parts of a shard with these label offsets, cut at these per-mille
    fractions of its labels.  Runs without a GPU."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    per_mille = np.ascontiguousarray(per_mille, dtype=np.uint64)
    cuts = np.zeros(per_mille.size + 2, dtype=np.uint32)
    n = lib().fst_debug_stream_part_cuts(offsets.ctypes.data, offsets.size - 1,
                                         per_mille.ctypes.data, per_mille.size, cuts.ctypes.data)
    return cuts[:n]


def coalescer_state(device: int = 0):
    """(leader slots in use, queued calls) of the single-call coalescer on `device`."""
    q = _u32(0)
    return int(lib().fst_debug_coalescer_state(device, C.byref(q))), int(q.value)


def last_launch_stats() -> FstLaunchStats:
    st = FstLaunchStats()
    lib().fst_last_launch_stats(C.byref(st))
    return st
