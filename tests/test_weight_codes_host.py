"""The host half of the streamed batch's weight codes (csrc/weight_codes.hpp, exported as
fst_debug_expand_weight_codes): one byte per arc becomes the arc's f64 weight through a
256-entry table, written with non-temporal stores where whole 64-B lines of the destination
allow.  No GPU: the export against numpy's table[codes], bit pattern for bit pattern, for
every length 0..200 at every destination offset 0..7 elements from a 64-B boundary, and the
elements around the destination untouched.
"""
import numpy as np
import pytest

from libfst_amd import fst as FF

GUARD = np.float64(-12345.5)


def tables():
    rng = np.random.default_rng(99)
    dyadic = rng.integers(0, 1 << 20, 256).astype(np.float64) * 2.0 ** -8   # scaled by 2^-8
    dyadic[0] = 0.0
    integer = np.arange(256, dtype=np.float64)                             # winv = 1
    nondyadic = np.zeros(256)                                               # an RK 4 / 5 table
    nondyadic[:200] = rng.random(200) * 10
    nondyadic[1:4] = [0.1, 1.0 / 3.0, np.log(3.0)]
    nondyadic[255] = np.log(3.0) / 7
    return {"integer": integer, "dyadic": dyadic, "nondyadic": nondyadic}


def aligned_f64(n_elems, offset):
    """A float64 view of n_elems elements that starts `offset` elements past a 64-B boundary,
    with 8 guard elements on both sides; returns (whole buffer, start index)."""
    raw = np.full(n_elems + 32, GUARD)
    start = (-(raw.ctypes.data // 8)) % 8 + 8 + offset
    assert (raw.ctypes.data + 8 * (start - offset)) % 64 == 0
    return raw, start


@pytest.mark.parametrize("name", ["integer", "dyadic", "nondyadic"])
def test_expand_matches_numpy_bits(name):
    table = tables()[name]
    rng = np.random.default_rng(7)
    for n in range(0, 201):
        codes = rng.integers(0, 256, n).astype(np.uint8)
        if n:
            codes[-1] = 255
            codes[0] = 0
        want = table[codes].view(np.uint64)
        for off in range(8):
            raw, s = aligned_f64(n, off)
            FF.debug_expand_weight_codes(codes, table, raw[s:s + n])
            assert np.array_equal(raw[s:s + n].view(np.uint64), want), (n, off)
            assert (raw[:s] == GUARD).all() and (raw[s + n:] == GUARD).all(), (n, off)


def test_every_code_and_unaligned_source():
    table = tables()["nondyadic"]
    codes = np.concatenate([np.arange(256), np.full(9, 255), np.arange(255, -1, -1)]).astype(np.uint8)
    for soff in range(8):
        c = codes[soff:]
        raw, s = aligned_f64(len(c), 3)
        FF.debug_expand_weight_codes(c, table, raw[s:s + len(c)])
        assert np.array_equal(raw[s:s + len(c)].view(np.uint64), table[c].view(np.uint64))
        assert (raw[:s] == GUARD).all() and (raw[s + len(c):] == GUARD).all()


def test_negative_zero_and_inf_bits_survive():
    # the table is copied bit for bit, whatever it holds
    table = np.zeros(256)
    table[1], table[2], table[255] = -0.0, np.inf, np.nextafter(0.0, 1.0)
    codes = np.tile(np.array([0, 1, 2, 255], np.uint8), 20)
    raw, s = aligned_f64(len(codes), 5)
    FF.debug_expand_weight_codes(codes, table, raw[s:s + len(codes)])
    assert np.array_equal(raw[s:s + len(codes)].view(np.uint64), table[codes].view(np.uint64))
