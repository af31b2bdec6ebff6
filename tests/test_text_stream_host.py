"""CPU tests of the streamed text route's host step (c_api.cpp text_compact, through its debug
symbol fst_debug_text_compact): the device leaves every string's bytes at the start of its
fixed slot (the string's own input byte range); the host closes the short slots up, moving
left in input order, and fills what a non-OK string reports.

Every case is compared with a restatement in plain Python.  The text buffer handed to the
library ends exactly at the last slot and is followed in the same allocation by guard bytes
the call must leave alone, and the values past the slots' used bytes are distinct from
every payload byte, so a byte read from the wrong place shows in the output."""
import math

import numpy as np
import pytest

import libfst_amd as F
from libfst_amd import fst as FF

OK, EMPTY, UNSUPPORTED, INTERNAL = (F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED,
                                    FF.FST_PATH_INTERNAL)
NOT_BYTES = 0xFFFFFFFF
GUARD = 64


def python_compact(slots, nbytes, status, total_weight, text):
    offsets, out = [], bytearray(text)
    status, tw = list(status), list(total_weight)
    dst = 0
    for i in range(len(status)):
        a, cap = int(slots[i]), int(slots[i + 1] - slots[i])
        offsets.append(dst)
        if status[i] == OK and nbytes[i] == NOT_BYTES:
            status[i] = UNSUPPORTED
        elif status[i] == OK and nbytes[i] > cap:
            status[i] = INTERNAL
        if status[i] != OK:
            tw[i] = math.inf
            continue
        chunk = bytes(out[a:a + int(nbytes[i])])
        out[dst:dst + len(chunk)] = chunk
        dst += len(chunk)
    offsets.append(dst)
    return offsets, status, tw, bytes(out), dst


def run_case(lens, nbytes, status, seed=0):
    """Slots of `lens` bytes; slot i starts with its payload (values 1..200, distinct per
    string) and ends with filler (201..255) the result must never contain."""
    rng = np.random.default_rng(seed)
    num = len(lens)
    slots = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(slots[-1])
    buf = np.full(total + GUARD, 0xEE, np.uint8)
    for i in range(num):
        a, z = int(slots[i]), int(slots[i + 1])
        buf[a:z] = rng.integers(201, 256, z - a)
        n = min(int(nbytes[i]), z - a) if nbytes[i] != NOT_BYTES else 0
        buf[a:a + n] = (np.arange(n) * 7 + i * 13) % 200 + 1
    tw = rng.random(num) + 1.0
    want = python_compact(slots, nbytes, status, tw, buf[:total].tobytes())
    # the library works on the first `total` bytes of a longer allocation
    offsets, st, w, text, tot = FF.debug_text_compact(slots, nbytes, status, tw, buf)
    assert tot == want[4] and int(offsets[-1]) == tot and int(offsets[0]) == 0
    assert [int(x) for x in offsets] == want[0]
    assert list(st) == want[1]
    assert np.array_equal(w.view(np.uint64), np.asarray(want[2], np.float64).view(np.uint64))
    assert text[:tot].tobytes() == want[3][:tot]
    assert np.all(text[total:] == 0xEE), "wrote past the last slot"
    # only payload bytes reach the result: nothing was read from a filler or the guard
    assert np.all((text[:tot] >= 1) & (text[:tot] <= 200))
    # non-OK strings: no bytes, +inf; OK strings keep their weight
    for i in range(num):
        if st[i] != OK:
            assert offsets[i + 1] == offsets[i] and w[i] == math.inf
        else:
            assert int(offsets[i + 1] - offsets[i]) == nbytes[i] and w[i] == tw[i]
    return offsets, st, w, text, tot


def test_all_slots_full_is_a_noop():
    lens = [5, 1, 64, 0, 7, 130]
    before = run_case(lens, lens, [OK] * len(lens))
    assert [int(x) for x in before[0]] == [0, 5, 6, 70, 70, 77, 207]


def test_short_slots_move_left():
    lens = [8, 8, 8, 70, 3, 9]
    nbytes = [8, 3, 8, 1, 3, 0]
    off, st, _, _, tot = run_case(lens, nbytes, [OK] * 6, seed=1)
    assert tot == 23 and [int(x) for x in off] == [0, 8, 11, 19, 20, 23, 23]


def test_zero_length_slots():
    lens = [0, 0, 4, 0, 5, 0]
    run_case(lens, [0, 0, 2, 0, 5, 0], [OK] * 6, seed=2)
    run_case([0, 0, 0], [0, 0, 0], [OK, EMPTY, OK], seed=3)


def test_non_ok_strings_drop_their_slots():
    lens = [6, 6, 6, 6, 6, 6, 6]
    nbytes = [6, 4, NOT_BYTES, 5, 6, 7, 2]       # (a count beyond its slot: INTERNAL)
    status = [OK, EMPTY, OK, F.FST_PATH_OVERFLOW, OK, OK, OK]
    off, st, w, _, tot = run_case(lens, nbytes, status, seed=4)
    assert list(st) == [OK, EMPTY, UNSUPPORTED, F.FST_PATH_OVERFLOW, OK, INTERNAL, OK]
    assert tot == 14 and [int(x) for x in off] == [0, 6, 6, 6, 6, 12, 12, 14]


def test_first_slot_short_and_first_slot_failed():
    run_case([9, 4, 4], [2, 4, 4], [OK] * 3, seed=5)
    run_case([9, 4, 4], [0, 4, 4], [OK] * 3, seed=6)
    run_case([9, 4, 4], [9, 4, 4], [EMPTY, OK, OK], seed=7)
    run_case([9, 4, 4], [NOT_BYTES, 4, 1], [OK, OK, OK], seed=8)


def test_no_strings():
    offsets, st, w, text, tot = FF.debug_text_compact([0], [], [], [], np.full(8, 0xEE, np.uint8))
    assert tot == 0 and list(offsets) == [0] and np.all(text == 0xEE)


@pytest.mark.parametrize("seed", range(4))
def test_random_batches(seed):
    rng = np.random.default_rng(100 + seed)
    num = 300
    lens = rng.integers(0, 20, num)
    nbytes = np.minimum(lens, rng.integers(0, 20, num)).astype(np.uint64)
    status = rng.choice([OK, OK, OK, EMPTY, F.FST_PATH_OVERFLOW], num)
    nbytes[rng.random(num) < 0.05] = NOT_BYTES
    run_case(lens, nbytes, status, seed=seed)
