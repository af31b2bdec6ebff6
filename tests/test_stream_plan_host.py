"""The streamed batch's part planner (csrc/stream_plan.hpp stream_part_cuts, exported as
fst_debug_stream_part_cuts): a shard's strings are cut into parts where its labels pass
per-mille fractions of their total.  No GPU: the export against a restatement with
np.searchsorted(..., side="right"), at the sizes where the plan changes (2^15 strings, 2^22
labels) and on the profiles where a cut is dropped.
"""
import numpy as np
import pytest

from libfst_amd import fst as FF

NUM = 1 << 15
TOTAL = 1 << 22
DEFAULT = [23, 163]                     # the f64 copy-out's cuts
ALL_CODED = [23, 163, 700, 900, 970]    # every part leaves codes


def offsets_of(lens, first=0):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64) \
        + np.uint64(first)


def restated(off, per_mille):
    num = len(off) - 1
    base, total = int(off[0]), int(off[num]) - int(off[0])
    cut = [0]
    if total >= TOTAL and num >= NUM:
        for f in per_mille:
            want = base + total * f // 1000
            i = int(np.searchsorted(off[:num], np.uint64(want), side="right"))
            if cut[-1] < i < num:
                cut.append(i)
    return cut + [num]


def check(off, per_mille):
    got = FF.debug_stream_part_cuts(off, per_mille).tolist()
    assert got == restated(off, per_mille)
    assert got[0] == 0 and got[-1] == len(off) - 1
    assert all(a < b for a, b in zip(got, got[1:]))
    return got


@pytest.mark.parametrize("per_mille", [DEFAULT, ALL_CODED])
def test_equal_lengths_at_the_threshold(per_mille):
    """Exactly 2^15 strings of 128 labels (2^22 in all) are cut; one string or one label
    fewer gives a single part."""
    lens = np.full(NUM, TOTAL // NUM)
    got = check(offsets_of(lens), per_mille)
    assert len(got) == len(per_mille) + 2
    # one string fewer, still 2^22 labels and more
    fewer = np.full(NUM - 1, TOTAL // NUM + 1)
    assert int(fewer.sum()) >= TOTAL
    assert check(offsets_of(fewer), per_mille) == [0, NUM - 1]
    # one label fewer, still 2^15 strings
    lens[-1] -= 1
    assert check(offsets_of(lens), per_mille) == [0, NUM]


def test_long_first_string_takes_the_first_cut():
    """A first string with more than 2.3 % of the labels: the first cut falls inside it and
    lands right behind it, on string 1 (no cut can land on string 0: part 0 is never
    empty); with more than 16.3 % both cuts land there and the second is dropped."""
    lens = np.full(NUM, 128)
    lens[0] = TOTAL // 20
    got = check(offsets_of(lens), DEFAULT)
    assert got[1] == 1 and len(got) == 4
    lens[0] = TOTAL // 2
    assert check(offsets_of(lens), DEFAULT) == [0, 1, NUM]


def test_two_cuts_on_one_string_keep_the_first():
    lens = np.full(NUM, 128)
    lens[100] = TOTAL // 3          # labels 0.3 % .. 25 %: both default cuts fall inside
    assert check(offsets_of(lens), DEFAULT) == [0, 101, NUM]
    got = check(offsets_of(lens), ALL_CODED)
    assert got[:2] == [0, 101] and len(got) == 6


def test_cut_on_the_string_count_is_dropped():
    lens = np.full(NUM, 128)
    lens[-1] = TOTAL // 10          # the last string starts before 97 % of the labels
    got = check(offsets_of(lens), ALL_CODED)
    assert len(got) == 6            # 23 .. 900 land before the last string, 970 on NUM
    assert check(offsets_of(lens), [999]) == [0, NUM]


def test_unsorted_and_empty_fractions():
    off = offsets_of(np.full(NUM, 128))
    assert check(off, []) == [0, NUM]
    got = check(off, [500, 100, 900])       # a cut behind the previous one is dropped
    assert len(got) == 4


def test_first_offset_not_zero():
    rng = np.random.default_rng(5)
    lens = rng.integers(64, 257, NUM)
    assert int(lens.sum()) >= TOTAL
    base = check(offsets_of(lens), ALL_CODED)
    for first in (1, 12345, 1 << 33):
        assert check(offsets_of(lens, first), ALL_CODED) == base


def test_random_length_profiles():
    rng = np.random.default_rng(2024)
    cut_some = 0
    for k in range(200):
        kind = k % 4
        if kind == 0:
            lens = rng.integers(100, 200, NUM)
        elif kind == 1:                       # many empty strings, a few long ones
            lens = np.where(rng.random(NUM) < 0.9, 0, rng.integers(0, 4000, NUM))
        elif kind == 2:                       # geometric
            lens = rng.geometric(1 / 140.0, NUM)
        else:                                 # around the thresholds
            lens = rng.integers(120, 137, NUM - int(rng.integers(0, 2)))
        per_mille = DEFAULT if k % 3 == 0 else ALL_CODED if k % 3 == 1 else \
            rng.integers(1, 1000, int(rng.integers(1, 8))).tolist()
        got = check(offsets_of(lens, int(rng.integers(0, 2)) * 777), per_mille)
        cut_some += len(got) > 2
    assert cut_some >= 100
