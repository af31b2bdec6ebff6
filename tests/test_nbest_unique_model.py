"""fst_nbest_unique_lhs_batch's definition (include/fst_batch.h), checked on the CPU alone: the
streaming recurrence (nbest_unique_model.nbest_unique, what the kernels compute) against the
declarative definition (nbest_unique_brute: every path in fst_nbest_lhs_batch's order, repeats of
a text dropped), and both against answers written by hand."""
import random

import pytest

import nbest_model as M
import nbest_unique_model as U

NS = (1, 2, 3, 5, 16)


def test_recurrence_equals_the_definition_on_random_items():
    rng = random.Random(20261021)
    differ = 0
    for _ in range(2000):
        item = U.random_item_dup(rng)
        for n in NS:
            got = U.nbest_unique(*item, n)
            want = U.nbest_unique_brute(*item, n)
            assert got == want, (item, n, got, want)
            assert isinstance(got, list) and len(got) <= n
            texts = [U.text_of(item[2], seq) for seq, _ in got]
            assert len(set(texts)) == len(texts), (item, n, got)
            differ += got != M.nbest(*item, n)
    # a condition on the inputs: the rule does change the answer on a good share of them
    # (31 % when this was written), or the comparison above would test nothing
    assert differ >= 0.2 * 2000 * len(NS), differ


def test_the_order_of_the_in_arcs_does_not_show():
    """The kernels fill a state's in-arcs in any order."""
    rng = random.Random(99)
    for _ in range(500):
        item = U.random_item_dup(rng)
        keys = {}
        order = lambda a: keys.setdefault(a, rng.random())
        for n in (1, 2, 3, 5):
            assert U.nbest_unique(*item, n, arc_order=order) == U.nbest_unique(*item, n), (item, n)


def test_n_1_is_the_plain_best_path():
    rng = random.Random(7)
    for _ in range(1000):
        item = U.random_item_dup(rng)
        assert U.nbest_unique(*item, 1) == M.nbest(*item, 1), item


def test_statuses_are_the_plain_entrys():
    for name, item, answers in M.KNOWN:
        for n, want in answers.items():
            if not isinstance(want, list):
                assert U.nbest_unique(*item, n) == want, (name, n)
                assert U.nbest_unique_brute(*item, n) == want, (name, n)


@pytest.mark.parametrize("name,item,answers", U.KNOWN_UNIQUE, ids=[k[0] for k in U.KNOWN_UNIQUE])
def test_known_answers(name, item, answers):
    for n, want in answers.items():
        assert U.nbest_unique(*item, n) == want, (name, n)
        assert U.nbest_unique_brute(*item, n) == want, (name, n)
