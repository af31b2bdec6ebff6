"""fst_nbest_lhs_batch's definition (include/fst_batch.h), checked on the CPU alone: the
recurrence (nbest_model.nbest, what the kernels compute) against the declarative definition
(nbest_model.nbest_brute: every path, sorted with the recursive comparator), and both against
answers written by hand."""
import random

import pytest

import nbest_model as M

NS = (1, 2, 3, 5, 16)


def test_recurrence_equals_the_definition_on_random_items():
    rng = random.Random(20261021)
    short = full = 0
    for _ in range(2000):
        item = M.random_item(rng)
        for n in NS:
            got = M.nbest(*item, n)
            want = M.nbest_brute(*item, n)
            assert got == want, (item, n, got, want)
            assert isinstance(got, list) and len(got) <= n
            if len(got) < n:
                short += 1
            else:
                full += 1
    cases = short + full
    assert cases == 2000 * len(NS)
    # both kinds are well represented: items with fewer than n paths, and with at least n
    assert short >= 0.2 * cases and full >= 0.2 * cases, (short, full)


@pytest.mark.parametrize("name,item,answers", M.KNOWN, ids=[k[0] for k in M.KNOWN])
def test_known_answers(name, item, answers):
    for n, want in answers.items():
        assert M.nbest(*item, n) == want, (name, n)
        assert M.nbest_brute(*item, n) == want, (name, n)
