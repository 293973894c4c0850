"""CPU: tests/ans_model.py, the branch-reporting restatement of the 12-bit normalisation and of the alias table, held to the
oracle (orc.normalize, orc.alias_slot) on every cluster of tests/entropy_corpus.py and on seeded random histograms.  The
model only witnesses what a picture reaches; this file is what entitles it to."""
import numpy as np
import pytest

import ans_model as am
import entropy_corpus as ec
from oracle import binding as orc


def _check_against_oracle(hist, log_alpha):
    """frequencies equal to orc.normalize; the slot of every (symbol, offset), all 4096 of them, equal to orc.alias_slot"""
    freq, unique, ntags = am.normalize(hist)
    want, want_unique = orc.normalize(hist)
    assert freq == [int(v) for v in want] and int(unique) == want_unique, hist
    slots, atags = am.slots(freq, log_alpha, unique)
    assert len(slots) == am.ANS_SLOTS
    f = np.ascontiguousarray(freq, np.uint32)  # orc.alias_slot's own call, without converting the list 4096 times
    fn, n = orc.lib().orc_alias_slot, len(freq)
    for (sym, off), slot in slots.items():
        assert fn(f.ctypes.data, n, log_alpha, int(unique), sym, off) == slot, (hist, log_alpha, sym, off)
    assert orc.alias_slot(freq, log_alpha, unique, len(freq) - 1, 0) == slots[(len(freq) - 1, 0)]
    return ntags, atags


def _random_histogram(rng, log_alpha):
    """alphabets of 1 .. 2^log_alpha; totals from a handful to far above 4096; zeros inside; one dominant count, many
    counts of 1 or a flat spread - the shapes that decide the branches"""
    n = 1 << log_alpha if rng.integers(0, 8) == 0 else int(rng.integers(1, (1 << log_alpha) + 1))  # one in eight fills the table
    shape = int(rng.integers(0, 7))
    if shape == 6:  # one symbol, the alphabet's last
        h = np.zeros(n, np.int64)
        h[-1] = int(rng.integers(1, 9000))
    elif shape == 5:  # token 0 dominant, counts of 1, and a last count that scales to little more than 1: flatten
        h = rng.integers(0, 2, n)
        h[0] = int(rng.integers(4097, 30000))
        h[-1] = int(rng.integers(2, 16))
    elif shape == 0:
        h = rng.integers(0, 50, n)
    elif shape == 1:
        h = rng.integers(0, 3, n)
        h[int(rng.integers(0, n))] += int(rng.integers(4000, 40000))
    elif shape == 2:
        h = (rng.integers(0, 2, n) * rng.integers(1, 100000, n))
    elif shape == 3:
        h = np.full(n, int(rng.integers(1, 400)))
    else:
        h = rng.integers(0, 4, n) * rng.integers(0, 2, n)
        h[int(rng.integers(0, n))] += int(rng.integers(4097, 9000))
        h[int(rng.integers(0, n))] += int(rng.integers(0, 12))
    h = [int(v) for v in h]
    h[-1] = max(h[-1], 1)
    return h


@pytest.mark.parametrize("log_alpha", [5, 6, 7])
def test_model_equals_oracle_on_random_histograms(log_alpha):
    rng = np.random.default_rng(4100 + log_alpha)
    seen = set()
    for _ in range(120):
        nt, at = _check_against_oracle(_random_histogram(rng, log_alpha), log_alpha)
        seen |= nt | at
    # the random shapes are there to reach every branch of both constructions
    assert seen >= {"floor_to_1", "zero_inside", "deficit", "deficit_into_empty_f0", "exact", "excess_partial", "excess_flatten",
                    "excess_skip", "excess_at_0", "unique", "over_to_under", "over_stays", "over_lands_exact",
                    "exact_bucket_initial", "pad_under", "n_eq_table"}, seen


@pytest.mark.parametrize("name", ec.NAMES)
def test_model_equals_oracle_on_every_cluster_of_the_corpus(name):
    for res in ec.stage(name):
        for c, h in am.histograms(res).items():
            freq, unique, _ = am.normalize(h)
            assert freq == [int(v) for v in res.freqs[c][:len(h)]], (name, c)  # what the oracle coded the picture with
            _check_against_oracle(h, res.log_alphabet_size)


def test_hand_made_histograms_take_the_branch_they_are_made_for():
    assert am.normalize([8190, 1, 0, 1])[2] >= {"excess_skip", "excess_partial", "excess_at_0", "floor_to_1", "zero_inside"}
    assert "excess_flatten" not in am.normalize([8190, 1, 0, 1])[2]
    f, _, t = am.normalize([20465, 0, 0, 1, 0, 1, 1, 12])
    assert t >= {"excess_flatten", "excess_skip", "excess_partial"} and f[-1] == 1
    assert am.normalize([0, 0, 3])[1] and am.normalize([0, 0, 3])[0] == [0, 0, 4096]
    assert "deficit_into_empty_f0" in am.normalize([0, 1, 1, 1])[2] and am.normalize([0, 1, 1, 1])[0][0] == 4096 - 3 * 1365
    assert am.normalize([1, 1])[2] == {"exact"}
    assert [am.log_alphabet_size(m) for m in (0, 1, 2, 31, 32, 33, 64, 65, 128)] == [5, 5, 5, 5, 5, 6, 6, 7, 7]
