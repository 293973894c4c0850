"""CPU: the crafted residual streams of tests/lf_streams.py.  Each is what it claims to be (the inversion of the predictor
gives LF ints whose residuals are the wanted stream; the property the case exists for holds in the model's output), and the
two references the GPU tests use agree on it: the numpy model's stream spliced by the host equals the serial host coder's
LFGroup section, byte for byte."""
import numpy as np
import pytest

from tests import lf_model, lf_streams as ls


@pytest.mark.parametrize("case", ls.CASES, ids=[c.name for c in ls.CASES])
def test_crafted_stream(case):
    v, dc = case.stream(), case.lf_ints()
    assert dc.shape == (3, case.vbh, case.vbw) and dc.dtype == np.int32
    np.testing.assert_array_equal(lf_model.residuals(dc), v)
    assert case.holds(), "the stream does not have the property it was made for"
    _, lengths, alphabet, pairs, bits, nbits = lf_model.model(dc)
    assert lf_model.coded_lf_group(case.vbw, case.vbh, lengths, alphabet, pairs, bits, nbits) == lf_model.host_lf_group(dc)


def test_the_background_has_no_runs():
    v = ls.background(5000)
    assert (v[1:] != v[:-1]).all()
    lit, r = lf_model.emissions(v)
    assert lit.all() and not r.any()


def test_stream_lengths_cover_every_remainder_of_four():
    """a thread owns four consecutive values: the stream's last thread holds 1, 2, 3 or 4 of them"""
    assert {3 * w * h % 4 for w, h in ls.C_SHAPES} == {0, 1, 2, 3}
    assert all(c.n == 3 * c.vbw * c.vbh for c in ls.CASES)


def test_plane_boundaries_fall_inside_a_thread():
    assert all((w * h) % 4 != 0 for w, h in ls.D_SHAPES)


def test_families_have_their_cases():
    count = {}
    for c in ls.CASES:
        count[c.family] = count.get(c.family, 0) + 1
    assert count == {"a": 44, "b": 24, "c": 55, "d": 8, "e": 46, "f": 12, "g": 1}, count
    for f in ls.FRAMES:
        assert 2 <= len(f.slots) <= 4 and all(s.name in ls.BY_NAME for s in f.slots)
    assert {len(f.slots) for f in ls.FRAMES} >= {3, 4}
    assert ls.FRAMES[2].slots[1].n == 3 and ls.TWICE[0].n == 3 * 256 * 256 and ls.TWICE[1].n == 6


def test_longest_string_lands_on_every_wanted_bit():
    for pos in (ls.WINDOW - 1, ls.WINDOW):
        offs = set(ls._fib_rotations(pos))
        assert {0, 31} <= offs and any(o >= 6 for o in offs)
