"""CPU: every claim of tests/entropy_corpus.py's docstring, from the oracle and tests/ans_model.py - and the negative
that the corpus exists for: none of the stage cases of test_gpu_device_parity.py reaches the excess loop or a 64-entry
table."""
import numpy as np
import pytest

import ans_model as am
import entropy_corpus as ec


def _excess(tags):
    return frozenset(t for t in tags if t.startswith("excess_"))


def test_the_lists_name_every_picture_once():
    assert len(set(ec.NAMES)) == len(ec.NAMES) == 26
    assert set(ec.EXCESS_CLAIMS) == set(ec.EXCESS)
    assert set(ec.ALPHABET_CLAIMS) == set(ec.LOG6 + ec.HANDOVER)
    assert set(ec.COUNT_CLAIMS) == set(ec.COUNTS)
    for name in ec.NAMES:
        img = ec.picture(name)
        assert img.dtype in (np.uint8, np.float32) and img.shape[0] * img.shape[1] <= 2048 * 200
        assert ec.lf_groups(name) == (2 if name in ec.HANDOVER else 1)


@pytest.mark.parametrize("name", ec.EXCESS)
def test_excess_pictures_take_their_branches_and_no_others(name):
    cluster, tags = ec.EXCESS_CLAIMS[name]
    (res,) = ec.stage(name)
    assert ec.picture(name).dtype == np.uint8 and res.log_alphabet_size == 5
    w = am.witness(res)
    for c, (hist, ntags, _) in w.items():
        assert _excess(ntags) == (tags if c == cluster else frozenset()), (name, c, hist, sorted(ntags))
    assert "floor_to_1" in w[cluster][1] and sum(w[cluster][0]) > 4096
    assert (cluster >= 3) == (name == "excess_coef")


def test_the_excess_histograms_are_the_ones_the_docstring_prints():
    hist = {name: am.witness(ec.stage(name)[0])[ec.EXCESS_CLAIMS[name][0]][0] for name in ec.EXCESS}
    assert hist["excess_at_0"] == [5115, 1, 1, 1, 1, 0, 1]
    assert hist["excess_partial"] == [5110, 1, 1, 1, 1, 0, 1, 0, 0, 5]
    assert hist["excess_skip"] == [5110, 1, 1, 1, 4, 0, 1, 0, 0, 1, 1]
    assert hist["excess_flatten"] == [6388, 1, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 4]
    assert hist["excess_coef"][:8] == [4762, 0, 0, 0, 1021, 0, 0, 1]
    # where the partial step lands: the frequency the oracle coded with is below the scaled count there, and only there
    for name, at in (("excess_at_0", 0), ("excess_partial", 9), ("excess_skip", 4), ("excess_flatten", 0), ("excess_coef", 4)):
        h, (res,) = hist[name], ec.stage(name)
        got = [int(v) for v in res.freqs[ec.EXCESS_CLAIMS[name][0]][:len(h)]]
        floor = [max(1, (v << 12) // sum(h)) if v else 0 for v in h]
        lower = [k for k in range(len(h)) if got[k] < floor[k]]
        assert lower == ([at, len(h) - 1] if name == "excess_flatten" else [at]), (name, lower)
    assert sum(am.witness(ec.stage("excess_coef")[0])[0][0]) == 352


@pytest.mark.parametrize("name", ec.LOG6 + ec.HANDOVER)
def test_alphabets_running_maxima_and_table_sizes(name):
    claims = ec.ALPHABET_CLAIMS[name]
    results = ec.stage(name)
    assert ec.is_float(name) and len(results) == len(claims)
    for res, (own, running, log_alpha) in zip(results, claims):
        assert int(res.alphabet_size[res.cluster_from:res.cluster_to].max()) == own
        assert (res.max_alphabet_size, res.log_alphabet_size) == (running, log_alpha) == (running, am.log_alphabet_size(running))
        tags = am.all_tags(res)
        assert ("n_eq_table" in tags) == (name in ec.N_EQ_TABLE), (name, sorted(tags))
        if name in ec.N_EQ_TABLE:
            assert own == 1 << log_alpha
        if name in ec.EMPTY_F0:
            assert "deficit_into_empty_f0" in tags
        assert not _excess(tags)


def test_handover_second_groups():
    """what the second LF group of each handover picture is there for"""
    _, black = ec.stage("log6_then_black")
    assert black.log_alphabet_size == 6 and black.num_symbols == 3
    w = am.witness(black)
    assert len(w) == 3 and all(h == [1] and "unique" in a for h, _, a in w.values())  # three one-symbol tables of 64 entries
    first, second = ec.stage("black_then_log6")
    assert am.all_tags(first) == {"exact", "unique"} and (first.log_alphabet_size, second.log_alphabet_size) == (5, 6)
    first, second = ec.stage("log7_then_log6")
    assert am.log_alphabet_size(int(second.alphabet_size.max())) == 6 and second.log_alphabet_size == 7
    for name in ec.HANDOVER:
        assert ec.picture(name).shape == (8, 2048 + 8, 3)
        assert [r.cluster_from for r in ec.stage(name)] == [0, 9]  # two presets, nine clusters each


@pytest.mark.parametrize("name", ec.COUNTS)
def test_group_symbol_counts(name):
    (res,) = ec.stage(name)
    assert res.group_symbols.tolist() == ec.COUNT_CLAIMS[name]
    assert ec.is_float(name) == name.startswith("f32_")
    assert ec.picture(name).shape[0] == 8 and res.log_alphabet_size == 5


def test_the_counts_sit_on_the_kernels_own_boundaries():
    single = sorted(c[0] for n, c in ec.COUNT_CLAIMS.items() if len(c) == 1 and not n.startswith("f32_"))
    assert single == [15, 16, 17, 63, 64, 65, 127, 128, 129]
    # 16: rounds of k_rans_lanes and flag words of k_rans_emit; 64, 128: chunks of k_rans_encode
    first, second = ec.COUNT_CLAIMS["n_128_then_3"]
    assert first % 64 == 0 and second == 3
    assert sorted(c[0] for n, c in ec.COUNT_CLAIMS.items() if n.startswith("f32_")) == [64, 65]


def test_no_older_stage_case_reaches_the_excess_loop_or_a_64_entry_table():
    """the gap: if a picture of test_gpu_device_parity.CASES ever carries an excess tag or log_alphabet_size 6, this fails and
    the corpus docstring (and DESIGN.md) are to be corrected"""
    import test_gpu_device_parity as parity
    from hydrium_amd import synth
    from oracle import binding as orc

    for kind, w, h, depth in parity.CASES:
        res, _ = orc.encode_lf_group(synth.make_image(kind, w, h, depth))
        assert res.log_alphabet_size == 5, (kind, w, h, depth)
        for c, (hist, ntags, _) in am.witness(res).items():
            assert not _excess(ntags), (kind, w, h, depth, c, hist)


@pytest.mark.parametrize("name", ec.NAMES)
def test_the_oracle_codes_every_corpus_picture_as_the_reference_does(ref_lib, name):
    """the oracle's own excess loop and 64-entry tables ran on no picture before either: its stages, wrapped by the host
    glue, are the compiled reference's file"""
    import glue
    from hydrium_amd import api

    img = ec.picture(name)
    assert bytes(glue.encode_with_oracle_stages(img, coded_lf=True)) == bytes(api.encode_image(ref_lib, img, out_buf_size=1 << 22))
