"""CPU: the content corpus (tests/content_corpus.py) contains the extremes it claims — asserted from the oracle's stage
results at the very sizes the builder tests use.  The thresholds are the format's own (hydk_toc_entry's size classes, the
alphabet sizes hydk_put_hf_config distinguishes), not measurements; what is measured is printed."""
import numpy as np
import pytest

import content_corpus as cc


@pytest.fixture(scope="module")
def stages():
    """{picture: (oracle result, running maximum, LF stream, frame.c's file)} of every one-LF-group picture of the lists"""
    return {p: cc.stage(*p) for p in cc.one_group_pictures()}


def _tile_results(p, sx, sy):
    """the oracle's result for every tile of a tiled case, raster order"""
    from hydrium_amd import api
    from oracle import binding as orc

    img = cc.picture(*p)
    h, w, _ = img.shape
    tw, th = api.tile_dims(w, h, sx, sy)
    isz = img.dtype.itemsize
    out = []
    for y0 in range(0, h, th):
        for x0 in range(0, w, tw):
            a = img.ctypes.data + (y0 * w + x0) * 3 * isz
            out.append(orc.encode_lf_group_ptrs([a, a + isz, a + 2 * isz], 3 * w, 3, orc.FMT[img.dtype], 0, min(tw, w - x0), min(th, h - y0),
                                                0, 1, 0)[0])
    return out


def test_every_name_at_every_depth_it_has():
    for name in cc.NAMES:
        depths = [32] if name in cc.FLOAT else [16] if name == "extremes16" else [8, 16, 32]
        w = 2100 if name in cc.SPLIT else 40
        for d in depths:
            img = cc.picture(name, w, 24, d)
            assert img.shape == (24, w, 3) and not img.flags.writeable
    with pytest.raises(ValueError):
        cc.picture("extremes16", 40, 24, 8)
    with pytest.raises(ValueError):
        cc.picture("float_neg", 40, 24, 8)
    assert cc.picture("float_neg", 64, 64, 32).min() < 0 < 1 < cc.picture("float_neg", 64, 64, 32).max()
    assert cc.picture("float_wide", 64, 64, 32).min() < -2 and cc.picture("float_wide", 64, 64, 32).max() > 30
    assert 0 <= cc.picture("float_photo", 64, 64, 32).min() and cc.picture("float_photo", 64, 64, 32).max() <= 1


def test_quadrants_are_what_they_are_called():
    q = cc.quadrants(600, 520, 8)
    assert not q[:256, :256].any()                                                 # black
    assert np.array_equal(q[:256, 256:], cc.picture("noise", 344, 256, 8))
    assert np.array_equal(q[256:, :256], cc.picture("primaries", 256, 264, 8))
    assert np.array_equal(q[256:, 256:], cc.picture("photo", 344, 264, 8))
    two = cc.picture("quadrants_black", 2312, 264, 8)
    assert np.array_equal(two[:, :2048], cc.quadrants(2048, 264, 8)) and not two[:, 2048:].any()
    assert not cc.picture("black_noise", 2312, 264, 8)[:, :2048].any() and not cc.picture("noise_black", 2312, 264, 8)[:, 2048:].any()


def test_the_corpus_reaches_the_toc_size_classes(stages):
    sizes = {p: cc.hf_section_bytes(r) for p, (r, _, _, _) in stages.items()}
    for p, s in sizes.items():
        print(p, "HF sections", min(s), "..", max(s), "bytes in", len(s), "groups; file", len(stages[p][3]), "bytes")
    tiny = [p for p, s in sizes.items() if max(s) < cc.TOC_10_BIT_END]
    assert any(len(sizes[p]) > 1 for p in tiny)           # ... in a frame that has a TOC
    for p in [p for lst in cc.MIXED.values() for p in lst if p[0] == "black"]:
        assert p in tiny and set(sizes[p]) == {4}, p    # every black picture: sections of 4 bytes
    both = [p for p, s in sizes.items() if min(s) < cc.TOC_10_BIT_END and max(s) >= cc.TOC_14_BIT_END]
    assert both, "no frame mixes the 10-bit and the 22-bit TOC class"
    assert ("noise", 520, 264, 8, 1234) in both
    # a file that is almost all LF stream: two HF sections of 4 bytes inside a file of some 3 KB
    r, _, lf, file = stages[("primaries", 264, 200, 8, 1234)]
    assert cc.hf_section_bytes(r) == [4, 4] and (lf[5] + 7) // 8 > len(file) * 3 // 4
    # tile mode: one picture whose frames are tiny and large
    tiles = [cc.hf_section_bytes(r) for r in _tile_results(*cc.TILED[0])]
    print("quadrants 600x520 u8, shift 0: HF bytes per tile frame", [sum(t) for t in tiles])
    assert min(map(sum, tiles)) < cc.TOC_10_BIT_END and max(map(sum, tiles)) >= cc.TOC_14_BIT_END
    whole = cc.hf_section_bytes(cc.stage("quadrants", 600, 520, 8)[0])
    print("quadrants 600x520 u8, one frame: HF sections", min(whole), "..", max(whole))
    assert min(whole) < cc.TOC_10_BIT_END and max(whole) >= cc.TOC_14_BIT_END


def test_the_corpus_reaches_both_alphabet_sizes_and_the_largest_integer_token(stages):
    for p, (r, mx, _, _) in stages.items():
        print(p, "running alphabet maximum", mx, "log_alphabet_size", r.log_alphabet_size, "largest token", int(r.symbols["token"].max()))
    for name in ("float_neg", "float_wide"):
        r, mx, _, _ = stages[(name, 264, 136, 32, 1234)]
        assert (mx, r.log_alphabet_size) == (72, 7), name
    for p, (r, mx, _, _) in stages.items():
        if p[0] not in ("float_neg", "float_wide"):
            assert mx <= 32 and r.log_alphabet_size == 5, p
    # the float batch: 5 between two frames of 7
    assert [stages[p][0].log_alphabet_size for p in cc.BATCH[1]] == [7, 5, 7]
    assert int(stages[("basis_grey", 256, 256, 16, 1234)][0].symbols["token"].max()) >= 28
    # one-symbol histograms: black's only cluster in use holds one symbol
    r = stages[("black", 520, 264, 8, 1234)][0]
    assert max(int(a) for a in r.alphabet_size[r.cluster_from:r.cluster_to]) <= 1


def test_the_smallest_lf_stream(stages):
    """bit_count 0 is reachable from pixels (the module docstring says which content gives it): that picture stands in
    every list, so every builder places an empty piece between a frame's head and its tail"""
    import lf_model

    counts = {p: lf[5] for p, (_, _, lf, _) in stages.items()}
    for p, n in sorted(counts.items(), key=lambda kv: kv[1])[:8]:
        print(p, "LF stream bit_count", n)
    empty = {p for p, n in counts.items() if n == 0}
    assert min(counts.values()) == 0 and all(p[:3] == ("black", 8, 8) for p in empty)
    for lst in cc.MIXED.values():
        assert any(p in empty for p in lst), lst
    assert any(lst[1] in empty for lst in cc.BATCH)
    tiles = [lf_model.model(np.ascontiguousarray(r.dc, np.int32))[5] for r in _tile_results(*cc.TILED[3])]
    print("black 520x264 u8 in 256x256 tiles: LF stream bit_counts", tiles)
    assert tiles[-1] == 0 and min(tiles[:-1]) > 0
