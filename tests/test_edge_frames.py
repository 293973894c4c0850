"""CPU: the frames of tests/edge_frames.py against the oracle they take their numbers from.

tests/test_gpu_buffer_edges.py sets HYDAMD_TOKEN_CAP and HYDAMD_PAYLOAD_CAP to exactly what these frames need, and to one
step less; what they need is n (the largest group's symbols), p (the symbols of the transform part that holds the noise
band) and B (the section bytes).  Here the helper's way to those numbers is checked without a device."""
import numpy as np
import pytest

import edge_frames as ef

CASES = sorted({(f, ef.band_plog(m)) for m, frames in ef.FRAMES.items() for f in frames})
SMALL = [c for c in CASES if not c[0].startswith("E")]


@pytest.mark.parametrize("gbh,plog,want", [(32, 2, [(0, 8), (8, 16), (16, 24), (24, 32)]), (32, 1, [(0, 16), (16, 32)]),
                                           (17, 2, [(0, 5), (5, 10), (10, 15), (15, 17)]), (17, 1, [(0, 9), (9, 17)]),
                                           (1, 2, [(0, 1), (1, 1), (1, 1), (1, 1)])])
def test_parts_are_ceil_gbh_over_parts_strips(gbh, plog, want):
    assert [ef.part_strips(gbh, plog, q) for q in range(1 << plog)] == want


def test_rounding_units():
    assert [ef.r16(x) for x in (0, 1, 16, 17)] == [0, 16, 16, 32]
    assert [ef.r32(x) for x in (0, 1, 32, 33)] == [0, 32, 32, 64]


@pytest.mark.parametrize("frame,plog", CASES, ids=[f"{f}-plog{p}" for f, p in CASES])
def test_black_blocks_and_part_counts_come_from_the_oracle(frame, plog):
    c = ef.case(frame, plog)
    res = c.res
    assert c.black_confirmed, "a block outside the band has non-zero coefficients in res.nz"
    # an all-black block is three symbols: the black-block formula for p and the cut of the symbol stream agree
    assert c.p == c.n - 3 * c.blocks_outside_part == c.parts[plog][c.g][c.part]
    _, _, _, _, gbw, gbh = ef.group_geometry(c.width, c.height, c.g)
    starts = ef.block_starts(res, c.g)
    sizes = np.diff(starts).reshape(gbh, gbw)
    band = np.zeros(gbh, bool)
    band[c.y0 // 8:-(-c.y1 // 8)] = True
    assert (sizes[~band] == 3).all() and (sizes[band] > 3).all()
    for pl in ef.PLOGS:
        for k in range(res.num_groups):
            assert sum(c.parts[pl][k]) == int(res.group_symbols[k])
    assert c.B == len(res.stream) == sum((int(b) + 7) // 8 for b in res.group_bits)
    assert c.n == c.largest_group()


@pytest.mark.parametrize("frame,plog", [k for k in CASES if "_" in k[0]], ids=lambda v: str(v))
def test_recorded_seeds_still_give_equality(frame, plog):
    c = ef.case(frame, plog)
    what, mod = ef.EQUALITY[frame.split("_")[1]]
    assert getattr(c, what) % mod == 0, (frame, what, getattr(c, what))
    assert (mod == 32) == (plog == 1)


@pytest.mark.parametrize("mode", list(ef.MODES))
def test_every_planned_cap_rests_on_the_oracle(mode):
    plog = ef.MODES[mode][1]
    for frame in ef.FRAMES[mode]:
        c = ef.case(frame, ef.band_plog(mode))
        assert ef.preconditions(mode, c) == [], (mode, frame)
        caps = {name: (tok, pay) for name, tok, pay, _ in ef.plan(mode, c)}
        exact, short = caps["tokens_exact"][0], caps["tokens_short"][0]
        if plog:
            room = exact >> plog
            assert exact % 64 == 0 and short == exact - 64 and room - (64 >> plog) < c.p <= room
            # the overflow of the short cap is the part's doing: the group as a whole still fits
            assert c.n <= (1 << plog) * (room - 16) and c.n <= short
            assert c.p > short >> plog
        else:
            assert exact - 16 < c.n <= exact and short == exact - 16 < c.n
            assert caps["payload_exact"] == (None, c.B) and caps["payload_short"] == (None, c.B - 1)
        if plog == 2:
            assert caps["tokens_16_mod_64"][0] % 64 == 16 and caps["tokens_16_mod_64"][0] >= c.n
        assert caps["tokens_and_payload_exact"] == (exact, c.B)
        # the frame itself fits what "exact" says, and does not fit what "short" says
        assert ef.fits(c.res, c.width, c.height, mode, exact, c.B)
        assert not ef.fits(c.res, c.width, c.height, mode, short, None)
        assert not ef.fits(c.res, c.width, c.height, mode, None if plog == 0 else exact, c.B - 1)
    equal = {"plog2": "p16", "plog1": "p32", "unsplit": "n16"}[mode]
    assert {f for f in ef.FRAMES[mode] if "_" in f} == {f"A_{equal}", f"C_{equal}"}


def test_neighbour_of_frame_a_holds_content():
    """One record written past group 0's array lands in group 1's: that must change bytes, so group 1 is no black group."""
    for plog in ef.PLOGS:
        c = ef.case("A", plog)
        assert c.res.num_groups == 2 and int(c.res.group_symbols[1]) > 1024 * 3
        assert min(np.diff(ef.block_starts(c.res, 1))) >= 3 and np.diff(ef.block_starts(c.res, 1)).mean() > 3


def test_frame_shapes_reach_what_they_are_for():
    a, b, cf, d, e = (ef.case(f, 2) for f in "ABCDE")
    assert (a.part, b.part, cf.part) == (0, 3, 1) and a.img.dtype == np.uint8 and b.img.dtype == np.uint16
    assert cf.img.dtype == np.float32 and cf.img.max() > 8 and cf.img.min() == 0 and cf.res.symbols["residue_bits"].max() >= 8
    # nothing of the float frame is near the edge of a 32-bit integer, where C leaves the conversion undefined
    assert np.abs(cf.res.quant).max() < 1 << 24 and np.abs(cf.res.dc).max() < 1 << 24 and np.isfinite(cf.res.dct).all()
    _, _, _, _, gbw, gbh = ef.group_geometry(d.width, d.height, 0)
    assert (gbw, gbh) == (32, 17) and [s1 - s0 for s0, s1 in (ef.part_strips(17, 2, q) for q in range(4))] == [5, 5, 5, 2]
    assert (d.y0, d.y1) == (120, 136) and ef.group_geometry(d.width, d.height, 1)[2] == 8
    assert e.res.num_groups == 64 and e.g == 63 and (e.y0, e.y1) == (192, 256) and ef.case("E", 1).y0 == 192 and ef.case("E", 1).p == e.p + 3 * 256
    assert (e.res.group_symbols[:63] == 3 * 1024).all()


def test_search_finds_the_recorded_seed_again():
    assert ef.search_seed("C_p32", 1, start=ef.SEEDS[("C_p32", 1)] - 3, tries=4) == ef.SEEDS[("C_p32", 1)]
