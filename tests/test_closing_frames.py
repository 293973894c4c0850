"""CPU: what the oracle says about the frames of tests/closing_frames.py, so that the GPU test's premises are checked and not
only stated.

The emit launch that places its own sections stores a word that sections share as byte stores, so the frames must hold
section byte lengths of every residue mod 4 and shared words of every split.  The claim that no picture puts more than two
sections into one 32-bit word rests on two facts, both asserted here over every frame of the set: a populated group's section is
never shorter than the four bytes of its rANS final state, and a place with g >= ngroups has no bytes at all.  With every
non-empty section at least a word long, a word holds at most the end of one and the start of the next; the case of up to four
writers of one word, which no picture reaches, is held to account in tests/test_closing_edges.py."""
import numpy as np
import pytest

import closing_frames as cf


@pytest.fixture(scope="module")
def frame_bits():
    """name -> (section bit counts, populated groups per slot), the oracle alone"""
    out = {}
    makers = dict(cf.FRAMES)
    makers.update({f"batch_{k}": f for k, f in enumerate(cf.BATCH)})
    makers["black_512"] = lambda: np.zeros((512, 512, 3), np.uint8)   # nothing to code: the shortest populated sections
    for name, make in makers.items():
        img = make()
        _, bits, _ = cf.oracle_frame(img)
        h, w, _ = img.shape
        populated = []
        for ty in range(-(-h // 2048)):
            for tx in range(-(-w // 2048)):
                gw, gh = min(2048, w - tx * 2048), min(2048, h - ty * 2048)
                populated.append(-(-gw // 256) * -(-gh // 256))
        out[name] = (bits, populated)
    return out


def test_a_populated_section_is_never_shorter_than_a_word(frame_bits):
    for name, (bits, populated) in frame_bits.items():
        nbytes = (np.asarray(bits, np.int64) + 7) >> 3
        for slot, n in enumerate(populated):
            sl = nbytes[slot * cf.GROUPS_PER_LFG:(slot + 1) * cf.GROUPS_PER_LFG]
            print(f"  {name} slot {slot}: {n} groups, shortest section {int(sl[:n].min())} bytes")
            assert (sl[:n] >= 4).all(), f"{name} slot {slot}: a populated group's section is shorter than its final state"
            assert not sl[n:].any(), f"{name} slot {slot}: a place with g >= ngroups has bytes"
        assert int(nbytes[nbytes > 0].min()) >= 4


def test_at_most_two_sections_meet_in_a_word(frame_bits):
    mods, splits = set(), set()
    for name, (bits, _) in frame_bits.items():
        m, s, most = cf.section_facts(bits)
        mods |= m
        splits |= s
        assert most <= 2, f"{name}: {most} sections in one word"
    assert {1, 2, 3} <= mods, f"no section of every byte length mod 4: {sorted(mods)}"
    assert {(1, 3), (2, 2), (3, 1)} <= splits, f"shared words of every split are not all there: {sorted(splits)}"
