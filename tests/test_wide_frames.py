"""CPU: the pictures of tests/wide_frames.py hold what tests/test_gpu_wide_frames.py rests on.  Properties of inputs, shown with
the CPU oracle and tests/lf_model.py alone; nothing of the code under test runs here.

1. The frame's running alphabet maximum still rises at an LF group >= 65 (>= 193 too in the strips of 255): a prefix maximum
   that looks at the first stride of slots only would not pass.
2. The LF streams leave no slack that hides a misplaced slot: most bit counts behind slot 65 are no multiples of 32, and the
   slots' word counts differ.
3. Section byte lengths of every residue mod 4 occur among the groups of slots >= 65: words shared between two sections far
   into the payload.
4. Every group fits the token cap the GPU tests set — by its shape, whatever its content."""
import numpy as np
import pytest

import wide_frames as wf

STRIPS = [pytest.param(n, v, id=f"{n}{'v' if v else 'h'}") for n, v in wf.ONE_FRAME_STRIPS]


@pytest.mark.parametrize("n,vertical", STRIPS)
def test_strip_shapes(n, vertical):
    img = wf.strip(n, vertical)
    w, h = 2048 * (n - 1) + 8, 8
    assert img.shape == ((w, h, 3) if vertical else (h, w, 3)) and img.dtype == np.uint8 and not img.flags.writeable
    assert wf.lf_groups_of(img) == n
    slots = wf.strip_slots(n, vertical)
    assert [s.num_groups for s in slots] == [8] * (n - 1) + [1]
    for s in slots:  # eight populated places, then 56 empty ones, in every slot: empty places between all populated ones
        assert (s.bits[:s.num_groups] > 0).all() and not s.bits[s.num_groups:].any()
    if n > 129:
        return
    wide = wf.strip(255, vertical)  # a narrower strip is the start of the widest one, up to its own last, narrow LF group
    a, b = (img[:w - 8], wide[:w - 8]) if vertical else (img[:, :w - 8], wide[:, :w - 8])
    assert np.array_equal(a, b)


@pytest.mark.parametrize("n,vertical", STRIPS)
def test_the_running_maximum_rises_late(n, vertical):
    slots = wf.strip_slots(n, vertical)
    at = wf.rises(slots)
    print(f"  rises at {at}: {[slots[k].running_max for k in at]} after {slots[0].running_max}")
    assert any(k >= 65 for k in at), at
    if n == 255:
        assert any(k >= 193 for k in at), at
    run = [s.running_max for s in slots]
    assert run == list(np.maximum.accumulate(run))
    assert run[-1] > max(run[:64]), "a maximum over the first 64 slots would do"


@pytest.mark.parametrize("n,vertical", STRIPS)
def test_lf_streams_leave_no_slack(n, vertical):
    from tests import lf_model

    nbits = [int(lf_model.model(s.dc)[5]) for s in wf.strip_slots(n, vertical)]
    late = nbits[65:]
    unaligned = sum(1 for b in late if b % 32)
    print(f"  {unaligned} of {len(late)} slots >= 65 end inside a word; word counts {sorted({(b + 31) >> 5 for b in nbits})}")
    assert 2 * unaligned >= len(late)
    assert len({(b + 31) >> 5 for b in nbits}) > 1
    for s in wf.model_slots(n):  # what the GPU test compares byte by byte
        bits, nb = wf.lf_stream(n, vertical, s)
        assert nb == nbits[s] and len(bits) == (nb + 7) // 8


@pytest.mark.parametrize("n,vertical", STRIPS)
def test_section_lengths_of_every_residue_far_into_the_payload(n, vertical):
    slots = wf.strip_slots(n, vertical)
    mods = set()
    for s in slots[65:]:
        mods |= {int(b) % 4 for b in (s.bits[:s.num_groups] + 7) >> 3}
    assert mods == {0, 1, 2, 3}
    payload, bits, offs = wf.frame_sections(slots)
    assert len(bits) == len(offs) == 64 * n and int(offs[-1] + ((bits[-1] + 7) >> 3)) == len(payload)
    starts = {int(o) % 4 for o, b in zip(offs[65 * 64:], bits[65 * 64:]) if b}
    assert starts == {0, 1, 2, 3}, "sections behind slot 65 start at every place inside a word"


def test_every_group_fits_the_token_cap():
    """By shape: a group of at most 32 varblocks codes at most 32 x 3 x 64 symbols."""
    assert wf.GROUP_VARBLOCKS * wf.SYMBOLS_PER_VARBLOCK == 6144 <= wf.TOKEN_CAP and wf.TOKEN_CAP % 16 == 0
    shapes = [wf.strip(n, v).shape for n, v in wf.ONE_FRAME_STRIPS]
    shapes += [p.shape for p in wf.planner_strips()] + [p.shape for p in wf.planner_strips_f32()]
    shapes += [(h, w, 3) for w, h in wf.mixed_sizes()]
    shapes += [(8, 256, 3), (9, 33, 3), (8, 2056, 3), (8, 2048 * 4 + 8, 3), wf.tile_strip().shape, wf.tile_strip().shape[1::-1] + (3,)]
    shapes += [(8, 2048 * 127 + 8, 3), (8, 2048 * 255 + 8, 3)]  # the refused strips
    for h, w, _ in shapes:
        assert wf.varblocks_of_largest_group(w, h) <= wf.GROUP_VARBLOCKS, (w, h)
    # and the oracle's own counts for the widest strips
    for n, v in ((255, False), (255, True)):
        assert max(int(s.symbols.max()) for s in wf.strip_slots(n, v)) <= wf.GROUP_VARBLOCKS * wf.SYMBOLS_PER_VARBLOCK


def test_the_batches_pictures():
    sizes = wf.mixed_sizes()
    pics = wf.mixed_pictures()
    assert len(pics) == 255 and [p.shape for p in pics] == [(h, w, 3) for w, h in sizes]
    for w, h, count in ((256, 8, 255), (33, 9, 255)):
        g = wf.graded(w, h, count)
        assert len(g) == count and all(p.shape == (h, w, 3) for p in g)
        assert len({p.tobytes() for p in g}) == count, "the pictures of a batch are distinct"
    assert wf.tile_strip().shape == (8, 255 * 256 + 8, 3)


@pytest.mark.slow
def test_the_planner_strips_differ_in_their_final_running_maximum():
    strips = wf.planner_strips()
    assert [wf.lf_groups_of(s) for s in strips] == [28] * 9 + [3] and sum(wf.lf_groups_of(s) for s in strips) == wf.MAX_SLOTS
    final = [wf.oracle_slots(s)[-1].running_max for s in strips]
    print(f"  final running maxima, RGB8: {final}")
    assert len(set(final[:9])) >= 2
    # float: a strip whose tables are sized larger than 2^5 in front of one whose are not
    f32 = wf.planner_strips_f32()
    slots = [wf.oracle_slots(s) for s in f32]
    final = [s[-1].running_max for s in slots]
    logs = [[x.log_alphabet for x in s] for s in slots]
    print(f"  final running maxima, float: {final}")
    for k in range(10):
        if k in wf.WIDE_NOISE:
            at = wf.WIDE_NOISE[k]
            assert final[k] > 32 and all(v == 5 for v in logs[k][:at]) and all(v > 5 for v in logs[k][at:]), (k, logs[k])
        else:
            assert final[k] <= 32 and set(logs[k]) == {5}, (k, logs[k])
    assert all(k + 1 not in wf.WIDE_NOISE for k in wf.WIDE_NOISE), "a strip that stays below the floor follows each noisy one"
