"""Pictures for tests/test_gpu_wide_frames.py and what the CPU oracle says about them; needs no GPU.

A context holds at most 255 LF-group slots, and a set of limits follows from that number (2040 pieces of the copy kernel,
255 frame sizes in one scan, the cluster map's schemes at 29, 86 and 128 LF groups, sums over 255 x 64 section sizes).  None
of it needs big pictures: an LF group may be 2048 x 8 pixels, so a frame of 255 LF groups is a strip of 520 200 x 8.

strip(n) is such a strip of n LF groups, the last one a single 8 x 8 group: a 4096 x 8 photo tiled along it plus noise
whose amplitude steps up with the LF-group index (NOISE_STEPS), so that the frame's running alphabet maximum still rises far
into the strip.  A horizontal strip has its 8 groups side by side in every LF group, a vertical one stacked; either way 56 of
a slot's 64 places are empty, and empty places lie between all populated ones.

tests/test_wide_frames.py holds the chosen pictures, with the oracle and tests/lf_model.py alone, to the conditions the GPU
tests rest on (late rises of the running maximum, LF streams that are no multiples of 32 bits, section byte lengths of every
residue mod 4 far into the payload, every group inside the token cap the GPU tests set)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hydrium_amd import synth  # noqa: E402
from oracle import binding as orc  # noqa: E402

LF = 2048
GROUPS_PER_LFG = 64
MAX_SLOTS = 255
TOKEN_CAP = 8192              # HYDAMD_TOKEN_CAP of the GPU tests: records per group
GROUP_VARBLOCKS = 32          # 256 x 8 or 8 x 256 pixels: the largest group of any picture here
SYMBOLS_PER_VARBLOCK = 3 * 64  # three channels of at most 64 symbols (a non-zero count and up to 63 coefficients)

# (first LF group, noise amplitude): the amplitude holds until the next step.  The photo alone has an alphabet maximum of 22
# and noise of an amplitude below about 28 adds nothing to it; 80 gives 23, 255 gives 25.  70 lies in 65...84, so that
# the strips of 85 and 86 LF groups see a late rise; 200 lies beyond 193 for the strips of 255.
NOISE_STEPS = ((0, 0), (20, 4), (45, 12), (70, 80), (110, 84), (150, 88), (200, 255))

ONE_FRAME_STRIPS = ((85, False), (86, False), (127, False), (129, False), (255, False), (255, True), (129, True))
MODEL_SLOTS = (0, 63, 64, 65, 128, 192)   # and n - 1: the slots whose LF streams are compared with tests/lf_model.py


def amplitude(lf_group):
    return [a for first, a in NOISE_STEPS if first <= lf_group][-1]


@functools.lru_cache(maxsize=None)
def _photo():
    return synth.make_image("photo", 2 * LF, 8, 8).astype(np.int16)


@functools.lru_cache(maxsize=None)
def strip_of_width(w, seed=1):
    """(8, w, 3) uint8, read-only: the tiled photo plus the stepped noise; column x belongs to LF group x // 2048"""
    base = _photo()
    img = np.tile(base, (1, -(-w // base.shape[1]), 1))[:, :w]
    amp = np.repeat(np.array([amplitude(i) for i in range(-(-w // LF))], np.int16), LF)[:w]
    rng = np.random.default_rng(seed)   # drawn column by column: a narrower strip is the start of a wider one
    noise = rng.integers(-128, 128, size=(w, 8, 3), dtype=np.int16).transpose(1, 0, 2) * amp[None, :, None] // 128
    out = np.ascontiguousarray(np.clip(img + noise, 0, 255).astype(np.uint8))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def strip(n, vertical=False):
    """RGB8 picture of n LF groups in a row, 2048 * (n - 1) + 8 by 8 pixels (transposed for vertical); read-only"""
    img = strip_of_width(LF * (n - 1) + 8)
    if vertical:
        img = np.ascontiguousarray(img.transpose(1, 0, 2))
        img.setflags(write=False)
    return img


def lf_groups_of(img):
    h, w, _ = img.shape
    return -(-w // LF) * -(-h // LF)


class Slot:
    """what the oracle says about one LF group of a frame"""

    def __init__(self, res, running):
        self.running_max = int(running)          # the frame's running alphabet maximum behind this LF group
        self.log_alphabet = int(res.log_alphabet_size)
        self.num_groups = int(res.num_groups)
        self.bits = np.zeros(GROUPS_PER_LFG, np.int64)
        self.bits[:self.num_groups] = res.group_bits
        self.stream = res.stream
        self.dc = res.dc
        self.symbols = res.group_symbols
        assert np.array_equal(res.group_offset, np.concatenate(([0], np.cumsum((res.group_bits + 7) >> 3)[:-1])))


def oracle_slots(img):
    """[Slot] of a one-frame image in send (raster) order, the running maximum carried as one frame's is"""
    img = np.ascontiguousarray(img)
    h, w, _ = img.shape
    lfx, lfy = -(-w // LF), -(-h // LF)
    out, mx = [], 0
    for ty in range(lfy):
        for tx in range(lfx):
            res, mx = orc.encode_lf_group(img, tx, ty, max_alphabet_size=mx)
            out.append(Slot(res, mx))
    return out


@functools.lru_cache(maxsize=None)
def strip_slots(n, vertical=False):
    return oracle_slots(strip(n, vertical))


def frame_sections(slots):
    """(payload, bits[64 * n], offsets[64 * n]): offsets are the running byte sum over ALL places, empty ones included"""
    bits = np.concatenate([s.bits for s in slots])
    nbytes = (bits + 7) >> 3
    offs = np.concatenate(([0], np.cumsum(nbytes)[:-1]))
    return b"".join(s.stream for s in slots), bits, offs


def rises(slots):
    """LF-group indexes at which the running maximum is larger than behind the LF group before"""
    run = [s.running_max for s in slots]
    return [k for k in range(1, len(run)) if run[k] > run[k - 1]]


@functools.lru_cache(maxsize=None)
def lf_stream(n, vertical, slot):
    """(bits as bytes, bit count) of tests/lf_model.py for one slot of a strip"""
    from tests import lf_model

    _, _, _, _, bits, nbits = lf_model.model(strip_slots(n, vertical)[slot].dc)
    return np.asarray(bits[:(nbits + 7) // 8], np.uint8), int(nbits)


def model_slots(n):
    return sorted({s for s in MODEL_SLOTS if s < n} | {n - 1})


# ---- pictures of the batches -------------------------------------------------------------------------------------------
def graded(w, h, count, seed=7):
    """`count` RGB8 pictures of one size whose content strength grows along the list (file sizes vary along a batch)"""
    base = synth.make_image("photo", max(w, 8), max(h, 8), 8)[:h, :w].astype(np.int16)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        noise = rng.integers(-128, 128, size=base.shape, dtype=np.int16) * np.int16(k // 2) // 128
        img = np.clip(np.roll(base, k, axis=1) + noise, 0, 255).astype(np.uint8)
        out.append(np.ascontiguousarray(img))
    return out


def mixed_sizes(count=MAX_SLOTS):
    """`count` distinct sizes, widths spread over 1...256 and heights over 1...8"""
    sizes = [(1 + (k * 37) % 256, 1 + k % 8) for k in range(count)]
    assert len(set(sizes)) == count and all(1 <= w <= 256 and 1 <= h <= 8 for w, h in sizes)
    assert {w for w, _ in sizes} >= {1, 256} and {h for _, h in sizes} == set(range(1, 9))
    return sizes


def mixed_pictures(count=MAX_SLOTS, seed=11):
    rng = np.random.default_rng(seed)
    src = strip_of_width(4 * LF + 256, seed=3)[:, 3 * LF // 2:]   # photo content, noise-free
    out = []
    for k, (w, h) in enumerate(mixed_sizes(count)):
        x0 = int(rng.integers(0, src.shape[1] - w))
        noise = rng.integers(-128, 128, size=(h, w, 3), dtype=np.int16) * np.int16(k // 3) // 128
        out.append(np.ascontiguousarray(np.clip(src[:h, x0:x0 + w].astype(np.int16) + noise, 0, 255).astype(np.uint8)))
    return out


@functools.lru_cache(maxsize=None)
def planner_strips():
    """nine strips of 28 LF groups and one of 3 (255 slots, the planner's largest case): every strip a window of the
    255-LF-group strip's content starting at another LF group, so that their final running maxima differ"""
    full = strip_of_width(LF * 254 + 8)
    out = []
    for k in range(9):
        x0 = LF * 27 * k
        out.append(np.ascontiguousarray(full[:, x0:x0 + LF * 27 + 8]))
    out.append(np.ascontiguousarray(full[:, LF * 250:LF * 252 + 8]))
    return tuple(out)


WIDE_NOISE = {1: 0, 4: 13, 6: 26}   # strip -> the LF group of it that holds noise beyond [0, 1]


@functools.lru_cache(maxsize=None)
def planner_strips_f32():
    """the same ten as float32 in [0, 1]; strips 1, 4 and 6 hold one LF group of noise spread over [-0.5, 1.5], whose
    alphabet maximum lies above 32, the table kernel's floor: from there on that strip's tables are sized larger, and a
    maximum carried into the next strip (which stays below 32 by itself) would change that strip's bytes"""
    rng = np.random.default_rng(5)
    out = []
    for k, img in enumerate(planner_strips()):
        f = img.astype(np.float32) / np.float32(255.0)
        if k in WIDE_NOISE:
            x0 = WIDE_NOISE[k] * LF
            f[:, x0:x0 + LF] = rng.random((8, LF, 3), dtype=np.float32) * np.float32(2.0) - np.float32(0.5)
        out.append(np.ascontiguousarray(f))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tile_strip():
    """65288 x 8: 256 tiles of 256 x 8, the last one 8 wide; tile k < 254 holds what LF group k of the 255-LF-group strip
    starts with, so the noise grows along the tiles and their frames differ in size; tile 254 is noise-free again"""
    full = strip_of_width(LF * 254 + 8)
    img = np.concatenate([full[:, k * LF:k * LF + 256] for k in range(254)] + [full[:, 100:356], full[:, 254 * LF:]], axis=1)
    assert img.shape == (8, 65288, 3)
    return np.ascontiguousarray(img)


def varblocks_of_largest_group(w, h):
    """varblocks of the largest group (256 x 256 pixels at most) of a w x h frame"""
    return -(-min(w, 256) // 8) * -(-min(h, 256) // 8)
