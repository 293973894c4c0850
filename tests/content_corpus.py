"""The content the device-side file builders are held to the reference on (tests/test_gpu_builder_content.py on the GPU;
the layout hooks of test_mixed_sections.py, test_batch_layout.py and test_tiled_sections.py on the CPU): pictures that move
the builders' own data-dependent fields as far as pixels can, where the synthetic `photo` keeps them in the middle.

picture(name, w, h, depth, seed) maps a name to a host array, built on hydrium_amd/synth.py and variant_corpus.edge_image:

  black, white, ramp, noise, photo     synth's kinds at 8, 16 or 32 bit (32: make_image_f32, samples in [0, 1])
  basis_grey, basis_rg, primaries      variant_corpus's edge kinds at 8 or 16 bit (32: the 16-bit samples / 65535)
  extremes16                           ... 16 bit only
  float_photo                          make_image_f32("photo"), in [0, 1]
  float_neg                            make_image_f32("noise") * 2 - 0.5: negative samples and samples above 1
  float_wide                           make_image_f32("noise") * 40 - 3
  quadrants                            black | noise over primaries | photo; the split lies on a multiple of 256, so in tile
                                       mode neighbouring tiles are entirely different frames
  quadrants_black, noise_black,        pictures wider than one LF group (2048 columns): `quadrants` / noise / black in the
  black_noise                          first LF group, black / black / noise behind it

What the corpus reaches at the sizes of the lists below (asserted by tests/test_content_corpus.py, from the oracle; the
thresholds are hydk_toc_entry's size classes: 10 bits below 1024 bytes, 14 below 17408, 22 below 4211712):

  * every HF section 4 bytes, every TOC entry in the 10-bit class, one-symbol histograms: black 8x8, 520x264, 2048x16
  * 10-bit and 22-bit entries in one TOC: noise 520x264 u8 (sections of 115 .. 115980 bytes), quadrants 600x520 u8
    (16 .. 116846; as 256x256 tiles, frames of 4 .. 115974 HF bytes), extremes16 300x260 (591 .. 99782)
  * a file that is nearly all LF stream: primaries 264x200 u8 (two HF sections of 4 bytes in 2937 bytes)
  * token 28, the integer path's largest: basis_grey 256x256 u16
  * a running alphabet maximum of 72 with log_alphabet_size 7 (float_neg, float_wide) beside 5 (everything in [0, 1])
  * the smallest LF stream: bit_count 0 — black 8x8 at any depth: one block, three LF residuals of zero, a one-symbol
    code.  (Larger black pictures code run pairs: 24 bits at 2048x16, 153 at 520x264; white starts with a non-zero
    residual.)  An EMPTY LF piece between a frame's head and tail is therefore reachable from pixels, and a black 8x8
    frame stands in every list below: in each mixed batch, in a batch of its own shape between two noise frames, and as
    the last tile of black 520x264 in 256x256 tiles.
"""
import functools

import numpy as np

from variant_corpus import edge_image

SYNTH = ("black", "white", "ramp", "noise", "photo")
EDGE = ("basis_grey", "basis_rg", "primaries", "extremes16")
FLOAT = {"float_photo": ("photo", 1.0, 0.0), "float_neg": ("noise", 2.0, -0.5), "float_wide": ("noise", 40.0, -3.0)}
SPLIT = {"quadrants_black": ("quadrants", "black"), "noise_black": ("noise", "black"), "black_noise": ("black", "noise")}
NAMES = SYNTH + EDGE + tuple(FLOAT) + ("quadrants",) + tuple(SPLIT)
LF_GROUP = 2048

# hydk_toc_entry's size classes (bytes): [0, 1024) 10 bits, [1024, 17408) 14 bits, [17408, 4211712) 22 bits
TOC_10_BIT_END, TOC_14_BIT_END = 1024, 17408


def _split_at(n):
    """where a side of `quadrants` is cut: its middle, on a tile boundary where the side has one"""
    return (n // 2) // 256 * 256 or n // 2


def _make(name, w, h, depth, seed):
    from hydrium_amd import synth

    if name in FLOAT:
        if depth != 32:
            raise ValueError(f"{name} is float32 content")
        kind, scale, shift = FLOAT[name]
        img = synth.make_image_f32(kind, w, h, seed)
        return img if (scale, shift) == (1.0, 0.0) else (img * np.float32(scale) + np.float32(shift)).astype(np.float32)
    if name in SYNTH:
        return synth.make_image_f32(name, w, h, seed) if depth == 32 else synth.make_image(name, w, h, depth, seed)
    if name in EDGE:
        if name == "extremes16" and depth != 16:
            raise ValueError(f"{name} has no {depth}-bit form")
        if depth == 32:  # as make_image_f32: the 16-bit samples / 65535, in float32
            return (edge_image(name, w, h, 16).astype(np.float32) * np.float32(1.0 / 65535.0)).astype(np.float32)
        return edge_image(name, w, h, depth)
    if name == "quadrants":
        x, y = _split_at(w), _split_at(h)
        img = np.empty((h, w, 3), np.float32 if depth == 32 else np.uint16 if depth == 16 else np.uint8)
        img[:y, :x] = _make("black", x, y, depth, seed)
        img[:y, x:] = _make("noise", w - x, y, depth, seed)
        img[y:, :x] = _make("primaries", x, h - y, depth, seed)
        img[y:, x:] = _make("photo", w - x, h - y, depth, seed)
        return img
    if name in SPLIT:
        if w <= LF_GROUP:
            raise ValueError(f"{name} needs more than one LF group")
        first, second = SPLIT[name]
        return np.concatenate([_make(first, LF_GROUP, h, depth, seed), _make(second, w - LF_GROUP, h, depth, seed)], axis=1)
    raise ValueError(f"unknown corpus picture {name!r}")


@functools.lru_cache(maxsize=None)
def picture(name, w, h, depth=8, seed=1234):
    """(h, w, 3) uint8 / uint16 / float32, C-contiguous and read-only; made once"""
    img = np.ascontiguousarray(_make(name, w, h, depth, seed))
    assert img.shape == (h, w, 3) and img.dtype == {8: np.uint8, 16: np.uint16, 32: np.float32}[depth]
    img.setflags(write=False)
    return img


def quadrants(w, h, depth=8, seed=1234):
    return picture("quadrants", w, h, depth, seed)


# ---- the lists: (name, w, h, depth, seed) ------------------------------------------------------------------------------
def _p(name, w, h, depth, seed=1234):
    return (name, w, h, depth, seed)


# one mixed batch per sample format (hydamd_encode_mixed takes one format per call); each runs forward and reversed
MIXED = {
    8: [_p("black", 8, 8, 8), _p("noise", 520, 264, 8), _p("black", 520, 264, 8), _p("primaries", 264, 200, 8), _p("black", 2048, 16, 8),
        _p("ramp", 33, 9, 8)],
    16: [_p("white", 257, 256, 16), _p("basis_grey", 256, 256, 16), _p("black", 8, 8, 16), _p("extremes16", 300, 260, 16),
         _p("noise", 256, 256, 16)],
    32: [_p("float_neg", 264, 136, 32), _p("float_photo", 200, 120, 32), _p("black", 8, 8, 32), _p("float_wide", 264, 136, 32)],
}
# same-shape batches.  The middle frame of the float batch carries log_alphabet_size 5 between two frames of 7: a running
# alphabet that leaked from frame to frame would change its header.  The third shape has two LF groups, the second black;
# the last is the empty LF stream (black 8x8) between two frames of noise.
BATCH = [
    [_p("black", 520, 264, 8), _p("noise", 520, 264, 8), _p("primaries", 520, 264, 8), _p("photo", 520, 264, 8)],
    [_p("float_neg", 264, 136, 32), _p("float_photo", 264, 136, 32), _p("float_neg", 264, 136, 32, 1251)],
    [_p("quadrants_black", 2312, 264, 8), _p("quadrants_black", 2312, 264, 8, 1251)],
    [_p("noise", 8, 8, 8), _p("black", 8, 8, 8), _p("noise", 8, 8, 8, 1251)],
]
# tile mode: (picture, tile_size_shift_x, tile_size_shift_y)
TILED = [
    (_p("quadrants", 600, 520, 8), 0, 0),
    (_p("quadrants", 600, 520, 8), 1, 0),
    (_p("black", 520, 300, 16), 1, 0),
    (_p("black", 520, 264, 8), 0, 0),  # its last tile is black 8x8: the empty LF stream
]
# the frame assembler: two LF groups, one of noise and one of black, in either order
ASSEMBLER = [_p("noise_black", 2312, 264, 8), _p("black_noise", 2312, 264, 8)]


def one_group_pictures():
    """every picture of the lists that is one LF group, once"""
    seen = []
    for p in [p for lst in MIXED.values() for p in lst] + [p for lst in BATCH for p in lst] + [p for p, _, _ in TILED]:
        if p[1] <= LF_GROUP and p[2] <= LF_GROUP and p not in seen:
            seen.append(p)
    return seen


# ---- CPU: stage results of a picture, made once and shared by the CPU tests ----------------------------------------------
@functools.lru_cache(maxsize=None)
def stage(name, w, h, depth=8, seed=1234):
    """One-LF-group pictures: (oracle result, running alphabet maximum, lf_model.model's LF stream, frame.c's file for
    the picture alone: file header, one frame, is_last, both shifts -1).  Never changed."""
    import glue
    import lf_model
    from hydrium_amd import api
    from oracle import binding as orc

    assert w <= LF_GROUP and h <= LF_GROUP
    img = picture(name, w, h, depth, seed)
    p, isz = img.ctypes.data, img.dtype.itemsize
    r, mx = orc.encode_lf_group_ptrs([p, p + isz, p + 2 * isz], 3 * w, 3, orc.FMT[img.dtype], 0, w, h, 0, 1, 0)
    lf = lf_model.model(np.ascontiguousarray(r.dc, np.int32))
    md = api.HYDImageMetadata(w, h, 0, -1, -1)
    return r, mx, lf, glue.frame_from_stages(md, True, True, [(0, 0)], [r], mx, None, coded_lf=True)


def hf_section_bytes(r):
    """the sizes a frame's TOC carries for the HF sections of one oracle result"""
    return [(int(b) + 7) // 8 for b in r.group_bits]
