"""One table of named RGB pixel layouts, for the tests that hold the transform kernel's pixel loaders and the host's origin
arithmetic to the oracle (test_pixel_layouts.py on the CPU, test_gpu_pixel_layouts.py on the device).  Data and helpers
only: no tests, no GPU.

build(name, picture, filler) lays a contiguous (H, W, 3) picture of 1-, 2- or 4-byte samples out in a flat byte buffer and
says where its three channels start and how far apart rows and pixels are, as the device API takes them.  Every byte of the
buffer that is no sample of the picture holds `filler`: with 0xFF that is 255, 65535 or a NaN (float32, float16 and
bfloat16 alike), so a loader that reads a byte outside the picture changes the output or fails with "Invalid NaN Float";
with 0 it reads what a cleared allocation holds.  MARGIN bytes of filler lie before the first and behind the last sample
(no picture starts or ends an allocation), and the builder assumes that the buffer's base is a multiple of 256 — what a
device allocator gives; the GPU tests assert it before they add the offsets.

loader(sample_fmt, channel_addresses, row_stride, pixel_stride) restates which loader k_transform_tokenize picks for a
layout (hydrium_amd/csrc/hip/k1_transform_body.h, from `const bool packed` to `hfast`).  The kernel decides from address bits, not
from anything the API names; the two are changed together.
"""
import numpy as np

MARGIN = 256  # bytes of filler before and behind; a multiple of 256, so the first sample keeps the base's alignment
SAMPLE_BYTES = {0: 1, 1: 2, 2: 4, 3: 2, 4: 2}  # by sample format: uint8, uint16, float32, float16, bfloat16
TYPES = {"u8": 0, "u16": 1, "f32": 2, "f16": 3, "bf16": 4}
LOADERS = ("packed", "half run", "half planes", "per sample")
# the shapes of the GPU matrix (width, height), all one LF group: two groups across (px0 = 256) of whole blocks; ragged by
# 7; a second group that is a single ragged one-pixel block column; the smallest whole block.  Heights that are no multiple
# of 8 exercise row_ok.
SHAPES = [(264, 40), (263, 41), (257, 9), (8, 8)]

_BASE_K = {1: (1, 2, 3), 2: (2,), 4: (4,)}  # every sample-aligned residue of 4 (float32: 4 itself, still a dword's)


def layout_names(sample_bytes):
    """the table's names for a sample size, in a fixed order"""
    return (["interleaved"] + [f"interleaved, base + {k} bytes" for k in _BASE_K[sample_bytes]] +
            ["padded pitch, dword rows", "padded pitch, odd rows", "negative pitch, dword rows", "negative pitch, odd rows",
             "bgr", "rgba", "crop", "planes", "planes, odd pitch", "planes in B, G, R order", "planes, negative pitch"])


def _dword_pitch(samples, s):
    """the smallest row stride (in samples) above `samples` whose bytes are a multiple of 4"""
    return (samples * s + 4) // 4 * 4 // s if s < 4 else samples + 1


def _odd_pitch(samples, s):
    """a row stride above `samples` whose bytes are no multiple of 4 (float32: an odd number of samples)"""
    if s == 1:
        return _dword_pitch(samples, 1) + 1
    return samples + 1 + samples % 2


def _spec(name, w, h, s):
    """(buffer bytes, byte offsets of the three channels' first samples, row_stride, pixel_stride), strides in samples"""
    tight = 3 * w
    if name.startswith("planes"):
        pitch = {"planes": w, "planes, odd pitch": _odd_pitch(w, s), "planes in B, G, R order": _dword_pitch(w, s),
                 "planes, negative pitch": _dword_pitch(w, s)}[name]
        plane = -(-(h * pitch * s + MARGIN) // 256) * 256  # planes start on multiples of 256, filler between them
        starts = [MARGIN, MARGIN + plane, MARGIN + 2 * plane + 256]  # (unequal gaps: no plane's place follows from the others')
        if name == "planes in B, G, R order":
            starts = starts[::-1]
        if name == "planes, negative pitch":
            return MARGIN + 3 * plane + 256, [p + (h - 1) * pitch * s for p in starts], -pitch, 1
        return MARGIN + 3 * plane + 256, starts, pitch, 1
    if name == "rgba":
        return 2 * MARGIN + 4 * w * h * s, [MARGIN + c * s for c in range(3)], 4 * w, 4
    if name == "crop":  # the picture at (3, 2) of a surface 8 pixels wider and 3 rows taller
        sw, x0, y0 = w + 8, 3, 2
        first = MARGIN + (y0 * sw + x0) * 3 * s
        return 2 * MARGIN + 3 * sw * (h + 3) * s, [first + c * s for c in range(3)], 3 * sw, 3
    k, pitch, order = 0, tight, (0, 1, 2)
    if name.startswith("interleaved, base + "):
        k = int(name.split()[3])
    elif name in ("padded pitch, dword rows", "negative pitch, dword rows"):
        pitch = _dword_pitch(tight, s)
    elif name in ("padded pitch, odd rows", "negative pitch, odd rows"):
        pitch = _odd_pitch(tight, s)
    elif name == "bgr":  # R, the channel the kernel's alignment test looks at, on a dword: only the pointer order refuses
        k, order = (4 - 2 * s) % 4, (2, 1, 0)
    elif name != "interleaved":
        raise KeyError(name)
    first = MARGIN + k
    size = first + h * pitch * s + MARGIN
    if name.startswith("negative pitch"):
        first, pitch = first + (h - 1) * pitch * s, -pitch
    return size, [first + c * s for c in order], pitch, 3


def sample_positions(offsets, row_stride, pixel_stride, w, h, s):
    """int64 (H, W, 3): the byte offset of every sample's first byte"""
    y = np.arange(h, dtype=np.int64)[:, None, None]
    x = np.arange(w, dtype=np.int64)[None, :, None]
    return np.asarray(offsets, np.int64)[None, None, :] + (y * row_stride + x * pixel_stride) * s


def build(name, picture, filler):
    """(buffer, channel_byte_offsets[3], row_stride, pixel_stride) of the contiguous (H, W, 3) `picture` in layout `name`"""
    h, w, c = picture.shape
    s = picture.dtype.itemsize
    assert c == 3 and s in (1, 2, 4) and picture.flags["C_CONTIGUOUS"] and name in layout_names(s)
    size, offsets, row_stride, pixel_stride = _spec(name, w, h, s)
    buf = np.full(size, filler, np.uint8)
    at = sample_positions(offsets, row_stride, pixel_stride, w, h, s)
    assert MARGIN <= int(at.min()) and int(at.max()) + s + MARGIN <= size
    raw = picture.view(np.uint8).reshape(h, w, 3, s)
    for b in range(s):
        buf[at + b] = raw[..., b]
    return buf, offsets, row_stride, pixel_stride


def gather(buf, offsets, row_stride, pixel_stride, w, h, dtype):
    """the (H, W, 3) picture that the offsets and strides name in `buf`, and a mask of the bytes it is made of"""
    s = np.dtype(dtype).itemsize
    at = sample_positions(offsets, row_stride, pixel_stride, w, h, s)
    raw = np.stack([buf[at + b] for b in range(s)], -1)
    used = np.zeros(buf.size, bool)
    for b in range(s):
        used[at + b] = True
    return np.ascontiguousarray(raw).view(dtype).reshape(h, w, 3), used


def loader(sample_fmt, channel_addresses, row_stride, pixel_stride):
    """The loader k_transform_tokenize takes for whole 8-pixel block rows of such a picture: "packed" (dword rows of 8- and
    16-bit samples), "half run", "half planes" or "per sample".  A ragged last block reads per sample whatever this says."""
    s = SAMPLE_BYTES[sample_fmt]
    a0, a1, a2 = (int(a) for a in channel_addresses)
    if sample_fmt in (0, 1):
        if pixel_stride == 3 and a1 == a0 + s and a2 == a0 + 2 * s and ((a0 | (row_stride * s)) & 3) == 0:
            return "packed"
    elif sample_fmt in (3, 4):
        rows4 = ((row_stride * 2) & 3) == 0
        if pixel_stride == 3 and rows4 and (a0 & 3) == 0 and a1 == a0 + 2 and a2 == a0 + 4:
            return "half run"
        if pixel_stride == 1 and rows4 and ((a0 | a1 | a2) & 3) == 0:
            return "half planes"
    return "per sample"


def widen_half_bits(bits, type_name):
    """float32 of the uint16 patterns of float16 or bfloat16 samples, exactly; a non-finite pattern stays non-finite"""
    bits = np.ascontiguousarray(bits, np.uint16)
    if type_name == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def knee_picture(w, h, seed=5):
    """uint16 (H, W, 3) with samples on both sides of the sRGB knee (2650: the last code of the curve's linear segment) in
    every 8-pixel block row, whole or ragged: each pixel has R at or below the knee and G above it, B on either side."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 2651, (h, w, 3))
    high = rng.integers(2651, 65536, (h, w, 3))
    side = rng.integers(0, 2, (h, w, 3)).astype(bool)
    side[..., 0], side[..., 1] = False, True
    return np.ascontiguousarray(np.where(side, high, low).astype(np.uint16))


def both_sides_of_the_knee(pic):
    """True when every 8-pixel block row of the uint16 picture, the ragged last one included, has samples <= 2650 and > 2650"""
    h, w, _ = pic.shape
    for x0 in range(0, w, 8):
        blk = pic[:, x0:x0 + 8, :].reshape(h, -1)
        if not ((blk <= 2650).any(1) & (blk > 2650).any(1)).all():
            return False
    return True
