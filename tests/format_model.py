"""The sample formats as include/hydrium_amd.h and the opening comment of csrc/hyd_sample_fmt.h DEFINE them in prose, written
without a look at the C: the 165 numbers spelled per family, and describe(fmt) — everything a caller may ask of a number.  The
C side's hyd_fmt_describe is held to it on every number of -8 ... 4100 (tests/format_dump.py, tests/test_host_sanitizers.py), and
the four family models (yuv_model / chroma_model, p016_model, planar_model, planar16_model) are held to it in turn.

  0, 1, 2     uint8, uint16, float32: what host and device entry points take
  3, 4        float16, bfloat16: device pixels only, float class
  16 + matrix + 16 * filter + 64 * depth                        a Y plane and a plane of (U, V) pairs, 4:2:0; depth 0: NV12, 8
                                                                bits; depth 1, 2, 3: P010, P012, P016 in 16-bit words
  512 + matrix + 4 * subsampling + 16 * filter                  a plane each, 8 bits: I420, I422, I444
  2048 + matrix + 4 * subsampling + 16 * filter + 64 * depth    a plane each in 16-bit words, depth 1, 2, 3: I010 ... I416

matrix 0 ... 3; filter 0 nearest, 1 centre-sited, 2 left-sited; subsampling 0 4:2:0, 1 4:2:2, 2 4:4:4 (nearest only)."""
from collections import namedtuple

Fmt = namedtuple("Fmt", "device host is_float bytes layout matrix filter sub sx sy depth bits")
NOTHING = Fmt(*[0] * 12)
RGB, PAIRS, PLANES = 0, 1, 2  # layout; of a YCbCr format, the number of its chroma planes
LO, HI = -8, 4101  # the range the C side is dumped over

# the numbers, family by family, as the public header lists them
RGB_FORMATS = (0, 1, 2, 3, 4)
NV12_FAMILY = (16, 17, 18, 19, 32, 33, 34, 35, 48, 49, 50, 51)
P016_FAMILY = tuple(first + m for first in (80, 96, 112, 144, 160, 176, 208, 224, 240) for m in range(4))
_PLANAR_ROWS = (0, 4, 8, 16, 20, 32, 36)  # I420, I422, I444, I420C, I422C, I420L, I422L
PLANAR_FAMILY = tuple(512 + row + m for row in _PLANAR_ROWS for m in range(4))
PLANAR16_FAMILY = tuple(first + row + m for first in (2112, 2176, 2240) for row in _PLANAR_ROWS for m in range(4))
FAMILIES = (RGB_FORMATS, NV12_FAMILY, P016_FAMILY, PLANAR_FAMILY, PLANAR16_FAMILY)
ALL = tuple(f for family in FAMILIES for f in family)
assert [len(f) for f in FAMILIES] == [5, 12, 36, 28, 84] and len(ALL) == len(set(ALL)) == 165

BITS = (8, 10, 12, 16)
MATRIX_NAMES = ("BT709", "BT709_FULL", "BT601", "BT601_FULL")


def describe(fmt):
    if fmt not in ALL:
        return NOTHING
    if fmt in RGB_FORMATS:
        size = (1, 2, 4, 2, 2)[fmt]
        return Fmt(1, int(fmt <= 2), int(fmt >= 2), size, RGB, 0, 0, 0, 0, 0, 0, 8 * size)
    base = 16 if fmt < 512 else 512 if fmt < 2048 else 2048
    matrix, rest = (fmt - base) % 4, (fmt - base) // 4
    sub, rest = rest % 4, rest // 4
    filt, depth = rest % 4, rest // 4
    sx, sy = int(sub != 2), int(sub == 0)  # pairs are 4:2:0, and their subsampling field is 0
    return Fmt(1, 0, 0, 2 if depth else 1, PAIRS if base == 16 else PLANES, matrix, filt, sub, sx, sy, depth, BITS[depth])


def storage_of(fmt):
    """(class, storage form, variant bit) a job of this format holds — csrc/hip/hydk_store.h's table, read off its comments:
    forms 0 ... 2 float32 / float16 / bfloat16 (0 also RGB of 8 and 16 bits), 3 NV12, 4 NV12 interpolated, 5, 6 P016, 7, 8
    planar, 9, 10 planar of 16-bit words; class 0 8-bit, 1 16-bit, 2 float; the YCbCr forms' variant bits 8, 16 ... 1024"""
    d = describe(fmt)
    if not d.device:
        return (0, 0, 0)
    if d.layout == RGB:
        return (2 if d.is_float else fmt, {3: 1, 4: 2}.get(fmt, 0), 0)
    form = {(PAIRS, 1): 3, (PAIRS, 2): 5, (PLANES, 1): 7, (PLANES, 2): 9}[d.layout, d.bytes] + int(d.filter != 0)
    return (d.bytes - 1, form, 8 << (form - 3))


def public_name(fmt, d=None):
    """the stem of HYDAMD_* and of the Python layer's constant that a YCbCr format's description (d: as the C side gave it)
    spells: layout and depth give the stem, the filter the C / L infix, the matrix the suffix"""
    d = d or describe(fmt)
    assert d.layout != RGB
    if d.layout == PAIRS:
        stem = "NV12" if d.depth == 0 else f"P0{d.bits}"
    else:
        stem = f"I{('420', '422', '444')[d.sub]}" if d.depth == 0 else f"I{'024'[d.sub]}{d.bits}"
    return f"{stem}{('', 'C', 'L')[d.filter]}_{MATRIX_NAMES[d.matrix]}"
