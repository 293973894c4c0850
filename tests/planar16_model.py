"""The numpy model of the planar YCbCr formats of 16-bit words (include/hydrium_amd.h, csrc/hyd_sample_fmt.h 2112 ...,
csrc/hip/hydk_yuvp16.h), composed from planar_model (geometry and taps) and p016_model (the conversion): sample format = 2048 +
matrix + 4 * subsampling + 16 * filter + 64 * depth; a stored word w of n significant bits is the sample (w << (16 - n)) & 0xFFFF;
each chroma plane of samples is upsampled by itself with planar_model's taps, then p016_model converts.  No third formula.  The
tests hold the library to the reference's file for the RGB16 picture this model makes.

Also a forward RGB16 -> planes helper, which only manufactures realistic inputs and is not under test."""
import numpy as np

import chroma_model as cm
import p016_model as p16
import planar_model as plm
import yuv_model as ym

FIRST_FORMAT = 2048
DEPTHS, BITS = p16.DEPTHS, p16.BITS
FORMS = plm.FORMS
FAMILY = tuple(FIRST_FORMAT + m + 4 * s + 16 * f + 64 * d for d in DEPTHS for s, f in FORMS for m in ym.MATRICES)
INTERPOLATED = tuple(f for f in FAMILY if (f >> 4) & 3)
NEAREST = tuple(f for f in FAMILY if not (f >> 4) & 3)
assert len(FAMILY) == 84 and len(INTERPOLATED) == 48 and len(NEAREST) == 36 and min(FAMILY) == 2112 and max(FAMILY) == 2279


def sample_fmt(matrix, sub, filt, depth):
    assert matrix in ym.MATRICES and (sub, filt) in FORMS and depth in DEPTHS
    return FIRST_FORMAT + matrix + 4 * sub + 16 * filt + 64 * depth


def matrix_of(fmt):
    return (fmt - FIRST_FORMAT) & 3


def sub_of(fmt):
    return ((fmt - FIRST_FORMAT) >> 2) & 3


def filter_of(fmt):
    return ((fmt - FIRST_FORMAT) >> 4) & 3


def depth_of(fmt):
    return (fmt - FIRST_FORMAT) >> 6


def bits_of(fmt):
    return BITS[depth_of(fmt)]


def is_format(fmt):
    return FIRST_FORMAT + 64 <= fmt < FIRST_FORMAT + 256 and (sub_of(fmt), filter_of(fmt)) in FORMS


def name_of(fmt):
    return f"i{'024'[sub_of(fmt)]}{bits_of(fmt)}{plm.INFIX[filter_of(fmt)]}-{ym.NAMES[matrix_of(fmt)]}"


def public_name(fmt):
    """the stem of HYDAMD_* and of the Python layer's constant"""
    return f"I{'024'[sub_of(fmt)]}{bits_of(fmt)}{plm.INFIX[filter_of(fmt)].upper()}_{('BT709', 'BT709_FULL', 'BT601', 'BT601_FULL')[matrix_of(fmt)]}"


def samples(depth, words):
    """stored words -> the P01x samples they stand for, uint16"""
    n = BITS[depth]
    return ((np.asarray(words).astype(np.uint32) << (16 - n)) & 0xFFFF).astype(np.uint16)


def upsample16(sub, filt, plane, w, h):
    """plane (ch, cw) uint16 SAMPLES -> (h, w) uint16: planar_model's geometry and taps, which are written for any integer width
    but assert 8-bit results; the same index arithmetic on int64 through its own function with the assertion lifted"""
    ch, cw = plm.chroma_shape(sub, w, h)
    assert plane.shape == (ch, cw) and plane.dtype == np.uint16
    if filt == cm.NEAREST:
        return plm.upsample(sub, filt, plane, w, h)  # a pure gather: any dtype
    if sub == plm.S420:  # p016_model's upsampling is chroma_model's taps on 16-bit pairs: feed it the plane twice
        return p16.upsample(filt, np.stack([plane, plane], -1), w, h)[..., 0]
    # 4:2:2: the 4:2:0 taps with the far row equal to the near one (tests/test_planar_formats.py proves it of the 8-bit model): a
    # picture of 2h rows whose chroma rows are these, every picture row y of ours being row 2y there ... which reads row y - 1 as
    # far; so instead double the ROWS of the plane and read picture rows 4y + 1 (near and far both copies of row y)
    tall = p16.upsample(filt, np.stack([np.repeat(plane, 2, 0)] * 2, -1), w, 4 * h)
    return np.ascontiguousarray(tall[1::4, :, 0])


def expected_rgb(planes, fmt):
    """planes = (y (H, W), u (ch, cw), v (ch, cw)) of stored 16-bit words -> the (H, W, 3) uint16 picture `fmt` stands for"""
    y, u, v = planes
    h, w = y.shape
    d, sub, filt = depth_of(fmt), sub_of(fmt), filter_of(fmt)
    up = [upsample16(sub, filt, samples(d, c), w, h) for c in (u, v)]
    return np.ascontiguousarray(p16.yuv_to_rgb(d, matrix_of(fmt), samples(d, y), up[0], up[1]))


def planes_of_rgb(rgb16, depth, matrix, sub):
    """a realistic planar picture of valid n-bit codes, LSB-aligned, from an RGB16 one: p016_model's forward helper for luma and
    range, planar_model's box for the subsampling.  Input manufacture only"""
    n = BITS[depth]
    top = float((1 << n) - 1)
    kr, kb = ym.KR_KB[matrix]
    kg = 1.0 - kr - kb
    p = rgb16.astype(np.float64) / 65535.0
    luma = kr * p[..., 0] + kg * p[..., 1] + kb * p[..., 2]
    cb, cr = (p[..., 2] - luma) / (2 * (1 - kb)), (p[..., 0] - luma) / (2 * (1 - kr))
    h, w = luma.shape
    sx, sy = plm.shifts(sub)
    ch, cw = plm.chroma_shape(sub, w, h)

    def box(a):
        a = np.pad(a, ((0, (ch << sy) - h), (0, (cw << sx) - w)), mode="edge")
        return a.reshape(ch, 1 << sy, cw, 1 << sx).mean((1, 3))

    unit = float(1 << (n - 8))
    if ym.LIMITED[matrix]:
        y, u, v = (16 + 219 * luma) * unit, (128 + 224 * box(cb)) * unit, (128 + 224 * box(cr)) * unit
    else:
        y, u, v = luma * top, 128 * unit + box(cb) * top, 128 * unit + box(cr) * top
    q = lambda a: np.ascontiguousarray(np.clip(np.rint(a), 0, top).astype(np.uint16))
    return q(y), q(u), q(v)


def interleave(u, v):
    """two (ch, cw) planes -> the (ch, cw, 2) pair plane of a P01x picture"""
    return np.ascontiguousarray(np.stack([u, v], -1))


# ---- the C side's predicates (csrc/hyd_sample_fmt.h) as a table: what tests/c/planar16_formats.cc is held to ----
def predicate_row(fmt):
    """(is_planar16, sub, filter, matrix, depth, bits, sx, sy, is_planar16_interp); zeros where the number is no such format"""
    if not is_format(fmt):
        return (0,) * 9
    sx, sy = plm.shifts(sub_of(fmt))
    return (1, sub_of(fmt), filter_of(fmt), matrix_of(fmt), depth_of(fmt), bits_of(fmt), sx, sy, int(filter_of(fmt) != 0))


def older_row(fmt):
    """the eight columns planar_model.predicate_row gives, with this family's bytes and is_device added"""
    row = list(plm.predicate_row(fmt))
    if is_format(fmt):
        row[5], row[6] = 2, 1
    return tuple(row)
