"""The numpy model of the formats whose pixel is one 32-bit word of three 10-bit fields and two spare bits (include/hydrium_amd.h,
csrc/hyd_sample_fmt.h 131072 ..., csrc/hip/hydk_rgb10.h): RGB10A2 = 131072 (R in bits 0 ... 9), BGR10A2 = 131073 (B in bits
0 ... 9), Y410 = 131072 + matrix + 4 * 2 + 64 * 1 (U in bits 0 ... 9, Y in 10 ... 19, V in 20 ... 29).  An RGB field v stands for the
16-bit sample (v * 65535 + 511) // 1023; a Y410 picture is the I410 picture of its three fields, so planar16_model makes it: no
formula of its own for YCbCr.  The tests hold the library to the reference's file for the RGB16 picture this model makes.  Written
from the header's prose."""
from collections import namedtuple

import numpy as np

import planar16_model as p16m
import planar_model as plm
import yuv_model as ym

FIRST_FORMAT = 131072
RGB10A2, BGR10A2 = 131072, 131073
RGB_FORMS = (RGB10A2, BGR10A2)
Y410 = tuple(FIRST_FORMAT + m + 4 * 2 + 64 * 1 for m in ym.MATRICES)
FAMILY = RGB_FORMS + Y410
assert FAMILY == (131072, 131073, 131144, 131145, 131146, 131147)
DWORD = 4  # HydFmt.layout: a pixel is one dword
LAYOUT_MSG = "RGB10A2/Y410 wants pixel_stride 1 and three equal pointers on a 4-byte boundary"
STORE_RGB10, STORE_Y410 = 15, 16  # csrc/hip/hydk_store.h
VARIANT_RGB10, VARIANT_Y410 = 32768, 65536

Fmt = namedtuple("Fmt", "device host is_float bytes layout matrix filter sub sx sy depth bits")
NOTHING = Fmt(*[0] * 12)


def is_format(fmt):
    return fmt in FAMILY


def is_ycbcr(fmt):
    return fmt in Y410


def matrix_of(fmt):
    assert is_ycbcr(fmt)
    return (fmt - FIRST_FORMAT) & 3


def public_name(fmt):
    """the stem of HYDAMD_* and of the Python layer's constant"""
    if fmt in RGB_FORMS:
        return ("RGB10A2", "BGR10A2")[fmt - FIRST_FORMAT]
    return "Y410_" + ("BT709", "BT709_FULL", "BT601", "BT601_FULL")[matrix_of(fmt)]


def as_i410(fmt):
    """the planar number of 16-bit words with the same matrix: I410, 2120 + matrix"""
    planar = p16m.sample_fmt(matrix_of(fmt), plm.S444, 0, 1)
    assert planar == 2120 + matrix_of(fmt)
    return planar


def describe(fmt):
    """what hyd_fmt_describe says of a number from 130900 up (the issue's table: device 1, host 0, bytes 4, bits 10, the new layout,
    filter, sx, sy 0; Y410 sub 2, depth 1 and its matrix; the RGB forms sub, depth and matrix 0)"""
    if not is_format(fmt):
        return NOTHING
    if fmt in RGB_FORMS:
        return Fmt(1, 0, 0, 4, DWORD, 0, 0, 0, 0, 0, 0, 10)
    return Fmt(1, 0, 0, 4, DWORD, matrix_of(fmt), 0, plm.S444, 0, 0, 1, 10)


def job(fmt):
    """(ok, the format encoded back, cls, storage, a job's matrix, variant) of csrc/hip/hydk_store.h: both forms of the 16-bit class;
    Y410's matrix is matrix + 4 * depth as P010's"""
    if not is_format(fmt):
        return (0, -1, 0, 0, 0, 0)
    if fmt in RGB_FORMS:
        return (1, fmt, 1, STORE_RGB10, 0, VARIANT_RGB10)
    return (1, fmt, 1, STORE_Y410, matrix_of(fmt) + 4, VARIANT_Y410)


def fields(dwords):
    """(H, W) uint32 -> the three (H, W) uint16 planes of fields 0, 1, 2; bits 30 and 31 fall away"""
    d = np.asarray(dwords).astype(np.uint32)
    return tuple(np.ascontiguousarray(((d >> (10 * k)) & 1023).astype(np.uint16)) for k in range(3))


def pack(f0, f1, f2, spare=0):
    """three planes of 10-bit codes -> dwords, `spare` (0 ... 3, or a plane of them) in bits 30 and 31"""
    f = [np.asarray(a).astype(np.uint32) for a in (f0, f1, f2)]
    assert all(int(a.max(initial=0)) < 1024 for a in f)
    return np.ascontiguousarray(f[0] | f[1] << 10 | f[2] << 20 | (np.asarray(spare).astype(np.uint32) & 3) << 30)


def widen(v):
    """the 16-bit sample nearest to v / 1023, in integers as the issue writes it"""
    v = np.asarray(v).astype(np.int64)
    return ((v * 65535 + 511) // 1023).astype(np.uint16)


def y410_planes(dwords):
    """the I410 planes of a Y410 surface: Y, U, V LSB-aligned, chroma pitch = width"""
    u, y, v = fields(dwords)
    return y, u, v


def expected_rgb(dwords, fmt):
    """(H, W) uint32 -> the (H, W, 3) uint16 picture `fmt` stands for"""
    assert is_format(fmt)
    if fmt in RGB_FORMS:
        lo, mid, hi = fields(dwords)
        r, b = (lo, hi) if fmt == RGB10A2 else (hi, lo)
        return np.ascontiguousarray(np.stack([widen(r), widen(mid), widen(b)], -1))
    return p16m.expected_rgb(y410_planes(dwords), as_i410(fmt))


def surface_of_rgb(rgb16, fmt, spare=0):
    """a realistic surface of valid codes from an RGB16 picture.  Input manufacture only: the RGB forms take the top ten bits, Y410
    planar16_model's forward helper at 4:4:4"""
    if fmt in RGB_FORMS:
        r, g, b = (rgb16[..., c] >> 6 for c in range(3))
        return pack(r, g, b, spare) if fmt == RGB10A2 else pack(b, g, r, spare)
    y, u, v = p16m.planes_of_rgb(rgb16, 1, matrix_of(fmt), plm.S444)
    return pack(u, y, v, spare)
