"""The numpy model of the packed 4:2:2 YCbCr formats of 16-bit words, Y210 / Y212 / Y216 (include/hydrium_amd.h,
csrc/hyd_sample_fmt.h 32832 ..., csrc/hip/hydk_y216.h), composed from what exists: sample format = 32768 + matrix + 16 * filter +
64 * depth; the word order is what the three pointers spell; the words are MSB-aligned and count as stored.  De-interleave the
words, upsample each chroma plane of samples AS STORED with planar16_model.upsample16(S422, ...), convert with
p016_model.yuv_to_rgb(depth, matrix, ...).  No formula of its own.  The tests hold the library to the reference's file for the
RGB16 picture this model makes.  Written from the header's prose."""
from collections import namedtuple

import numpy as np

import chroma_model as cm
import p016_model as p16
import planar16_model as p16m
import planar_model as plm
import yuv_model as ym

FIRST_FORMAT = 32768
DEPTHS, BITS = p16.DEPTHS, p16.BITS
INFIX = ("", "c", "l")
FAMILY = tuple(FIRST_FORMAT + m + 16 * f + 64 * d for d in DEPTHS for f in cm.FILTERS for m in ym.MATRICES)
INTERPOLATED = tuple(f for f in FAMILY if ((f - FIRST_FORMAT) >> 4) & 3)
NEAREST = tuple(f for f in FAMILY if not ((f - FIRST_FORMAT) >> 4) & 3)
assert len(FAMILY) == 36 and len(INTERPOLATED) == 24 and len(NEAREST) == 12 and FAMILY[0] == 32832 and FAMILY[-1] == 32995
assert (FAMILY[0], FAMILY[12], FAMILY[24]) == (32832, 32896, 32960)  # Y210, Y212, Y216

# word order -> (offset of U, offset of V) from the first Y word, in words; listed in the C side's index order (HYD_PACKED_*)
ORDERS = {"yuyv": (1, 3), "yvyu": (3, 1), "uyvy": (-1, 1), "vyuy": (1, -1)}
ORDER_NAMES = tuple(ORDERS)
PACKED = 3  # HydFmt.layout: Y and chroma in one plane
LAYOUT_MSG = "Y210/Y216 wants pixel_stride 2 and U and V in the words beside Y"


def sample_fmt(matrix, filt, depth):
    assert matrix in ym.MATRICES and filt in cm.FILTERS and depth in DEPTHS
    return FIRST_FORMAT + matrix + 16 * filt + 64 * depth


def matrix_of(fmt):
    return (fmt - FIRST_FORMAT) & 3


def filter_of(fmt):
    return ((fmt - FIRST_FORMAT) >> 4) & 3


def depth_of(fmt):
    return (fmt - FIRST_FORMAT) >> 6


def bits_of(fmt):
    return BITS[depth_of(fmt)]


def is_format(fmt):
    n = fmt - FIRST_FORMAT
    return 64 <= n < 256 and not n & 12 and (n >> 4) & 3 != 3


def name_of(fmt):
    return f"y2{bits_of(fmt)}{INFIX[filter_of(fmt)]}-{ym.NAMES[matrix_of(fmt)]}"


def public_name(fmt):
    """the stem of HYDAMD_* and of the Python layer's constant"""
    return f"Y2{bits_of(fmt)}{INFIX[filter_of(fmt)].upper()}_{('BT709', 'BT709_FULL', 'BT601', 'BT601_FULL')[matrix_of(fmt)]}"


def as_i2xx(fmt):
    """the planar number of 16-bit words with the same matrix, filter and depth: I210, I212, I216"""
    return p16m.sample_fmt(matrix_of(fmt), plm.S422, filter_of(fmt), depth_of(fmt))


Fmt = namedtuple("Fmt", "device host is_float bytes layout matrix filter sub sx sy depth bits")
NOTHING = Fmt(*[0] * 12)


def describe(fmt):
    """what hyd_fmt_describe says of a number from 32700 up (the issue's prose: layout PACKED, bytes 2, 4:2:2, sx 1, sy 0, depth
    1 ... 3, bits 10 / 12 / 16, device 1, host 0)"""
    if not is_format(fmt):
        return NOTHING
    return Fmt(1, 0, 0, 2, PACKED, matrix_of(fmt), filter_of(fmt), plm.S422, 1, 0, depth_of(fmt), bits_of(fmt))


def y_offset(order):
    """where the first Y word sits in its group"""
    return 1 if min(ORDERS[order]) < 0 else 0


def interleave(planes, order, w):
    """(y (H, W), u (H, cw), v (H, cw)) uint16 -> (H, 4 cw) uint16 rows; for odd W the last group's second Y word is 0xEEEE: no pixel"""
    y, u, v = planes
    h, cw = y.shape[0], (w + 1) // 2
    assert y.shape == (h, w) and u.shape == v.shape == (h, cw)
    rows = np.zeros((h, 4 * cw), np.uint16)
    yo = y_offset(order)
    du, dv = ORDERS[order]
    luma = np.full((h, 2 * cw), 0xEEEE, np.uint16)
    luma[:, :w] = y
    rows[:, yo::2] = luma
    rows[:, yo + du::4] = u
    rows[:, yo + dv::4] = v
    return rows


def deinterleave(rows, order, w):
    """the definition: Y[y][x] the word at 2 x from the first Y word, U[y][cx], V[y][cx] the words at 4 cx from the first U and V word"""
    cw = (w + 1) // 2
    yo = y_offset(order)
    du, dv = ORDERS[order]
    assert rows.shape[1] >= 4 * cw and rows.dtype == np.uint16
    return (np.ascontiguousarray(rows[:, yo:4 * cw:2][:, :w]), np.ascontiguousarray(rows[:, yo + du:4 * cw:4]),
            np.ascontiguousarray(rows[:, yo + dv:4 * cw:4]))


def expected_rgb(rows, order, w, fmt):
    """(H, >= 4 cw) uint16 rows -> the (H, W, 3) uint16 picture `fmt` stands for: the 4:2:2 picture of the words as stored"""
    y, u, v = deinterleave(rows, order, w)
    h = y.shape[0]
    up = [p16m.upsample16(plm.S422, filter_of(fmt), c, w, h) for c in (u, v)]
    return np.ascontiguousarray(p16.yuv_to_rgb(depth_of(fmt), matrix_of(fmt), y, up[0], up[1]))
