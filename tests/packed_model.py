"""The numpy model of the packed 4:2:2 YCbCr formats (include/hydrium_amd.h, csrc/hyd_sample_fmt.h 8192 ..., csrc/hip/hydk_yuy2.h),
on top of planar_model by de-interleaving: sample format = 8192 + matrix + 16 * filter; the byte order is what the three pointers
spell; the picture is the I422 picture of the de-interleaved bytes.  The tests hold the library to the reference's file for the
RGB8 picture this model makes.  Written from the header's prose."""
from collections import namedtuple

import numpy as np

import chroma_model as cm
import planar_model as plm
import yuv_model as ym

FIRST_FORMAT = 8192
INFIX = ("", "c", "l")
FAMILY = tuple(FIRST_FORMAT + m + 16 * f for f in cm.FILTERS for m in ym.MATRICES)
INTERPOLATED = tuple(f for f in FAMILY if (f - FIRST_FORMAT) >> 4)
assert len(FAMILY) == 12 and len(INTERPOLATED) == 8 and FAMILY[0] == 8192 and FAMILY[-1] == 8227

# byte order -> (offset of U, offset of V) from the first Y byte; the order in which the header lists them is the C side's index
ORDERS = {"yuyv": (1, 3), "yvyu": (3, 1), "uyvy": (-1, 1), "vyuy": (1, -1)}
ORDER_NAMES = tuple(ORDERS)
PACKED = 3  # HydFmt.layout: Y and chroma in one plane
LAYOUT_MSG = "YUY2/UYVY wants pixel_stride 2 and U and V in the bytes beside Y"


def sample_fmt(matrix, filt):
    assert matrix in ym.MATRICES and filt in cm.FILTERS
    return FIRST_FORMAT + matrix + 16 * filt


def matrix_of(fmt):
    return (fmt - FIRST_FORMAT) & 3


def filter_of(fmt):
    return (fmt - FIRST_FORMAT) >> 4


def is_format(fmt):
    n = fmt - FIRST_FORMAT
    return 0 <= n < 48 and not n & 12


def name_of(fmt):
    return f"yuy2{INFIX[filter_of(fmt)]}-{ym.NAMES[matrix_of(fmt)]}"


def as_i422(fmt):
    """the planar number the same planes have"""
    return plm.sample_fmt(matrix_of(fmt), plm.S422, filter_of(fmt))


Fmt = namedtuple("Fmt", "device host is_float bytes layout matrix filter sub sx sy depth bits")
NOTHING = Fmt(*[0] * 12)


def describe(fmt):
    """what hyd_fmt_describe says of a number from 8150 up (the issue's prose: bytes 1, bits 8, 4:2:2, sx 1, sy 0, device 1, host 0)"""
    if not is_format(fmt):
        return NOTHING
    return Fmt(1, 0, 0, 1, PACKED, matrix_of(fmt), filter_of(fmt), plm.S422, 1, 0, 0, 8)


def y_offset(order):
    """where the first Y byte sits in its group"""
    return 1 if min(ORDERS[order]) < 0 else 0


def interleave(planes, order, w):
    """(y (H, W), u (H, cw), v (H, cw)) -> (H, 4 cw) uint8 rows; for odd W the last group's second Y byte is 0xEE: no pixel"""
    y, u, v = planes
    h, cw = y.shape[0], (w + 1) // 2
    assert y.shape == (h, w) and u.shape == v.shape == (h, cw)
    rows = np.zeros((h, 4 * cw), np.uint8)
    yo = y_offset(order)
    du, dv = ORDERS[order]
    luma = np.full((h, 2 * cw), 0xEE, np.uint8)
    luma[:, :w] = y
    rows[:, yo::2] = luma
    rows[:, yo + du::4] = u
    rows[:, yo + dv::4] = v
    return rows


def deinterleave(rows, order, w):
    """the definition: Y[y][x] the byte at 2 x from the first Y byte, U[y][cx], V[y][cx] the bytes at 4 cx from the first U and V byte"""
    cw = (w + 1) // 2
    yo = y_offset(order)
    du, dv = ORDERS[order]
    assert rows.shape[1] >= 4 * cw
    return (np.ascontiguousarray(rows[:, yo:4 * cw:2][:, :w]), np.ascontiguousarray(rows[:, yo + du:4 * cw:4]),
            np.ascontiguousarray(rows[:, yo + dv:4 * cw:4]))


def expected_rgb(rows, order, w, matrix, filt):
    """(H, >= 4 cw) uint8 rows -> the (H, W, 3) uint8 picture the format stands for: the I422 picture of the de-interleaved bytes"""
    return plm.expected_rgb(deinterleave(rows, order, w), matrix, plm.S422, filt)
