"""The numpy model of the formats whose pixel is one group of four samples, Y, U, V and a fourth that is ignored (include/hydrium_amd.h,
csrc/hyd_sample_fmt.h 524288 ..., csrc/hip/hydk_quad.h): packed 4:4:4 YCbCr, 524288 + matrix + 4 * 2 + 64 * depth.  AYUV (depth 0) is
one dword of the bytes V, U, Y, A and stands for the I444 picture of its three bytes; Y412 and Y416 (depth 2, 3) are one qword of the
words U, Y, V, A, MSB-aligned, the words as stored under the P01x conversion of that depth — a Y416 picture is the I416 picture of its
words.  There is no formula of its own here: planar_model and p016_model make the pictures.  The tests hold the library to the
reference's file for the RGB8 or RGB16 picture this model makes.  Written from the header's prose."""
from collections import namedtuple

import numpy as np

import p016_model as p6m
import planar16_model as p16m
import planar_model as plm
import yuv_model as ym

FIRST_FORMAT = 524288
AYUV = tuple(FIRST_FORMAT + m + 4 * 2 for m in ym.MATRICES)
Y412 = tuple(FIRST_FORMAT + m + 4 * 2 + 64 * 2 for m in ym.MATRICES)
Y416 = tuple(FIRST_FORMAT + m + 4 * 2 + 64 * 3 for m in ym.MATRICES)
FAMILY = AYUV + Y412 + Y416
assert FAMILY == (524296, 524297, 524298, 524299, 524424, 524425, 524426, 524427, 524488, 524489, 524490, 524491)
QUAD = 5  # HydFmt.layout: a pixel is one group of four samples
LAYOUT_MSG = "AYUV/Y416 wants pixel_stride 1 and three equal pointers on a boundary of the pixel's size"
STORE_AYUV, STORE_Y416 = 17, 18  # csrc/hip/hydk_store.h
VARIANT_AYUV, VARIANT_Y416 = 131072, 262144
BITS = {0: 8, 2: 12, 3: 16}

Fmt = namedtuple("Fmt", "device host is_float bytes layout matrix filter sub sx sy depth bits")
NOTHING = Fmt(*[0] * 12)


def is_format(fmt):
    return fmt in FAMILY


def matrix_of(fmt):
    assert is_format(fmt)
    return (fmt - FIRST_FORMAT) & 3


def depth_of(fmt):
    assert is_format(fmt)
    return (fmt - FIRST_FORMAT) >> 6


def pixel_bytes(fmt):
    return 8 if depth_of(fmt) else 4


def dtype_of(fmt):
    """a pixel as one integer: the dword, or the qword"""
    return np.uint64 if depth_of(fmt) else np.uint32


def public_name(fmt):
    """the stem of HYDAMD_* and of the Python layer's constant"""
    return {0: "AYUV_", 2: "Y412_", 3: "Y416_"}[depth_of(fmt)] + ("BT709", "BT709_FULL", "BT601", "BT601_FULL")[matrix_of(fmt)]


def describe(fmt):
    """what hyd_fmt_describe says of a number from 524000 up (the issue's table: device 1, host 0, bytes 4 or 8, bits 8 / 12 / 16,
    the new layout, 4:4:4, filter, sx, sy 0)"""
    if not is_format(fmt):
        return NOTHING
    d = depth_of(fmt)
    return Fmt(1, 0, 0, 8 if d else 4, QUAD, matrix_of(fmt), 0, plm.S444, 0, 0, d, BITS[d])


def job(fmt):
    """(ok, the format encoded back, cls, storage, a job's matrix, variant) of csrc/hip/hydk_store.h: AYUV of the 8-bit class,
    Y412 / Y416 of the 16-bit class with matrix + 4 * depth as P01x's"""
    if not is_format(fmt):
        return (0, -1, 0, 0, 0, 0)
    d = depth_of(fmt)
    if d == 0:
        return (1, fmt, 0, STORE_AYUV, matrix_of(fmt), VARIANT_AYUV)
    return (1, fmt, 1, STORE_Y416, matrix_of(fmt) + 4 * d, VARIANT_Y416)


def samples(pixels, fmt):
    """(H, W) dwords or qwords -> the (H, W) planes Y, U, V and the fourth, as stored (uint8 or uint16)"""
    p = np.asarray(pixels).astype(np.uint64)
    if depth_of(fmt):
        u, y, v, a = (((p >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.uint16) for k in range(4))
    else:
        assert int(p.max(initial=0)) < 2 ** 32
        v, u, y, a = (((p >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint8) for k in range(4))
    return tuple(np.ascontiguousarray(x) for x in (y, u, v, a))


def pack(y, u, v, a, fmt):
    """the planes Y, U, V and the fourth sample (a plane or a number) -> (H, W) dwords or qwords"""
    wide = depth_of(fmt) != 0
    top = 0xFFFF if wide else 0xFF
    y, u, v = (np.asarray(x).astype(np.uint64) for x in (y, u, v))
    a = np.broadcast_to(np.asarray(a).astype(np.uint64), y.shape)
    assert all(int(x.max(initial=0)) <= top for x in (y, u, v, a))
    order = (u, y, v, a) if wide else (v, u, y, a)
    out = np.zeros(y.shape, np.uint64)
    for k, x in enumerate(order):
        out |= x << np.uint64((16 if wide else 8) * k)
    return np.ascontiguousarray(out.astype(dtype_of(fmt)))


def as_planar(fmt):
    """the planar number with the same matrix whose picture this is: I444, I412 or I416"""
    d = depth_of(fmt)
    planar = 520 + matrix_of(fmt) if d == 0 else p16m.sample_fmt(matrix_of(fmt), plm.S444, 0, d)
    assert planar == {0: 520, 2: 2184, 3: 2248}[d] + matrix_of(fmt)
    return planar


def expected_rgb(pixels, fmt):
    """(H, W) dwords or qwords -> the (H, W, 3) uint8 or uint16 picture `fmt` stands for.  AYUV: hydk_yuv_to_rgb's model on its bytes (what the I444 model does at 4:4:4).
    Y412 / Y416: the words AS STORED under the P01x conversion of the depth (low bits are not masked)"""
    assert is_format(fmt)
    y, u, v, _ = samples(pixels, fmt)
    if depth_of(fmt) == 0:
        return np.ascontiguousarray(ym.yuv_to_rgb(matrix_of(fmt), y, u, v))
    return np.ascontiguousarray(p6m.yuv_to_rgb(depth_of(fmt), matrix_of(fmt), y, u, v))


def surface_of_rgb(rgb, fmt, fourth=0):
    """a realistic surface of valid codes from an RGB8 (AYUV) or RGB16 (Y412, Y416) picture.  Input manufacture only: the planar
    models' forward helpers at 4:4:4; Y412's codes are shifted to the top of the word, its low four bits zero"""
    d = depth_of(fmt)
    if d == 0:
        y, u, v = plm.planes_of_rgb(rgb, matrix_of(fmt), plm.S444)
    else:
        y, u, v = (np.asarray(x).astype(np.uint16) << (16 - BITS[d]) for x in p16m.planes_of_rgb(rgb, d, matrix_of(fmt), plm.S444))
    return pack(y, u, v, fourth, fmt)
