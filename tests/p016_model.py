"""The numpy model of the P010 / P012 / P016 formats (include/hydrium_amd.h, csrc/hip/hydk_yuv16.h): the fixed-point formula
in int64 with a table built from Kr, Kb, the range and the depth, nearest-neighbour chroma and both interpolations (the taps
of chroma_model.py on 16-bit samples).  The tests hold the library to the reference's file for the RGB16 picture this model
makes.

Also a forward RGB16 -> P0xx helper, which only manufactures realistic inputs and is not under test."""
from fractions import Fraction

import numpy as np

import chroma_model as cm
import yuv_model as ym

DEPTHS = (1, 2, 3)  # (sample format - 16) >> 6
BITS = {1: 10, 2: 12, 3: 16}
DEPTH_NAMES = {1: "p010", 2: "p012", 3: "p016"}
BOUND = 0.5625  # half a code of rounding + 65535 * 2^-21 + 2 * 32768 * 2^-21 from the coefficients' own


def sample_fmt(depth, matrix, filt=cm.NEAREST):
    return ym.FIRST_FORMAT + matrix + 16 * filt + 64 * depth


def depth_of(fmt):
    return (fmt - ym.FIRST_FORMAT) >> 6


def matrix_of(fmt):
    return (fmt - ym.FIRST_FORMAT) & 3


def filter_of(fmt):
    return ((fmt - ym.FIRST_FORMAT) >> 4) & 3


FAMILY = tuple(sample_fmt(d, m, f) for d in DEPTHS for f in cm.FILTERS for m in ym.MATRICES)


def name_of(fmt):
    return f"{DEPTH_NAMES[depth_of(fmt)]}-{cm.FILTER_NAMES[filter_of(fmt)]}-{ym.NAMES[matrix_of(fmt)]}"


def exact_coefficients(depth, matrix):
    """(yo, sy, crv, cgu, cgv, cbu): yo an int, the rest exact rationals, from Kr, Kb, the range and the depth"""
    kr, kb = (Fraction(str(k)) for k in ym.KR_KB[matrix])
    kg = 1 - kr - kb
    if ym.LIMITED[matrix]:
        yo, sy, sc = 4096, Fraction(65535, 219 * 256), Fraction(65535, 224 * 256)
    else:
        n = BITS[depth]
        yo, sy = 0, Fraction(65535, ((1 << n) - 1) << (16 - n))
        sc = sy
    return (yo, sy, 2 * (1 - kr) * sc, 2 * (1 - kb) * kb / kg * sc, 2 * (1 - kr) * kr / kg * sc, 2 * (1 - kb) * sc)


def table_row(depth, matrix):
    """(yo, cy, crv, cgu, cgv, cbu) at the scale 2^20: floor(v * 2^20 + 0.5)"""
    co = exact_coefficients(depth, matrix)
    return (co[0],) + tuple(int((v * (1 << 20) + Fraction(1, 2)).__floor__()) for v in co[1:])


TABLE = {(d, m): table_row(d, m) for d in DEPTHS for m in ym.MATRICES}


def yuv_to_rgb(depth, matrix, y, u, v):
    """arrays of Y, U, V words (any integer type, one shape) -> uint16 array of that shape + (3,)"""
    yo, cy, crv, cgu, cgv, cbu = TABLE[depth, matrix]
    c, d, e = np.asarray(y, np.int64) - yo, np.asarray(u, np.int64) - 32768, np.asarray(v, np.int64) - 32768
    r = (cy * c + crv * e + (1 << 19)) >> 20
    g = (cy * c - cgu * d - cgv * e + (1 << 19)) >> 20
    b = (cy * c + cbu * d + (1 << 19)) >> 20
    return np.clip(np.stack([r, g, b], -1), 0, 65535).astype(np.uint16)


def yuv_to_rgb_real(depth, matrix, y, u, v):
    """the clamped real-valued conversion, float64, unrounded"""
    yo, sy, crv, cgu, cgv, cbu = (float(x) for x in exact_coefficients(depth, matrix))
    c, d, e = np.asarray(y, np.float64) - yo, np.asarray(u, np.float64) - 32768, np.asarray(v, np.float64) - 32768
    return np.clip(np.stack([sy * c + crv * e, sy * c - cgu * d - cgv * e, sy * c + cbu * d], -1), 0.0, 65535.0)


def upsample(filt, uv, w, h):
    """uv (ceil(h / 2), ceil(w / 2), 2) uint16 -> (h, w, 2) uint16: U', V' of every pixel of the w x h picture"""
    ch, cw = -(-h // 2), -(-w // 2)
    assert uv.shape == (ch, cw, 2) and uv.dtype == np.uint16 and filt in cm.FILTERS
    c = uv.astype(np.int64)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    cy, cx = y >> 1, x >> 1
    if filt == cm.NEAREST:
        return uv[cy, cx]
    vy = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    if filt == cm.CENTRE:
        hx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
        out = (9 * c[cy, cx] + 3 * c[cy, hx] + 3 * c[vy, cx] + c[vy, hx] + 8) >> 4
    else:
        hx = np.minimum(cx + 1, cw - 1)
        even = (3 * c[cy, cx] + c[vy, cx] + 2) >> 2
        odd = (3 * (c[cy, cx] + c[cy, hx]) + c[vy, cx] + c[vy, hx] + 4) >> 3
        out = np.where((x & 1)[..., None].astype(bool), odd, even)
    assert out.min() >= 0 and out.max() <= 65535
    return out.astype(np.uint16)


def expected_rgb(planes, fmt):
    """planes = (y (H, W) uint16, uv (ceil(H / 2), ceil(W / 2), 2) uint16) -> the (H, W, 3) uint16 picture `fmt` stands for"""
    y, uv = planes
    h, w = y.shape
    up = upsample(filter_of(fmt), uv, w, h)
    return np.ascontiguousarray(yuv_to_rgb(depth_of(fmt), matrix_of(fmt), y, up[..., 0], up[..., 1]))


def p016_of_rgb(rgb16, depth, matrix):
    """a realistic P010 / P012 / P016 picture from an RGB16 one (float arithmetic, 2 x 2 box chroma, n-bit codes shifted left
    by 16 - n): input manufacture only"""
    n = BITS[depth]
    top = float((1 << n) - 1)
    kr, kb = ym.KR_KB[matrix]
    kg = 1.0 - kr - kb
    p = rgb16.astype(np.float64) / 65535.0
    luma = kr * p[..., 0] + kg * p[..., 1] + kb * p[..., 2]
    cb, cr = (p[..., 2] - luma) / (2 * (1 - kb)), (p[..., 0] - luma) / (2 * (1 - kr))
    h, w = luma.shape
    pad = lambda a: np.pad(a, ((0, h % 2), (0, w % 2)), mode="edge")
    box = lambda a: pad(a).reshape((h + 1) // 2, 2, (w + 1) // 2, 2).mean((1, 3))
    unit = float(1 << (n - 8))
    if ym.LIMITED[matrix]:
        y, u, v = (16 + 219 * luma) * unit, (128 + 224 * box(cb)) * unit, (128 + 224 * box(cr)) * unit
    else:
        y, u, v = luma * top, 128 * unit + box(cb) * top, 128 * unit + box(cr) * top
    q = lambda a: (np.clip(np.rint(a), 0, top).astype(np.uint16) << (16 - n)).astype(np.uint16)
    return np.ascontiguousarray(q(y)), np.ascontiguousarray(np.stack([q(u), q(v)], -1))
