"""The numpy model of the formats whose pixel is one 32-bit word of three unsigned floats (include/hydrium_amd.h, csrc/hyd_sample_fmt.h
8388608 ..., csrc/hip/hydk_ufloat.h): R11G11B10F = 8388608 (R in bits 0 ... 10, G in 11 ... 21, B in 22 ... 31; a 5-bit exponent of bias 15
above 6, 6 and 5 mantissa bits) and RGB9E5 = 8388609 (9-bit mantissas in bits 0 ... 8, 9 ... 17, 18 ... 26 under the shared exponent in
27 ... 31; a channel is m * 2^(E - 24)).  A field is widened exactly to float32: the values here are computed in float64, which holds every
one of them exactly, and then cast.  The tests hold the library to the reference's file for the float32 picture this model makes.
Written from the header's prose; the packers are for making test pictures."""
from collections import namedtuple

import numpy as np

FIRST_FORMAT = 8388608
R11G11B10F, RGB9E5 = 8388608, 8388609
FAMILY = (R11G11B10F, RGB9E5)
UFLOAT = 6  # HydFmt.layout: a pixel is one dword of unsigned floats
LAYOUT_MSG = "R11G11B10F/RGB9E5 wants pixel_stride 1 and three equal pointers on a 4-byte boundary"
STORE_R11G11B10F, STORE_RGB9E5 = 19, 20  # csrc/hip/hydk_store.h
CLS_FLOAT = 2

Fmt = namedtuple("Fmt", "device host is_float bytes layout matrix filter sub sx sy depth bits")
NOTHING = Fmt(*[0] * 12)


def is_format(fmt):
    return fmt in FAMILY


def which_of(fmt):
    """HYDK_UFLOAT_*: 0 R11G11B10F, 1 RGB9E5"""
    assert is_format(fmt)
    return fmt - FIRST_FORMAT


def public_name(fmt):
    return ("R11G11B10F", "RGB9E5")[which_of(fmt)]


def describe(fmt):
    """what hyd_fmt_describe says: device 1, host 0, float class, 4 bytes, the new layout, all 32 bits, nothing of YCbCr"""
    return Fmt(1, 0, 1, 4, UFLOAT, 0, 0, 0, 0, 0, 0, 32) if is_format(fmt) else NOTHING


def job(fmt):
    """(ok, the format encoded back, cls, storage, a job's matrix, variant) of csrc/hip/hydk_store.h: the float class has no variant"""
    if not is_format(fmt):
        return (0, -1, 0, 0, 0, 0)
    return (1, fmt, CLS_FLOAT, STORE_R11G11B10F + which_of(fmt), 0, 0)


def field_value(v, mbits):
    """an unsigned float of a 5-bit exponent above `mbits` mantissa bits, as float64 (exact); Inf and NaN where the exponent is 31"""
    v = np.asarray(v).astype(np.int64)
    e, m = v >> mbits, v & ((1 << mbits) - 1)
    normal = np.ldexp(1.0 + m / float(1 << mbits), (e - 15).astype(np.int64))
    sub = np.ldexp(m.astype(np.float64), -14 - mbits)
    out = np.where(e == 0, sub, normal)
    out = np.where((e == 31) & (m == 0), np.inf, out)
    return np.where((e == 31) & (m != 0), np.nan, out)


def widen_field(v, mbits):
    """the float32 BITS of a field: the exact value, and for a NaN the mantissa bits at the top of the float32 mantissa"""
    v = np.asarray(v).astype(np.int64)
    e, m = v >> mbits, v & ((1 << mbits) - 1)
    with np.errstate(invalid="ignore"):
        bits = field_value(v, mbits).astype(np.float32).view(np.uint32)
    nan = (0x7F800000 | (m << (23 - mbits))).astype(np.uint32)
    return np.where((e == 31) & (m != 0), nan, bits).astype(np.uint32)


def e5_value(m, e):
    """an RGB9E5 channel as float64 (exact): m * 2^(e - 24)"""
    return np.ldexp(np.asarray(m).astype(np.float64), np.asarray(e).astype(np.int64) - 24)


def widen_e5(m, e):
    return e5_value(m, e).astype(np.float32).view(np.uint32)


def fields(dwords, fmt):
    """(H, W) uint32 -> R11G11B10F: the three fields (11, 11, 10 bits); RGB9E5: the three mantissas and the exponent"""
    d = np.asarray(dwords).astype(np.uint32)
    if fmt == R11G11B10F:
        return d & 0x7FF, (d >> 11) & 0x7FF, d >> 22
    return d & 0x1FF, (d >> 9) & 0x1FF, (d >> 18) & 0x1FF, d >> 27


def expected_bits(dwords, fmt):
    """(H, W) uint32 -> the (H, W, 3) uint32 float32 bits of the picture `fmt` stands for"""
    assert is_format(fmt)
    if fmt == R11G11B10F:
        r, g, b = fields(dwords, fmt)
        planes = [widen_field(r, 6), widen_field(g, 6), widen_field(b, 5)]
    else:
        r, g, b, e = fields(dwords, fmt)
        planes = [widen_e5(c, e) for c in (r, g, b)]
    return np.ascontiguousarray(np.stack(planes, -1).astype(np.uint32))


def expected_f32(dwords, fmt):
    """the same picture as float32 samples"""
    return expected_bits(dwords, fmt).view(np.float32)


# ---- packers: float32 pictures to the nearest representable fields ----
def _finite_table(mbits):
    return field_value(np.arange(31 << mbits), mbits)  # increasing with the code


def pack_field(x, mbits):
    """float -> the code of the nearest finite value (ties to the even code); negatives to 0, above the largest to the largest"""
    table = _finite_table(mbits)
    x = np.clip(np.nan_to_num(np.asarray(x, np.float64), nan=0.0), 0.0, table[-1])
    hi = np.clip(np.searchsorted(table, x), 1, table.size - 1)
    lo = hi - 1
    dlo, dhi = x - table[lo], table[hi] - x
    return np.where((dlo < dhi) | ((dlo == dhi) & (lo % 2 == 0)), lo, hi).astype(np.uint32)


def pack_r11g11b10f(rgb):
    rgb = np.asarray(rgb)
    return np.ascontiguousarray(pack_field(rgb[..., 0], 6) | pack_field(rgb[..., 1], 6) << 11 | pack_field(rgb[..., 2], 5) << 22).astype(np.uint32)


def pack_rgb9e5(rgb):
    """the shared exponent of the largest channel, the mantissas rounded to nearest under it (the GL specification's recipe)"""
    c = np.clip(np.nan_to_num(np.asarray(rgb, np.float64), nan=0.0), 0.0, 511.0 * 2.0 ** 7)
    top = c.max(-1)
    e = np.maximum(-16, np.floor(np.log2(np.maximum(top, 2.0 ** -30)))).astype(np.int64) + 1 + 15
    e = np.where(np.floor(top / np.ldexp(1.0, e - 24) + 0.5) == 512, e + 1, e)
    e = np.clip(e, 0, 31)
    m = np.floor(c / np.ldexp(1.0, e - 24)[..., None] + 0.5).astype(np.int64)
    assert int(m.max(initial=0)) <= 511 and int(m.min(initial=0)) >= 0
    m = m.astype(np.uint32)
    return np.ascontiguousarray(m[..., 0] | m[..., 1] << 9 | m[..., 2] << 18 | e.astype(np.uint32) << 27).astype(np.uint32)


def pack(rgb, fmt):
    """(H, W, 3) float -> (H, W) uint32 dwords of `fmt`"""
    return pack_r11g11b10f(rgb) if fmt == R11G11B10F else pack_rgb9e5(rgb)
