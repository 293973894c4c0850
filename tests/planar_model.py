"""The numpy model of the planar YCbCr formats (include/hydrium_amd.h, csrc/hyd_sample_fmt.h 512 ..., csrc/hip/hydk_chroma.h),
on top of yuv_model and chroma_model: sample format = 512 + matrix + 4 * subsampling + 16 * filter; each chroma plane is
upsampled by itself with the taps written out as the header states them (4:2:2: the horizontal ones only), then converted.
The tests hold the library to the reference's file for the RGB8 picture this model makes.

Also a forward RGB8 -> planes helper, which only manufactures realistic inputs and is not under test."""
import numpy as np

import chroma_model as cm
import yuv_model as ym

FIRST_FORMAT = 512
S420, S422, S444 = 0, 1, 2
SUBS = (S420, S422, S444)
SUB_NAMES = ("i420", "i422", "i444")
INFIX = ("", "c", "l")
# (subsampling, filter) pairs that name a format: 4:4:4 has nothing to interpolate
FORMS = tuple((s, f) for f in cm.FILTERS for s in SUBS if not (s == S444 and f))
FAMILY = tuple(FIRST_FORMAT + m + 4 * s + 16 * f for s, f in FORMS for m in ym.MATRICES)
INTERPOLATED = tuple(f for f in FAMILY if (f - FIRST_FORMAT) >> 4)
assert len(FAMILY) == 28 and len(INTERPOLATED) == 16


def sample_fmt(matrix, sub, filt):
    assert matrix in ym.MATRICES and (sub, filt) in FORMS
    return FIRST_FORMAT + matrix + 4 * sub + 16 * filt


def matrix_of(fmt):
    return (fmt - FIRST_FORMAT) & 3


def sub_of(fmt):
    return ((fmt - FIRST_FORMAT) >> 2) & 3


def filter_of(fmt):
    return (fmt - FIRST_FORMAT) >> 4


def is_format(fmt):
    return FIRST_FORMAT <= fmt < FIRST_FORMAT + 48 and (sub_of(fmt), filter_of(fmt)) in FORMS


def name_of(fmt):
    return f"{SUB_NAMES[sub_of(fmt)]}{INFIX[filter_of(fmt)]}-{ym.NAMES[matrix_of(fmt)]}"


def shifts(sub):
    """(sx, sy): log2 of the pixels a chroma sample spans across and down"""
    return (0 if sub == S444 else 1), (1 if sub == S420 else 0)


def chroma_shape(sub, w, h):
    """(ch, cw) of a w x h picture"""
    sx, sy = shifts(sub)
    return (h + sy) >> sy, (w + sx) >> sx


def upsample(sub, filt, plane, w, h):
    """plane (ch, cw) uint8 -> (h, w) uint8: that component of every pixel of the w x h picture"""
    ch, cw = chroma_shape(sub, w, h)
    assert plane.shape == (ch, cw) and (sub, filt) in FORMS
    sx, sy = shifts(sub)
    c = plane.astype(np.int32)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    if filt == cm.NEAREST:
        return plane[y >> sy, x >> sx]
    if sub == S420:  # the taps of hydk_chroma.h on the plane as it stands
        cy, cx = y >> 1, x >> 1
        vy = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
        if filt == cm.CENTRE:
            hx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
            out = (9 * c[cy, cx] + 3 * c[cy, hx] + 3 * c[vy, cx] + c[vy, hx] + 8) >> 4
        else:
            hx = np.minimum(cx + 1, cw - 1)
            even = (3 * c[cy, cx] + c[vy, cx] + 2) >> 2
            odd = (3 * (c[cy, cx] + c[cy, hx]) + c[vy, cx] + c[vy, hx] + 4) >> 3
            out = np.where((x & 1).astype(bool), odd, even)
    else:  # 4:2:2: horizontal only
        cx = x >> 1
        if filt == cm.CENTRE:
            hx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
            out = (3 * c[y, cx] + c[y, hx] + 2) >> 2
        else:
            hx = np.minimum(cx + 1, cw - 1)
            out = np.where((x & 1).astype(bool), (c[y, cx] + c[y, hx] + 1) >> 1, c[y, cx])
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def expected_rgb(planes, matrix, sub, filt):
    """planes = (y (H, W), u (ch, cw), v (ch, cw)) uint8 -> the (H, W, 3) uint8 picture the format stands for"""
    y, u, v = planes
    h, w = y.shape
    return np.ascontiguousarray(ym.yuv_to_rgb(matrix, y, upsample(sub, filt, u, w, h), upsample(sub, filt, v, w, h)))


def planes_of_rgb(rgb, matrix, sub):
    """a realistic planar picture from an RGB8 one (float arithmetic, box chroma): input manufacture only"""
    kr, kb = ym.KR_KB[matrix]
    kg = 1.0 - kr - kb
    p = rgb.astype(np.float64)
    luma = kr * p[..., 0] + kg * p[..., 1] + kb * p[..., 2]
    cb, cr = (p[..., 2] - luma) / (2 * (1 - kb)), (p[..., 0] - luma) / (2 * (1 - kr))
    h, w = luma.shape
    sx, sy = shifts(sub)
    ch, cw = chroma_shape(sub, w, h)

    def box(a):
        a = np.pad(a, ((0, (ch << sy) - h), (0, (cw << sx) - w)), mode="edge")
        return a.reshape(ch, 1 << sy, cw, 1 << sx).mean((1, 3))

    if ym.LIMITED[matrix]:
        y, u, v = 16 + luma * 219 / 255, 128 + box(cb) * 224 / 255, 128 + box(cr) * 224 / 255
    else:
        y, u, v = luma, 128 + box(cb), 128 + box(cr)
    q = lambda a: np.ascontiguousarray(np.clip(np.rint(a), 0, 255).astype(np.uint8))
    return q(y), q(u), q(v)


# ---- the C side's predicates (csrc/hyd_sample_fmt.h) as a table: what tests/c/planar_formats.cc is held to ----
def predicate_row(fmt):
    """(is_planar_yuv, sub, filter, matrix, is_planar_interp, bytes, is_device, is_host) of one number; sub, filter and matrix
    are 0 where the number is no planar format"""
    planar = is_format(fmt)
    nv12 = 16 <= fmt < 64 and (fmt - 16) & 15 < 4
    p016 = 80 <= fmt <= 243 and 16 <= (fmt & 63) and ((fmt & 63) - 16) & 15 < 4 and (fmt & 63) < 64
    nbytes = 1 if (fmt == 0 or nv12 or planar) else 2 if (fmt in (1, 3, 4) or p016) else 4 if fmt == 2 else 0
    return (int(planar), sub_of(fmt) if planar else 0, filter_of(fmt) if planar else 0, matrix_of(fmt) if planar else 0,
            int(planar and filter_of(fmt) != 0), nbytes, int(0 <= fmt <= 4 or nv12 or p016 or planar), int(0 <= fmt <= 2))
