"""The numpy model of the NV12 formats with interpolated chroma (include/hydrium_amd.h, csrc/hip/hydk_chroma.h), on top of
yuv_model: the definition's taps written out as the header states them, in int32 (no sum exceeds 16 * 255), with the
clamps at the picture's edges.  The tests hold the library to the reference's file for the RGB8 picture this model makes."""
import numpy as np

import yuv_model as ym

NEAREST, CENTRE, LEFT = 0, 1, 2
FILTERS = (NEAREST, CENTRE, LEFT)
FILTER_NAMES = ("nearest", "centre", "left")


def sample_fmt(matrix, filt):
    return ym.FIRST_FORMAT + matrix + 16 * filt


def matrix_of(fmt):
    return (fmt - ym.FIRST_FORMAT) & 3


def filter_of(fmt):
    return (fmt - ym.FIRST_FORMAT) >> 4


def upsample(filt, uv, w, h):
    """uv (ceil(h / 2), ceil(w / 2), 2) uint8 -> (h, w, 2) uint8: U', V' of every pixel of the w x h picture"""
    ch, cw = -(-h // 2), -(-w // 2)
    assert uv.shape == (ch, cw, 2) and filt in FILTERS
    c = uv.astype(np.int32)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    cy, cx = y >> 1, x >> 1
    if filt == NEAREST:
        return uv[cy, cx]
    vy = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    if filt == CENTRE:
        hx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
        out = (9 * c[cy, cx] + 3 * c[cy, hx] + 3 * c[vy, cx] + c[vy, hx] + 8) >> 4
    else:
        hx = np.minimum(cx + 1, cw - 1)
        even = (3 * c[cy, cx] + c[vy, cx] + 2) >> 2
        odd = (3 * (c[cy, cx] + c[cy, hx]) + c[vy, cx] + c[vy, hx] + 4) >> 3
        out = np.where((x & 1)[..., None].astype(bool), odd, even)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def expected_rgb(planes, matrix, filt):
    """planes = (y (H, W) uint8, uv (ceil(H / 2), ceil(W / 2), 2) uint8) -> the (H, W, 3) uint8 picture the format stands for"""
    y, uv = planes
    h, w = y.shape
    up = upsample(filt, uv, w, h)
    return np.ascontiguousarray(ym.yuv_to_rgb(matrix, y, up[..., 0], up[..., 1]))
