"""The numpy model of the NV12 formats' conversion (include/hydrium_amd.h, csrc/hip/hydk_yuv.h): the fixed-point formula in
int64, nearest-neighbour chroma.  The tests hold the library to the reference's file for the RGB8 picture this model makes.

Also a forward RGB8 -> NV12 helper, which only manufactures realistic inputs and is not under test."""
import numpy as np

MATRICES = (0, 1, 2, 3)  # BT709, BT709_FULL, BT601, BT601_FULL: sample format - 16
NAMES = ("bt709", "bt709-full", "bt601", "bt601-full")
FIRST_FORMAT = 16
# yo, cy, crv, cgu, cgv, cbu
TABLE = (
    (16, 19077, 29372, 3494, 8731, 34610),
    (0, 16384, 25802, 3069, 7670, 30402),
    (16, 19077, 26149, 6419, 13320, 33050),
    (0, 16384, 22970, 5638, 11700, 29032),
)
KR_KB = ((0.2126, 0.0722), (0.2126, 0.0722), (0.299, 0.114), (0.299, 0.114))
LIMITED = (True, False, True, False)


def real_coefficients(matrix):
    """(yo, cy, crv, cgu, cgv, cbu) as real numbers, from Kr, Kb and the range"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if LIMITED[matrix] else (1.0, 1.0)
    return (16 if LIMITED[matrix] else 0, sy, 2 * (1 - kr) * sc, 2 * (1 - kb) * kb / kg * sc, 2 * (1 - kr) * kr / kg * sc, 2 * (1 - kb) * sc)


def yuv_to_rgb(matrix, y, u, v):
    """arrays of Y, U, V (any integer type, one shape) -> uint8 array of that shape + (3,)"""
    yo, cy, crv, cgu, cgv, cbu = TABLE[matrix]
    c, d, e = np.asarray(y, np.int64) - yo, np.asarray(u, np.int64) - 128, np.asarray(v, np.int64) - 128
    r = (cy * c + crv * e + 8192) >> 14
    g = (cy * c - cgu * d - cgv * e + 8192) >> 14
    b = (cy * c + cbu * d + 8192) >> 14
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def yuv_to_rgb_real(matrix, y, u, v):
    """the clamped real-valued conversion, float64, unrounded"""
    yo, sy, crv, cgu, cgv, cbu = real_coefficients(matrix)
    c, d, e = np.asarray(y, np.float64) - yo, np.asarray(u, np.float64) - 128, np.asarray(v, np.float64) - 128
    return np.clip(np.stack([sy * c + crv * e, sy * c - cgu * d - cgv * e, sy * c + cbu * d], -1), 0.0, 255.0)


def all_triples(lo=0, hi=256):
    """(n, 3) uint8: every (Y, U, V) with lo <= Y < hi, U and V over 0 ... 255"""
    y, u, v = np.meshgrid(np.arange(lo, hi, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.ascontiguousarray(np.stack([y, u, v], -1).reshape(-1, 3))


def expected_rgb(nv12, matrix):
    """nv12 = (y (H, W) uint8, uv (ceil(H / 2), ceil(W / 2), 2) uint8) -> the (H, W, 3) uint8 picture the formats stand for"""
    y, uv = nv12
    h, w = y.shape
    assert uv.shape == (-(-h // 2), -(-w // 2), 2)
    up = np.repeat(np.repeat(uv, 2, 0), 2, 1)[:h, :w]
    return np.ascontiguousarray(yuv_to_rgb(matrix, y, up[..., 0], up[..., 1]))


def nv12_of_rgb(rgb, matrix):
    """a realistic NV12 picture from an RGB8 one (float arithmetic, 2 x 2 box chroma): input manufacture only"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    p = rgb.astype(np.float64)
    luma = kr * p[..., 0] + kg * p[..., 1] + kb * p[..., 2]
    cb, cr = (p[..., 2] - luma) / (2 * (1 - kb)), (p[..., 0] - luma) / (2 * (1 - kr))
    h, w = luma.shape
    pad = lambda a: np.pad(a, ((0, h % 2), (0, w % 2)), mode="edge")
    box = lambda a: pad(a).reshape((h + 1) // 2, 2, (w + 1) // 2, 2).mean((1, 3))
    if LIMITED[matrix]:
        y, u, v = 16 + luma * 219 / 255, 128 + box(cb) * 224 / 255, 128 + box(cr) * 224 / 255
    else:
        y, u, v = luma, 128 + box(cb), 128 + box(cr)
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(q(y)), np.ascontiguousarray(np.stack([q(u), q(v)], -1))
