"""ctypes binding of the additive device-level C-ABI (include/hydrium_amd.h).

This is plumbing for tests, ``bench.py`` and the multi-GPU driver: it hands raw device pointers
(from torch tensors) to the HIP hot path and reads results back.  There is no CPU fallback — if the
library or a GPU is missing, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import api

MAX_CLUSTERS = 9
ALPHABET = 128
GROUPS_PER_LFG = 64
K_NAMES = ("transform_tokenize", "build_tables", "rans_encode", "pack_sections", "lf_coder")
LF_INFO_DTYPE = np.dtype([("bit_count", "<u4"), ("alphabet", "<u4"), ("run_pairs", "<u4"), ("error", "<u4"),
                          ("offset", "<u4"), ("reserved", "<u4", (3,)), ("lengths", "u1", (384,))])
LF_BITWORDS = 3 * 256 * 256 * 2 + 2                     # HYDK_LF_BITWORDS
LF_CODES = 384  # compact token space of the LF-coefficient stream (include/hydrium_amd.h HYDAMD_LF_CODES)

FMT_OF_DTYPE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}
# device pixels only (include/hydrium_amd.h, HYDAMD_FLOAT16 / HYDAMD_BFLOAT16): half-precision samples, widened exactly on load
FLOAT16 = 3
BFLOAT16 = 4
# device pixels only: YCbCr pictures, converted in fixed point right after the load.  ONE RULE names them all (csrc/hyd_sample_fmt.h):
# sample format = base + matrix + 4 * subsampling + 16 * filter + 64 * depth.  Base 16: a Y plane and a half-resolution plane of
# (U, V) pairs — NV12 at depth 0, P010 / P012 / P016 (16-bit words, MSB-aligned) at depth 1, 2, 3; base 512: PLANAR, 8 bits in three
# planes of their own (I420, I422, I444); base 2048: the same three planes in 16-bit words of 10, 12 or 16 bits, LSB-aligned (libyuv's
# names: I010, I210, I410 ...); base 8192: PACKED 4:2:2, 8 bits in one plane of Y, U, Y, V groups (YUY2 / UYVY / YVYU / VYUY: the byte order
# is what the three pointers spell), subsampling and depth 0; base 32768: the same groups in 16-bit words of 10, 12 or 16 bits, MSB-aligned
# (Y210 / Y212 / Y216), subsampling 0 and depth 1, 2, 3; base 131072: ONE DWORD A PIXEL, three 10-bit fields — Y410 at subsampling 2 (4:4:4)
# and depth 1, and at the base's depth-0 corner RGB10A2 (131072) and BGR10A2 (131073), which are no YCbCr; base 524288: FOUR SAMPLES A PIXEL, Y, U, V and
# an ignored fourth, subsampling 2 (4:4:4) — AYUV (bytes in a dword) at depth 0, Y412 / Y416 (MSB-aligned words in a qword) at depth 2, 3; depth 1
# names nothing (that surface is Y410).  matrix 0 ... 3: BT.709 limited range (HD video), BT.709 full, BT.601 limited (SD video), BT.601
# full (what a JPEG decoder leaves: JFIF).  filter: nearest, or INTERPOLATED for centre-sited chroma (C: JPEG / JFIF, MPEG-1) or
# left-sited (L: MPEG-2, H.264, HEVC, AV1 default) — csrc/hip/hydk_chroma.h; 4:4:4 has nearest chroma only.
CHROMA_FILTERS = {"nearest": 0, "centre": 1, "center": 1, "left": 2}
P016_DEPTHS = {10: 1, 12: 2, 16: 3}
PLANAR_SUBSAMPLINGS = {"420": 0, "422": 1, "444": 2}


def ycbcr_fmt(base: int, matrix: int = 0, sub: int = 0, filt: int = 0, depth: int = 0) -> int:
    return base + matrix + 4 * sub + 16 * filt + 64 * depth


def ycbcr_fields(fmt: int):
    """(base, matrix, subsampling, filter, depth) of a YCbCr sample format"""
    base = 524288 if fmt >= 524288 else 131072 if fmt >= 131072 else 32768 if fmt >= 32768 else 8192 if fmt >= 8192 else 2048 if fmt >= 2048 else 512 if fmt >= 512 else 16
    n = int(fmt) - base
    return base, n & 3, (n >> 2) & 3, (n >> 4) & 3, n >> 6


_stems = [("NV12", 16, 0, 0)] + [(f"P0{b}", 16, 0, d) for b, d in P016_DEPTHS.items()] + \
    [(f"I{s}", 512, k, 0) for s, k in PLANAR_SUBSAMPLINGS.items()] + \
    [(f"I{s[2]}{b}", 2048, k, d) for b, d in P016_DEPTHS.items() for s, k in PLANAR_SUBSAMPLINGS.items()] + [("YUY2", 8192, 0, 0)] + \
    [(f"Y2{b}", 32768, 0, d) for b, d in P016_DEPTHS.items()] + [("Y410", 131072, 2, 1)] + \
    [("AYUV", 524288, 2, 0), ("Y412", 524288, 2, 2), ("Y416", 524288, 2, 3)]
for _stem, _base, _sub, _depth in _stems:  # NV12_BT709 = 16 ... I416_BT601_FULL = 2251, YUY2_BT709 = 8192 ..., Y210_BT709 = 32832 ..., as include/hydrium_amd.h has them
    for _infix, _filter in (("", 0), ("C", 1), ("L", 2)):
        for _matrix, _name in enumerate(("BT709", "BT709_FULL", "BT601", "BT601_FULL")):
            if not (_sub == 2 and _filter):
                globals()[f"{_stem}{_infix}_{_name}"] = ycbcr_fmt(_base, _matrix, _sub, _filter, _depth)
NV12_FORMATS, NV12_CENTER_FORMATS, NV12_LEFT_FORMATS = (tuple(ycbcr_fmt(16, m, 0, f) for m in range(4)) for f in range(3))
NV12_FAMILY = NV12_FORMATS + NV12_CENTER_FORMATS + NV12_LEFT_FORMATS
P010_FORMATS, P012_FORMATS, P016_FORMATS = (tuple(ycbcr_fmt(16, m, 0, 0, d) for m in range(4)) for d in (1, 2, 3))  # nearest chroma
P016_FAMILY = tuple(ycbcr_fmt(16, m, 0, f, d) for d in (1, 2, 3) for f in range(3) for m in range(4))
PLANAR_FAMILY = tuple(ycbcr_fmt(512, m, s, f) for f in range(3) for s in range(3) for m in range(4) if not (s == 2 and f))
PLANAR16_FAMILY = tuple(ycbcr_fmt(2048, *ycbcr_fields(f)[1:4], d) for d in (1, 2, 3) for f in PLANAR_FAMILY)
PACKED_FAMILY = tuple(ycbcr_fmt(8192, m, 0, f) for f in range(3) for m in range(4))
# (U, V) byte offsets from the first Y byte, by byte order (include/hydrium_amd.h: the order is read off the pointers)
PACKED_ORDERS = {"yuyv": (1, 3), "yuy2": (1, 3), "yvyu": (3, 1), "uyvy": (-1, 1), "vyuy": (1, -1)}
# packed 4:2:2 in 16-bit words, Y210 / Y212 / Y216: the same four orders, the offsets in words ("y210": Y210's own, Y U Y V)
PACKED16_FAMILY = tuple(ycbcr_fmt(32768, m, 0, f, d) for d in (1, 2, 3) for f in range(3) for m in range(4))
PACKED16_ORDERS = dict(PACKED_ORDERS, y210=(1, 3), y212=(1, 3), y216=(1, 3))
del PACKED16_ORDERS["yuy2"]
# one dword a pixel: the two RGB orders, then Y410's four matrices (Y410_BT709 = 131144 ...)
RGB10A2, BGR10A2 = 131072, 131073
RGB10_ORDERS = {"rgb": RGB10A2, "bgr": BGR10A2}
Y410_FORMATS = tuple(ycbcr_fmt(131072, m, 2, 0, 1) for m in range(4))
DWORD_FAMILY = (RGB10A2, BGR10A2) + Y410_FORMATS
# four samples a pixel, the fourth ignored: AYUV_BT709 = 524296 ..., Y412_BT709 = 524424 ..., Y416_BT709 = 524488 ...
AYUV_FORMATS, Y412_FORMATS, Y416_FORMATS = (tuple(ycbcr_fmt(524288, m, 2, 0, d) for m in range(4)) for d in (0, 2, 3))
QUAD_FAMILY = AYUV_FORMATS + Y412_FORMATS + Y416_FORMATS
# three unsigned floats in one dword, the float render targets (no YCbCr, a base of their own: 2 ** 23): storage forms of the FLOAT class
R11G11B10F, RGB9E5 = 8388608, 8388609
UFLOAT_FAMILY = (R11G11B10F, RGB9E5)


def planar_fmt(matrix: int = NV12_BT709, subsampling="420", chroma=None) -> int:
    """The sample format of a planar YCbCr picture: ``matrix`` one of NV12_FORMATS (the matrix and range), ``subsampling``
    "420", "422" or "444", ``chroma`` None / "nearest", "centre" or "left" ("444" has nothing to interpolate)."""
    if int(matrix) not in NV12_FORMATS:
        raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL")
    if str(subsampling) not in PLANAR_SUBSAMPLINGS:
        raise ValueError("subsampling is '420', '422' or '444'")
    if chroma is not None and chroma not in CHROMA_FILTERS:
        raise ValueError("chroma is 'nearest', 'centre' or 'left'")
    sub, filt = PLANAR_SUBSAMPLINGS[str(subsampling)], CHROMA_FILTERS[chroma or "nearest"]
    if sub == 2 and filt:
        raise ValueError("4:4:4 has a chroma sample for every pixel: no chroma filter")
    return ycbcr_fmt(512, ycbcr_fields(matrix)[1], sub, filt)


def planar16_fmt(matrix: int = NV12_BT709, subsampling="420", chroma=None, depth: int = 10) -> int:
    """The sample format of a planar YCbCr picture of 16-bit words: planar_fmt's arguments and ``depth`` 10, 12 or 16."""
    if depth not in P016_DEPTHS:
        raise ValueError("depth is 10, 12 or 16")
    return ycbcr_fmt(2048, *ycbcr_fields(planar_fmt(matrix, subsampling, chroma))[1:4], P016_DEPTHS[depth])


class Nv12:
    """An NV12 picture in device memory, accepted wherever an image tensor is (DeviceContext.encode_image_tensor and
    encode_image_batch, FrameBatch, MixedBatch, TiledImage, MultiFrame).

    ``y``: uint8 tensor (H, W) with unit column stride.  ``uv``: uint8 tensor (ceil(H / 2), ceil(W / 2), 2) with strides
    (pitch, 2, 1), U first; its pitch is the Y plane's (NV12 has one pitch).  ``matrix``: one of NV12_FORMATS.  A crop of a
    larger surface must start on even coordinates (y[y0:, x0:] with uv[y0 // 2:, x0 // 2:]).

    ``chroma``: "nearest" (every 2 x 2 block shares its pair), "centre" or "left" — interpolated, for centre- or left-sited
    chroma, clamped at the edges of THIS picture (a crop's edges replicate).  Or give ``matrix`` as one of the twelve
    numbers of NV12_FAMILY and leave ``chroma`` out."""

    def __init__(self, y, uv, matrix: int = NV12_BT709, chroma=None):
        if int(matrix) not in NV12_FAMILY:
            raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL (or NV12C_*, NV12L_*)")
        if chroma is not None:
            if chroma not in CHROMA_FILTERS:
                raise ValueError("chroma is 'nearest', 'centre' or 'left'")
            if int(matrix) not in NV12_FORMATS and ycbcr_fields(matrix)[3] != CHROMA_FILTERS[chroma]:
                raise ValueError("matrix names another chroma filter than chroma does")
            matrix = ycbcr_fmt(16, ycbcr_fields(matrix)[1], 0, CHROMA_FILTERS[chroma])
        if y.element_size() != 1 or uv.element_size() != 1 or y.dim() != 2 or uv.dim() != 3:
            raise ValueError("NV12 planes are 8-bit: y (H, W), uv (ceil(H / 2), ceil(W / 2), 2)")
        h, w = y.shape
        if h < 1 or w < 1 or tuple(uv.shape) != (-(-h // 2), -(-w // 2), 2):
            raise ValueError("the chroma plane of an (H, W) picture is (ceil(H / 2), ceil(W / 2), 2)")
        if y.stride(1) != 1 or (uv.stride(1), uv.stride(2)) != (2, 1):
            raise ValueError("NV12 planes have unit column stride: y (pitch, 1), uv (pitch, 2, 1)")
        if uv.shape[0] > 1 and h > 1 and uv.stride(0) != y.stride(0):
            raise ValueError("the two planes of an NV12 picture share one pitch")
        self.y, self.uv, self.sample_fmt = y, uv, int(matrix)
        self.height, self.width = int(h), int(w)
        self.pitch = int(y.stride(0) if h > 1 else uv.stride(0) if uv.shape[0] > 1 else max(y.stride(0), uv.stride(0)))

    @classmethod
    def from_surface(cls, buf, width: int, height: int, pitch: int, chroma_offset: int, matrix: int = NV12_BT709, chroma=None):
        """A decoder's single allocation: ``buf`` a 1-D uint8 tensor, Y rows at 0, pitch, 2 * pitch ..., chroma rows at
        chroma_offset, chroma_offset + pitch ... (bytes)."""
        y = buf.as_strided((height, width), (pitch, 1), 0)
        uv = buf.as_strided((-(-height // 2), -(-width // 2), 2), (pitch, 2, 1), chroma_offset)
        return cls(y, uv, matrix, chroma)

    @property
    def shape(self):
        return (self.height, self.width, 3)

    pixel_stride = 1  # what the C API's pixel_stride argument takes for this picture

    def pointers(self):
        """src[0 ... 2] of the C API: Y, U, V = U + 1."""
        u = self.uv.data_ptr()
        return [self.y.data_ptr(), u, u + 1]


class P016(Nv12):
    """A P010 / P012 / P016 picture in device memory — NV12's two planes in 16-bit words, the significant bits MSB-aligned —
    accepted wherever an Nv12 object is.

    ``y``: (H, W) tensor of a 2-byte integer dtype with unit column stride.  ``uv``: (ceil(H / 2), ceil(W / 2), 2) of the same
    kind with strides (pitch, 2, 1) in words, U first; its pitch is the Y plane's.  ``matrix``: one of the four NV12_FORMATS
    (the matrix and range), ``chroma`` as Nv12's, ``depth`` 10, 12 or 16 — or ``matrix`` one of the 36 numbers of P016_FAMILY,
    which names all three.  The words are used as stored: low bits below the depth are not masked.  A crop starts on even
    coordinates."""

    def __init__(self, y, uv, matrix: int = NV12_BT709, chroma=None, depth: int = 10):
        matrix = int(matrix)
        if matrix in P016_FAMILY:
            if chroma is not None and ycbcr_fields(matrix)[3] != CHROMA_FILTERS.get(chroma, -1):
                raise ValueError("matrix names another chroma filter than chroma does")
            fmt = matrix
        else:
            if matrix not in NV12_FORMATS:
                raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL (or a P010 / P012 / P016 format)")
            if depth not in P016_DEPTHS:
                raise ValueError("depth is 10, 12 or 16")
            if chroma is not None and chroma not in CHROMA_FILTERS:
                raise ValueError("chroma is 'nearest', 'centre' or 'left'")
            fmt = ycbcr_fmt(16, ycbcr_fields(matrix)[1], 0, CHROMA_FILTERS[chroma or "nearest"], P016_DEPTHS[depth])
        names = [str(t.dtype).rpartition(".")[2] for t in (y, uv)]
        if y.element_size() != 2 or uv.element_size() != 2 or y.dim() != 2 or uv.dim() != 3 or \
                any(n.startswith(("float", "bfloat", "complex")) for n in names):
            raise ValueError("P010 / P016 planes are 16-bit integers: y (H, W), uv (ceil(H / 2), ceil(W / 2), 2)")
        h, w = y.shape
        if h < 1 or w < 1 or tuple(uv.shape) != (-(-h // 2), -(-w // 2), 2):
            raise ValueError("the chroma plane of an (H, W) picture is (ceil(H / 2), ceil(W / 2), 2)")
        if y.stride(1) != 1 or (uv.stride(1), uv.stride(2)) != (2, 1):
            raise ValueError("P010 / P016 planes have unit column stride: y (pitch, 1), uv (pitch, 2, 1)")
        if uv.shape[0] > 1 and h > 1 and uv.stride(0) != y.stride(0):
            raise ValueError("the two planes of a P010 / P016 picture share one pitch")
        self.y, self.uv, self.sample_fmt = y, uv, fmt
        self.height, self.width = int(h), int(w)
        self.pitch = int(y.stride(0) if h > 1 else uv.stride(0) if uv.shape[0] > 1 else max(y.stride(0), uv.stride(0)))  # in words

    @classmethod
    def from_surface(cls, buf, width: int, height: int, pitch_bytes: int, chroma_offset_bytes: int, matrix: int = NV12_BT709,
                     chroma=None, depth: int = 10):
        """A decoder's single allocation: ``buf`` a 1-D tensor of 1- or 2-byte integers, Y rows at byte 0, pitch_bytes,
        2 * pitch_bytes ..., chroma rows at chroma_offset_bytes, chroma_offset_bytes + pitch_bytes ...  The pitch and the
        offset are whole words (even)."""
        if pitch_bytes % 2 or chroma_offset_bytes % 2:
            raise ValueError("the pitch and the chroma offset of a P010 / P016 surface are even numbers of bytes")
        if buf.element_size() == 1:
            if buf.dim() != 1 or buf.stride(0) != 1 or buf.data_ptr() % 2 or buf.numel() % 2:
                raise ValueError("a byte buffer holding a P010 / P016 surface is contiguous, 2-byte aligned and of even size")
            import torch

            buf = buf.view(torch.int16)
        elif buf.element_size() != 2:
            raise ValueError("buf holds bytes or 16-bit words")
        pitch = pitch_bytes // 2
        y = buf.as_strided((height, width), (pitch, 1), 0)
        uv = buf.as_strided((-(-height // 2), -(-width // 2), 2), (pitch, 2, 1), chroma_offset_bytes // 2)
        return cls(y, uv, matrix, chroma, depth)

    def pointers(self):
        """src[0 ... 2] of the C API: Y, U, V = U + 2 bytes."""
        u = self.uv.data_ptr()
        return [self.y.data_ptr(), u, u + 2]


class PlanarYuv(Nv12):
    """A planar YCbCr picture in device memory — I420, I422 or I444: 8-bit Y, U and V planes of their own — accepted wherever
    an Nv12 object is.

    ``y``: uint8 tensor (H, W) with unit column stride.  ``u``, ``v``: uint8 tensors (ch, cw) with unit column stride and ONE
    row stride, which need not be half of y's; they may sit in separate allocations, and swapped they read YV12.  cw =
    ceil(W / 2) for "420" and "422" and W for "444"; ch = ceil(H / 2) for "420" and H otherwise.  ``matrix``: one of
    NV12_FORMATS; ``subsampling``: "420", "422" or "444"; ``chroma``: as Nv12's ("444": nearest only).  A crop starts on even
    x, and on even y for "420".  The C API takes the chroma planes' pitch in its pixel_stride argument."""

    def __init__(self, y, u, v, matrix: int = NV12_BT709, subsampling="420", chroma=None):
        fmt = planar_fmt(matrix, subsampling, chroma)
        names = [str(t.dtype).rpartition(".")[2] for t in (y, u, v)]
        if any(t.element_size() != 1 or t.dim() != 2 for t in (y, u, v)) or any(n.startswith(("float", "bool")) for n in names):
            raise ValueError("planar YCbCr planes are 8-bit: y (H, W), u and v (ch, cw)")
        self._planes(y, u, v, fmt, subsampling)

    def _planes(self, y, u, v, fmt, subsampling):
        """the shape, stride and pitch rules of three planes of one sample width"""
        sub = PLANAR_SUBSAMPLINGS[str(subsampling)]
        h, w = y.shape
        cw, ch = (w if sub == 2 else -(-w // 2)), (-(-h // 2) if sub == 0 else h)
        if h < 1 or w < 1 or tuple(u.shape) != (ch, cw) or tuple(v.shape) != (ch, cw):
            raise ValueError(f"the chroma planes of an (H, W) picture of subsampling {subsampling} are ({ch}, {cw})")
        if y.stride(1) != 1 or u.stride(1) != 1 or v.stride(1) != 1:
            raise ValueError("planar YCbCr planes have unit column stride")
        if ch > 1 and u.stride(0) != v.stride(0):
            raise ValueError("the U and V planes share one pitch")
        self.y, self.u, self.v, self.sample_fmt = y, u, v, fmt
        self.height, self.width = int(h), int(w)
        self.pitch = int(y.stride(0)) if h > 1 else max(int(y.stride(0)), w)
        self.pixel_stride = int(u.stride(0)) if ch > 1 else max(int(u.stride(0)), int(v.stride(0)), cw)  # the chroma pitch

    @classmethod
    def from_surface(cls, *args, **kwargs):
        raise TypeError("PlanarYuv takes its three planes")

    def pointers(self):
        """src[0 ... 2] of the C API: Y, U, V."""
        return [self.y.data_ptr(), self.u.data_ptr(), self.v.data_ptr()]


class PackedYuv(Nv12):
    """A packed 4:2:2 YCbCr picture in device memory — YUY2 (YUYV), UYVY, YVYU or VYUY: one plane of 4-byte groups, two pixels
    each — accepted wherever an Nv12 object is.  What rocJPEG's native output is for a 4:2:2 JPEG (order "yuyv", matrix
    NV12_BT601_FULL, chroma "centre").

    ``surface``: 2-D uint8 tensor of H rows with unit element stride, at least 4 * ceil(width / 2) bytes a row; its row stride is
    the pitch.  ``width``: the picture's width in pixels.  ``matrix``: one of NV12_FORMATS (the matrix and range) — or one of the
    twelve numbers of PACKED_FAMILY, with ``chroma`` left out; ``order``: "yuyv" (or "yuy2"), "uyvy", "yvyu", "vyuy"; ``chroma``:
    as Nv12's.  A crop starts on even x: surface[y0:, 2 * x0:]."""

    pixel_stride = 2  # the distance between two Y samples

    def __init__(self, surface, width: int, matrix: int = NV12_BT709, order: str = "yuyv", chroma=None):
        matrix = int(matrix)
        if chroma is not None and chroma not in CHROMA_FILTERS:
            raise ValueError("chroma is 'nearest', 'centre' or 'left'")
        if matrix in PACKED_FAMILY:
            if chroma is not None and ycbcr_fields(matrix)[3] != CHROMA_FILTERS[chroma]:
                raise ValueError("matrix names another chroma filter than chroma does")
            fmt = matrix
        elif matrix in NV12_FORMATS:
            fmt = ycbcr_fmt(8192, ycbcr_fields(matrix)[1], 0, CHROMA_FILTERS[chroma or "nearest"])
        else:
            raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL (or a YUY2 format)")
        if str(order).lower() not in PACKED_ORDERS:
            raise ValueError("order is 'yuyv', 'uyvy', 'yvyu' or 'vyuy'")
        name = str(surface.dtype).rpartition(".")[2]
        if surface.element_size() != 1 or surface.dim() != 2 or name.startswith(("float", "bool")):
            raise ValueError("a packed 4:2:2 surface is 8-bit: (H, at least 4 * ceil(width / 2)) bytes")
        h, row = surface.shape
        width = int(width)
        if h < 1 or width < 1 or row < 4 * -(-width // 2):
            raise ValueError("a row of a packed 4:2:2 picture is 4 * ceil(width / 2) bytes")
        if surface.stride(1) != 1:
            raise ValueError("a packed 4:2:2 surface has unit element stride")
        self.surface, self.sample_fmt, self.order = surface, fmt, str(order).lower()
        self.height, self.width = int(h), width
        self.pitch = int(surface.stride(0)) if h > 1 else max(int(surface.stride(0)), 4 * -(-width // 2))

    @classmethod
    def from_surface(cls, *args, **kwargs):
        raise TypeError("PackedYuv takes its surface")

    def pointers(self):
        """src[0 ... 2] of the C API: the first Y, U and V byte, all in the first group."""
        du, dv = PACKED_ORDERS[self.order]
        y = self.surface.data_ptr() + (1 if du < 0 or dv < 0 else 0)
        return [y, y + du, y + dv]


class PackedYuv16(PackedYuv):
    """A packed 4:2:2 YCbCr picture of 16-bit words in device memory — Y210, Y212 or Y216, what a VA-API or D3D decoder leaves for
    4:2:2 10-bit HEVC and ffmpeg's y210le / y212le / y216le: one plane of groups of four words, two pixels each, ``depth`` 10, 12
    or 16 significant bits MSB-aligned (the low bits count as stored) — accepted wherever a PackedYuv object is.

    ``surface``: 2-D tensor of a 2-byte integer dtype, H rows with unit element stride, at least 4 * ceil(width / 2) words a
    row; its row stride is the pitch, in words.  ``width``: the picture's width in pixels.  ``matrix``: one of NV12_FORMATS (the
    matrix and range) — or one of the 36 numbers of PACKED16_FAMILY, with ``chroma`` and ``depth`` left out; ``order``: "yuyv"
    (or "y210": Y U Y V, the formats' own), "uyvy", "yvyu", "vyuy"; ``chroma``: as Nv12's (video is "left").  A crop starts on
    even x: surface[y0:, 2 * x0:]."""

    def __init__(self, surface, width: int, matrix: int = NV12_BT709, order: str = "yuyv", chroma=None, depth: Optional[int] = None):
        matrix = int(matrix)
        if chroma is not None and chroma not in CHROMA_FILTERS:
            raise ValueError("chroma is 'nearest', 'centre' or 'left'")
        if depth is not None and depth not in P016_DEPTHS:
            raise ValueError("depth is 10, 12 or 16")
        if matrix in PACKED16_FAMILY:
            if chroma is not None and ycbcr_fields(matrix)[3] != CHROMA_FILTERS[chroma]:
                raise ValueError("matrix names another chroma filter than chroma does")
            if depth is not None and ycbcr_fields(matrix)[4] != P016_DEPTHS[depth]:
                raise ValueError("matrix names another depth than depth does")
            fmt = matrix
        elif matrix in NV12_FORMATS:
            fmt = ycbcr_fmt(32768, ycbcr_fields(matrix)[1], 0, CHROMA_FILTERS[chroma or "nearest"], P016_DEPTHS[10 if depth is None else depth])
        else:
            raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL (or a Y210 / Y212 / Y216 format)")
        if str(order).lower() not in PACKED16_ORDERS:
            raise ValueError("order is 'yuyv' (or 'y210'), 'uyvy', 'yvyu' or 'vyuy'")
        name = str(surface.dtype).rpartition(".")[2]
        if surface.element_size() != 2 or surface.dim() != 2 or name.startswith(("float", "bfloat", "complex")):
            raise ValueError("a packed 4:2:2 surface of 16-bit words is (H, at least 4 * ceil(width / 2)) words of a 2-byte integer dtype")
        h, row = surface.shape
        width = int(width)
        if h < 1 or width < 1 or row < 4 * -(-width // 2):
            raise ValueError("a row of a packed 4:2:2 picture is 4 * ceil(width / 2) words")
        if surface.stride(1) != 1:
            raise ValueError("a packed 4:2:2 surface has unit element stride")
        self.surface, self.sample_fmt, self.order = surface, fmt, str(order).lower()
        self.height, self.width = int(h), width
        self.pitch = int(surface.stride(0)) if h > 1 else max(int(surface.stride(0)), 4 * -(-width // 2))  # in words

    @classmethod
    def from_surface(cls, *args, **kwargs):
        raise TypeError("PackedYuv16 takes its surface")

    def pointers(self):
        """src[0 ... 2] of the C API: the first Y, U and V word, all in the first group."""
        du, dv = PACKED16_ORDERS[self.order]
        y = self.surface.data_ptr() + (2 if du < 0 or dv < 0 else 0)
        return [y, y + 2 * du, y + 2 * dv]


class Rgb10(Nv12):
    """An RGB picture of one dword a pixel in device memory — RGB10A2 or BGR10A2: three 10-bit fields and two spare bits, the
    render-target and scan-out format of HDR and deep-colour pipelines (Vulkan A2B10G10R10 / A2R10G10B10, DXGI R10G10B10A2, DRM
    XBGR2101010 / XRGB2101010) — accepted wherever a PackedYuv16 object is.  A field v stands for the 16-bit sample nearest to
    v / 1023; bits 30 and 31 are ignored.

    ``surface``: 2-D tensor of a 4-byte integer dtype, H rows with unit element stride, at least ``width`` dwords a row; its row
    stride is the pitch, in dwords.  ``width``: the picture's width in pixels.  ``order``: "rgb" — R in bits 0 ... 9 — or "bgr" —
    B in bits 0 ... 9.  A crop starts anywhere: surface[y0:, x0:]."""

    pixel_stride = 1  # a sample is the dword

    def __init__(self, surface, width: int, order: str = "rgb"):
        if str(order).lower() not in RGB10_ORDERS:
            raise ValueError("order is 'rgb' or 'bgr'")
        self._surface(surface, width, RGB10_ORDERS[str(order).lower()])
        self.order = str(order).lower()

    def _surface(self, surface, width, fmt):
        """the shape, stride and pitch rules of a surface of one dword a pixel"""
        name = str(surface.dtype).rpartition(".")[2]
        if surface.element_size() != 4 or surface.dim() != 2 or name.startswith(("float", "complex")):
            raise ValueError("a surface of one dword a pixel is (H, at least width) dwords of a 4-byte integer dtype")
        h, row = surface.shape
        width = int(width)
        if h < 1 or width < 1 or row < width:
            raise ValueError("a row of a picture of one dword a pixel is width dwords")
        if surface.stride(1) != 1:
            raise ValueError("a surface of one dword a pixel has unit element stride")
        self.surface, self.sample_fmt = surface, int(fmt)
        self.height, self.width = int(h), width
        self.pitch = int(surface.stride(0)) if h > 1 else max(int(surface.stride(0)), width)  # in dwords

    @classmethod
    def from_surface(cls, *args, **kwargs):
        raise TypeError(f"{cls.__name__} takes its surface")

    def pointers(self):
        """src[0 ... 2] of the C API: the first dword, three times over."""
        p = self.surface.data_ptr()
        return [p, p, p]


class Y410(Rgb10):
    """A Y410 picture in device memory — packed 4:4:4 YCbCr of 10 bits, one dword a pixel with U in bits 0 ... 9, Y in 10 ... 19
    and V in 20 ... 29 (DRM XVYU2101010): what a VA-API or D3D decoder leaves for 4:4:4 10-bit HEVC — accepted wherever an Rgb10
    object is.  The picture is the I410 picture of the three fields.

    ``surface``, ``width``: as Rgb10's.  ``matrix``: one of NV12_FORMATS (the matrix and range) or one of Y410_FORMATS."""

    def __init__(self, surface, width: int, matrix: int = NV12_BT709):
        matrix = int(matrix)
        if matrix not in Y410_FORMATS and matrix not in NV12_FORMATS:
            raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL (or a Y410 format)")
        self._surface(surface, width, Y410_FORMATS[ycbcr_fields(matrix)[1]])


class Ayuv(Nv12):
    """An AYUV picture in device memory — packed 4:4:4 YCbCr of 8 bits, one dword a pixel holding the bytes V, U, Y, A (DXGI AYUV,
    VA-API AYUV / XYUV, DRM XYUV8888, ffmpeg vuya / vuyx): what a decoder leaves for 4:4:4 8-bit video — accepted wherever a Y410
    object is.  The picture is the I444 picture of the three bytes; the fourth is ignored.

    ``surface``: 2-D tensor of a 4-byte integer dtype, H rows with unit element stride, at least ``width`` pixels a row; or a
    (H, at least width, 4) tensor of a 1-byte integer dtype with unit last stride and pixel stride 4, whose row stride is a whole
    number of pixels.  Its first pixel sits on a 4-byte boundary; its row stride is the pitch.  ``width``: the picture's width in
    pixels.  ``matrix``: one of NV12_FORMATS (the matrix and range) or one of AYUV_FORMATS.  A crop starts anywhere:
    surface[y0:, x0:]."""

    pixel_stride = 1  # a sample is the group
    _group_bytes = 4
    _kind = "AYUV"

    def __init__(self, surface, width: int, matrix: int = NV12_BT709):
        matrix = int(matrix)
        if matrix not in AYUV_FORMATS and matrix not in NV12_FORMATS:
            raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL (or an AYUV format)")
        self._surface(surface, width, AYUV_FORMATS[ycbcr_fields(matrix)[1]])

    def _surface(self, surface, width, fmt):
        """the shape, stride, pitch and alignment rules of a surface of one group of four samples a pixel"""
        group, kind = self._group_bytes, self._kind
        name = str(surface.dtype).rpartition(".")[2]
        if name.startswith(("float", "complex", "bfloat", "bool")) or surface.dim() not in (2, 3) or \
                surface.element_size() != (group if surface.dim() == 2 else group // 4):
            raise ValueError(f"an {kind} surface is (H, at least width) pixels of a {group}-byte integer dtype, or (H, at least width, 4) "
                             f"samples of a {group // 4}-byte integer dtype")
        if surface.dim() == 3 and (surface.shape[2] != 4 or surface.stride(2) != 1 or surface.stride(1) != 4):
            raise ValueError(f"an {kind} surface of samples has four to a pixel, unit sample stride and pixel stride 4")
        if surface.dim() == 2 and surface.stride(1) != 1:
            raise ValueError(f"an {kind} surface has unit element stride")
        h, row = surface.shape[:2]
        width = int(width)
        if h < 1 or width < 1 or row < width:
            raise ValueError(f"a row of an {kind} picture is width pixels")
        per = 1 if surface.dim() == 2 else 4  # elements a pixel
        if int(surface.stride(0)) % per:
            raise ValueError(f"the pitch of an {kind} surface is a whole number of pixels")
        if surface.data_ptr() % group:
            raise ValueError(f"an {kind} surface starts on a {group}-byte boundary")
        self.surface, self.sample_fmt = surface, int(fmt)
        self.height, self.width = int(h), width
        pitch = int(surface.stride(0)) // per
        self.pitch = pitch if h > 1 else max(pitch, width)  # in pixels

    @classmethod
    def from_surface(cls, *args, **kwargs):
        raise TypeError(f"{cls.__name__} takes its surface")

    def pointers(self):
        """src[0 ... 2] of the C API: the first pixel, three times over."""
        p = self.surface.data_ptr()
        return [p, p, p]


class Y416(Ayuv):
    """A Y412 or Y416 picture in device memory — packed 4:4:4 YCbCr of 12 or 16 bits, one qword a pixel holding the 16-bit words
    U, Y, V, A, MSB-aligned (XV36 / XV48, DRM XVYU12_16161616 / XVYU16161616) — accepted wherever an Ayuv object is.  The words
    count as stored; a Y416 picture is the I416 picture of the three words, and the fourth is ignored.

    ``surface``: 2-D tensor of an 8-byte integer dtype, or a (H, at least width, 4) tensor of a 2-byte integer dtype, under Ayuv's
    rules with an 8-byte boundary.  ``width``, ``matrix`` (or one of Y412_FORMATS / Y416_FORMATS): as Ayuv's.  ``depth``: 12 or 16."""

    _group_bytes = 8
    _kind = "Y416"

    def __init__(self, surface, width: int, matrix: int = NV12_BT709, depth: int = 16):
        matrix = int(matrix)
        if depth not in (12, 16):
            raise ValueError("depth is 12 or 16 (10 bits: Y410)")
        formats = Y412_FORMATS if depth == 12 else Y416_FORMATS
        if matrix not in formats and matrix not in NV12_FORMATS:
            raise ValueError("matrix is one of NV12_BT709, NV12_BT709_FULL, NV12_BT601, NV12_BT601_FULL (or a format of that depth)")
        self._surface(surface, width, formats[ycbcr_fields(matrix)[1]])
        self.depth = int(depth)


class R11g11b10f(Rgb10):
    """An R11G11B10F picture in device memory — one dword a pixel of three unsigned floats, R in bits 0 ... 10, G in 11 ... 21, B in
    22 ... 31 (DXGI R11G11B10_FLOAT, Vulkan B10G11R11_UFLOAT_PACK32, GL R11F_G11F_B10F): the HDR scene and post-processing buffer of
    real-time renderers — accepted wherever an Rgb10 object is.  A field is widened exactly to float32 on load; the picture is the
    float32 picture of the widened samples, and an Inf or NaN field is what a non-finite float32 sample is.

    ``surface``: 2-D tensor of a 4-byte integer dtype, H rows with unit element stride, at least ``width`` dwords a row; its row
    stride is the pitch, in dwords.  ``width``: the picture's width in pixels.  A crop starts anywhere: surface[y0:, x0:]."""

    _fmt = R11G11B10F

    def __init__(self, surface, width: int):
        self._surface(surface, width, self._fmt)


class Rgb9e5(R11g11b10f):
    """An RGB9E5 picture in device memory — one dword a pixel of three 9-bit mantissas (R in bits 0 ... 8, G in 9 ... 17, B in
    18 ... 26) and their shared 5-bit exponent (DXGI R9G9B9E5_SHAREDEXP, Vulkan E5B9G9R9_UFLOAT_PACK32, GL RGB9_E5): HDR textures,
    light maps and environment maps — accepted wherever an R11g11b10f object is.  Every dword is a finite picture.

    ``surface``, ``width``: as R11g11b10f's."""

    _fmt = RGB9E5


class PlanarYuv16(PlanarYuv):
    """A planar YCbCr picture of 16-bit words in device memory — I010, I210, I410, I012 ... I416: PlanarYuv's three planes as
    tensors of a 2-byte integer dtype, ``depth`` 10, 12 or 16 significant bits LSB-aligned (bits above the depth are ignored) —
    accepted wherever an Nv12 object is.  Shapes, strides and the one chroma pitch as PlanarYuv's, in words; the C API takes the
    chroma planes' pitch in words in its pixel_stride argument."""

    def __init__(self, y, u, v, matrix: int = NV12_BT709, subsampling="420", chroma=None, depth: int = 10):
        fmt = planar16_fmt(matrix, subsampling, chroma, depth)
        names = [str(t.dtype).rpartition(".")[2] for t in (y, u, v)]
        if any(t.element_size() != 2 or t.dim() != 2 for t in (y, u, v)) or any(n.startswith(("float", "bfloat", "complex")) for n in names):
            raise ValueError("planar YCbCr planes of 10 to 16 bits are 16-bit integers: y (H, W), u and v (ch, cw)")
        self._planes(y, u, v, fmt, subsampling)


def sample_fmt_of(t) -> int:
    """The sample format of a tensor's pixels, by DTYPE (two bytes may be uint16, int16 bits, float16 or bfloat16):
    float16 -> FLOAT16, bfloat16 -> BFLOAT16, float32 -> 2, any other 2-byte type -> 1, any 1-byte type -> 0.
    An Nv12, P016, PlanarYuv, PlanarYuv16, PackedYuv, PackedYuv16, Rgb10, Y410, Ayuv, Y416, R11g11b10f or Rgb9e5 object: its own format."""
    if isinstance(t, Nv12):
        return t.sample_fmt
    name = str(t.dtype).rpartition(".")[2]
    if name == "float16":
        return FLOAT16
    if name == "bfloat16":
        return BFLOAT16
    if name == "float32":
        return 2
    isz = t.element_size()
    if isz in (1, 2) and not name.startswith(("float", "bfloat", "complex")):
        return isz - 1
    raise ValueError(f"no sample format for pixels of type {t.dtype}")


class DeviceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hydamd error {code}: {msg}")
        self.code = code
        self.message = msg


class HydAmdImageDesc(C.Structure):  # include/hydrium_amd.h
    _fields_ = [("src", C.c_void_p * 3), ("row_stride", C.c_ssize_t), ("pixel_stride", C.c_ssize_t), ("width", C.c_size_t),
                ("height", C.c_size_t)]


_dll = None


def dll(path: Optional[str] = None):
    global _dll
    if _dll is None or path is not None:
        p = path or api.DEFAULT_LIB
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} missing: the HIP extension is not built (there is no CPU fallback)")
        from . import preload_hip_runtime

        preload_hip_runtime()
        d = C.CDLL(p)
        vp, i, u, sz = C.c_void_p, C.c_int, C.c_uint, C.c_size_t
        d.hydamd_device_count.restype = i
        d.hydamd_create.restype = vp
        d.hydamd_create.argtypes = [i, i, i, i, C.POINTER(i)]
        d.hydamd_destroy.argtypes = [vp]
        d.hydamd_error.restype = C.c_char_p
        d.hydamd_error.argtypes = [vp]
        d.hydamd_set_stream.argtypes = [vp, vp]
        d.hydamd_get_stream.restype = vp
        d.hydamd_get_stream.argtypes = [vp]
        d.hydamd_uses_register_luts.argtypes = [vp]
        d.hydamd_force_luts.argtypes = [vp, i]
        d.hydamd_xyb_mode.argtypes = [vp]
        d.hydamd_set_xyb_mode.argtypes = [vp, i]
        d.hydamd_begin_frame.argtypes = [vp, u]
        d.hydamd_set_rans_waves.argtypes = [vp, i]
        d.hydamd_set_curve_gathers.argtypes = [vp, i]
        lf_args = [vp, i, C.POINTER(vp), C.c_ssize_t, C.c_ssize_t, i, sz, sz, u]
        d.hydamd_encode_lf_group.argtypes = lf_args
        d.hydamd_encode_lf_group_host.argtypes = lf_args
        d.hydamd_encode_lf_group_at.argtypes = [vp, i, C.POINTER(vp), C.c_ssize_t, C.c_ssize_t, i, sz, sz, sz, sz, sz, sz, u]
        d.hydamd_encode_image.argtypes = [vp, C.POINTER(vp), C.c_ssize_t, C.c_ssize_t, i, sz, sz]
        d.hydamd_debug_shader_clock_mhz.argtypes = [vp, C.POINTER(C.c_double)]
        d.hydamd_encode_image_batch.argtypes = [vp, i, C.POINTER(vp), C.c_ssize_t, C.c_ssize_t, i, sz, sz]
        d.hydamd_begin_batch.argtypes = [vp, u, i]
        d.hydamd_begin_batch_frames.restype = i
        d.hydamd_begin_batch_frames.argtypes = [vp, i, C.POINTER(u)]
        d.hydamd_replay_frame.restype = i
        d.hydamd_replay_frame.argtypes = [vp]
        d.hydamd_finish_frame.argtypes = [vp, i]
        d.hydamd_run_transform.argtypes = [vp, i]
        d.hydamd_run_entropy.argtypes = [vp, i]
        d.hydamd_read_alphabet_max.argtypes = [vp, i, C.POINTER(C.c_uint32)]
        d.hydamd_set_bad_sample_per_slot.restype = i
        d.hydamd_set_bad_sample_per_slot.argtypes = [vp, i]
        d.hydamd_read_bad_slots.restype = i
        d.hydamd_read_bad_slots.argtypes = [vp, i, i, C.POINTER(C.c_uint32)]
        d.hydamd_set_alphabet_floor.argtypes = [vp, C.c_uint32]
        d.hydamd_alphabet_max_device.restype = vp
        d.hydamd_alphabet_max_device.argtypes = [vp]
        d.hydamd_set_alphabet_floor_device.argtypes = [vp, vp]
        d.hydamd_blob_bound.restype = sz
        d.hydamd_blob_bound.argtypes = [vp, i]
        d.hydamd_export_frame.argtypes = [vp, i, vp, sz]
        d.hydamd_export_frame_owned.argtypes = [vp, i, C.POINTER(vp), C.POINTER(sz)]
        d.hydamd_frame_from_blobs.restype = i
        d.hydamd_frame_from_blobs.argtypes = [C.POINTER(api.HYDImageMetadata), i, i, sz, C.POINTER(vp), C.POINTER(sz),
                                              C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_char_p)]
        d.hydamd_frame_from_results.restype = i
        d.hydamd_frame_from_results.argtypes = [
            C.POINTER(api.HYDImageMetadata), i, i, sz, vp, C.POINTER(vp), vp, vp, vp, u, vp, sz, C.c_char_p, sz,
            C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_char_p)]
        d.hydamd_frame_from_streams.restype = i
        d.hydamd_frame_from_streams.argtypes = [
            C.POINTER(api.HYDImageMetadata), i, i, sz, vp, vp, vp, vp, vp, u, C.c_char_p, sz, C.c_char_p, sz,
            C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_char_p)]
        d.hydamd_free.argtypes = [vp]
        d.hydamd_sync.argtypes = [vp]
        d.hydamd_payload_size.restype = sz
        d.hydamd_payload_size.argtypes = [vp]
        d.hydamd_payload_capacity.restype = sz
        d.hydamd_payload_capacity.argtypes = [vp]
        d.hydamd_token_capacity.restype = u
        d.hydamd_token_capacity.argtypes = [vp]
        d.hydamd_overflow_reruns.restype = u
        d.hydamd_overflow_reruns.argtypes = [vp]
        d.hydamd_grown_ahead.restype = u
        d.hydamd_grown_ahead.argtypes = [vp]
        d.hydamd_payload_device.restype = vp
        d.hydamd_payload_device.argtypes = [vp]
        d.hydamd_read_payload.argtypes = [vp, vp, sz]
        d.hydamd_read_sections.argtypes = [vp, i, vp, vp]
        d.hydamd_read_tables.argtypes = [vp, i, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        d.hydamd_read_dc.argtypes = [vp, i, vp, sz, sz]
        d.hydamd_read_symbol_counts.argtypes = [vp, i, vp]
        d.hydamd_read_tokens.argtypes = [vp, i, i, vp, sz]
        d.hydamd_read_debug_plane.argtypes = [vp, i, vp, sz, sz]
        d.hydamd_submit_lf_group.argtypes = [vp, i]
        d.hydamd_run_lf_coder.argtypes = [vp, i, i]
        d.hydamd_sync_lf.argtypes = [vp]
        d.hydamd_set_lf_coder.argtypes = [vp, i]
        d.hydamd_lf_coder.argtypes = [vp]
        d.hydamd_read_lf_stream.argtypes = [vp, i, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        d.hydamd_read_lf_bits.argtypes = [vp, i, vp, sz]
        d.hydamd_read_lf_streams.argtypes = [vp, i, i, vp]
        d.hydamd_lf_payload_size.restype = sz
        d.hydamd_lf_payload_size.argtypes = [vp]
        d.hydamd_lf_payload_device.restype = vp
        d.hydamd_lf_payload_device.argtypes = [vp]
        d.hydamd_read_lf_payload.argtypes = [vp, vp, sz]
        d.hydamd_debug_transform_footprint.restype = C.c_int
        d.hydamd_debug_transform_footprint.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        d.hydamd_debug_lf_code.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        d.hydamd_assembler_create.restype = vp
        d.hydamd_assembler_create.argtypes = [i, C.POINTER(i)]
        d.hydamd_assembler_destroy.argtypes = [vp]
        d.hydamd_assembler_error.restype = C.c_char_p
        d.hydamd_assembler_error.argtypes = [vp]
        d.hydamd_assembler_plan.argtypes = [vp, C.POINTER(api.HYDImageMetadata), i, i, sz, vp, vp, C.c_char_p, sz]
        d.hydamd_assembler_run.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), vp, vp, sz]
        d.hydamd_assembler_result.argtypes = [vp, C.POINTER(sz)]
        d.hydamd_profile.argtypes = [vp, i]
        d.hydamd_profile_read.argtypes = [vp, vp, vp]
        d.hydamd_multi_create.restype = vp
        d.hydamd_multi_create.argtypes = [i, C.POINTER(i), C.POINTER(api.HYDImageMetadata), C.POINTER(i)]
        d.hydamd_multi_destroy.argtypes = [vp]
        d.hydamd_multi_error.restype = C.c_char_p
        d.hydamd_multi_error.argtypes = [vp]
        d.hydamd_multi_context.restype = vp
        d.hydamd_multi_context.argtypes = [vp, i]
        d.hydamd_multi_shard_lf_groups.argtypes = [vp, i, C.POINTER(sz), C.POINTER(sz)]
        d.hydamd_encode_image_multi.argtypes = [vp, C.POINTER(vp), C.c_ssize_t, C.c_ssize_t, i, i]
        d.hydamd_multi_result.argtypes = [vp, C.POINTER(sz)]
        d.hydamd_multi_read.argtypes = [vp, vp, sz]
        d.hydamd_tiled_create.restype = vp
        d.hydamd_tiled_create.argtypes = [i, C.POINTER(api.HYDImageMetadata), i, C.POINTER(i)]
        d.hydamd_tiled_destroy.restype = None
        d.hydamd_tiled_destroy.argtypes = [vp]
        d.hydamd_tiled_error.restype = C.c_char_p
        d.hydamd_tiled_error.argtypes = [vp]
        d.hydamd_encode_image_tiled.restype = i
        d.hydamd_encode_image_tiled.argtypes = [vp, C.POINTER(vp), C.c_ssize_t, C.c_ssize_t, i]
        d.hydamd_tiled_result.restype = i
        d.hydamd_tiled_result.argtypes = [vp, C.POINTER(sz)]
        d.hydamd_tiled_read.restype = i
        d.hydamd_tiled_read.argtypes = [vp, C.POINTER(C.c_uint8), sz]
        d.hydamd_tiled_device.restype = C.POINTER(C.c_uint8)
        d.hydamd_tiled_device.argtypes = [vp]
        d.hydamd_tiled_overflow_reruns.restype = u
        d.hydamd_tiled_overflow_reruns.argtypes = [vp]
        d.hydamd_tiled_device_bytes.restype = sz
        d.hydamd_tiled_device_bytes.argtypes = [vp]
        d.hydamd_context_assembler.restype = vp
        d.hydamd_context_assembler.argtypes = [vp]
        d.hydamd_export_batch_owned.argtypes = [vp, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp)]
        d.hydamd_batch_create.restype = vp
        d.hydamd_batch_create.argtypes = [i, C.POINTER(api.HYDImageMetadata), i, C.c_char_p, sz, C.POINTER(i)]
        d.hydamd_batch_destroy.restype = None
        d.hydamd_batch_destroy.argtypes = [vp]
        d.hydamd_batch_error.restype = C.c_char_p
        d.hydamd_batch_error.argtypes = [vp]
        d.hydamd_encode_batch.restype = i
        d.hydamd_encode_batch.argtypes = [vp, i, C.POINTER(vp), C.c_ssize_t, C.c_ssize_t, i]
        d.hydamd_batch_result.restype = i
        d.hydamd_batch_result.argtypes = [vp, C.POINTER(sz)]
        d.hydamd_batch_offsets.restype = i
        d.hydamd_batch_offsets.argtypes = [vp, C.POINTER(C.c_uint64)]
        d.hydamd_batch_device.restype = C.POINTER(C.c_uint8)
        d.hydamd_batch_device.argtypes = [vp]
        d.hydamd_batch_offsets_device.restype = C.POINTER(C.c_uint64)
        d.hydamd_batch_offsets_device.argtypes = [vp]
        d.hydamd_batch_read.restype = i
        d.hydamd_batch_read.argtypes = [vp, i, C.POINTER(C.c_uint8), sz]
        d.hydamd_batch_overflow_reruns.restype = u
        d.hydamd_batch_overflow_reruns.argtypes = [vp]
        for obj in ("batch", "mixed"):
            f = getattr(d, f"hydamd_{obj}_set_image_errors")
            f.restype, f.argtypes = i, [vp, i]
            f = getattr(d, f"hydamd_{obj}_image_status")
            f.restype, f.argtypes = i, [vp, C.POINTER(C.c_uint32)]
            f = getattr(d, f"hydamd_{obj}_image_status_device")
            f.restype, f.argtypes = C.POINTER(C.c_uint32), [vp]
        d.hydamd_encode_mixed_formats.restype = i
        d.hydamd_encode_mixed_formats.argtypes = [vp, i, C.POINTER(HydAmdImageDesc), C.POINTER(i)]
        d.hydamd_mixed_create.restype = vp
        d.hydamd_mixed_create.argtypes = [i, i, i, C.POINTER(i)]
        d.hydamd_mixed_create_slots.restype = vp
        d.hydamd_mixed_create_slots.argtypes = [i, i, i, i, C.POINTER(i)]
        d.hydamd_mixed_destroy.restype = None
        d.hydamd_mixed_destroy.argtypes = [vp]
        d.hydamd_mixed_error.restype = C.c_char_p
        d.hydamd_mixed_error.argtypes = [vp]
        d.hydamd_encode_mixed.restype = i
        d.hydamd_encode_mixed.argtypes = [vp, i, C.POINTER(HydAmdImageDesc), i]
        d.hydamd_mixed_result.restype = i
        d.hydamd_mixed_result.argtypes = [vp, C.POINTER(sz)]
        d.hydamd_mixed_offsets.restype = i
        d.hydamd_mixed_offsets.argtypes = [vp, C.POINTER(C.c_uint64)]
        d.hydamd_mixed_device.restype = C.POINTER(C.c_uint8)
        d.hydamd_mixed_device.argtypes = [vp]
        d.hydamd_mixed_offsets_device.restype = C.POINTER(C.c_uint64)
        d.hydamd_mixed_offsets_device.argtypes = [vp]
        d.hydamd_mixed_read.restype = i
        d.hydamd_mixed_read.argtypes = [vp, i, C.POINTER(C.c_uint8), sz]
        d.hydamd_mixed_overflow_reruns.restype = u
        d.hydamd_mixed_overflow_reruns.argtypes = [vp]
        if path is not None:
            return d
        _dll = d
    return _dll


class DeviceContext:
    """One HydAmdContext: one GPU, one stream, ``max_lf_groups`` LF-group slots."""

    def __init__(self, device: int = 0, max_lf_groups: int = 1, linear_light: int = 0, debug_planes: bool = False):
        self.d = dll()
        st = C.c_int(0)
        self.h = self.d.hydamd_create(device, max_lf_groups, linear_light, int(debug_planes), C.byref(st))
        if not self.h:
            raise DeviceError(st.value, (self.d.hydamd_error(None) or b"").decode())
        self.max_lf_groups = max_lf_groups

    def close(self):
        if self.h:
            self.d.hydamd_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, code: int) -> int:
        if code != 0:
            raise DeviceError(code, (self.d.hydamd_error(self.h) or b"").decode())
        return code

    # -- control ---------------------------------------------------------------------------------
    def set_stream(self, stream_ptr: Optional[int]):
        self._ck(self.d.hydamd_set_stream(self.h, stream_ptr))

    def get_stream(self) -> int:
        return self.d.hydamd_get_stream(self.h) or 0

    def stream_class(self) -> int:
        """the queue pool of the context's own stream: 0 normal, 1 high, 2 low (hydamd_stream_class)"""
        return int(self.d.hydamd_stream_class(C.c_void_p(self.h)))

    def uses_register_luts(self) -> bool:
        return bool(self.d.hydamd_uses_register_luts(self.h))

    def xyb_mode(self) -> int:
        return self.d.hydamd_xyb_mode(self.h)

    def set_xyb_mode(self, mode: int):
        self._ck(self.d.hydamd_set_xyb_mode(self.h, mode))

    def force_luts(self, use_luts: bool):
        self._ck(self.d.hydamd_force_luts(self.h, int(use_luts)))

    def set_rans_waves(self, waves: int):
        self._ck(self.d.hydamd_set_rans_waves(self.h, waves))

    def set_curve_gathers(self, mode: int):
        """0: one curve of a pixel's six gathered unless the last frame was dense (noise); 1 always; 2 never"""
        self._ck(self.d.hydamd_set_curve_gathers(self.h, mode))

    def begin_frame(self, num_presets: int):
        self._ck(self.d.hydamd_begin_frame(self.h, num_presets))

    def begin_batch(self, num_presets: int, frames: int):
        """One launch group of `frames` independent images of `num_presets` LF groups each, image k in slots
        k * num_presets ...; then encode_lf_group per slot and finish_frame."""
        self._ck(self.d.hydamd_begin_batch(self.h, num_presets, frames))

    def begin_batch_frames(self, lf_groups: Sequence[int]):
        """One launch group of len(lf_groups) independent images, image k of lf_groups[k] LF groups (1..28) in the slots
        behind image k - 1's; then encode_lf_group per slot (preset: the raster index inside the image) and finish_frame."""
        counts = (C.c_uint * max(len(lf_groups), 1))(*[int(n) for n in lf_groups])
        self._ck(self.d.hydamd_begin_batch_frames(self.h, len(lf_groups), counts))

    def encode_lf_group(self, slot: int, ptrs: Sequence[int], row_stride: int, pixel_stride: int, fmt: int,
                        width: int, height: int, preset: int, host: bool = False):
        arr = (C.c_void_p * 3)(*ptrs)
        fn = self.d.hydamd_encode_lf_group_host if host else self.d.hydamd_encode_lf_group
        self._ck(fn(self.h, slot, arr, row_stride, pixel_stride, fmt, width, height, preset))

    def encode_lf_group_at(self, slot: int, ptrs: Sequence[int], row_stride: int, pixel_stride: int, fmt: int, pic_width: int,
                           pic_height: int, x0: int, y0: int, width: int, height: int, preset: int):
        """The LF group at (x0, y0) of a picture whose first pixel ``ptrs`` name (hydamd_encode_lf_group_at): interpolated
        chroma reads across the LF group's edges and clamps at the picture's."""
        arr = (C.c_void_p * 3)(*ptrs)
        self._ck(self.d.hydamd_encode_lf_group_at(self.h, slot, arr, row_stride, pixel_stride, fmt, pic_width, pic_height, x0, y0,
                                                  width, height, preset))

    def finish_frame(self, num_slots: int):
        self._ck(self.d.hydamd_finish_frame(self.h, num_slots))

    def run_transform(self, num_slots: int):
        self._ck(self.d.hydamd_run_transform(self.h, num_slots))

    def run_entropy(self, num_slots: int):
        self._ck(self.d.hydamd_run_entropy(self.h, num_slots))

    def read_alphabet_max(self, slot: int) -> int:
        v = C.c_uint32(0)
        self._ck(self.d.hydamd_read_alphabet_max(self.h, slot, C.byref(v)))
        return v.value

    def set_bad_sample_per_slot(self, on: bool):
        """A non-finite float sample flags its SLOT (read_bad_slots, the slot's record of a view) and is coded as 0.0,
        instead of failing the launch group through the status word.  For LF groups recorded after the call."""
        self._ck(self.d.hydamd_set_bad_sample_per_slot(self.h, int(bool(on))))

    def read_bad_slots(self, count: int, first: int = 0) -> np.ndarray:
        """uint32[count], non-zero where the slot held a non-finite float sample; waits for the frame."""
        out = np.zeros(count, np.uint32)
        self._ck(self.d.hydamd_read_bad_slots(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def set_alphabet_floor(self, floor: int):
        self._ck(self.d.hydamd_set_alphabet_floor(self.h, floor))

    # -- the same exchange and the result hand-over without the host in the loop (multi-GPU) ----------
    def alphabet_max_tensor(self, num_slots: int):
        """int32 CUDA view of the per-slot maxima in the context's memory; order reads behind the context's stream."""
        raw = self._device_view("alpha_max", int(self.d.hydamd_alphabet_max_device(self.h) or 0), self.max_lf_groups * 4)
        return raw.view(__import__("torch").int32)[:num_slots]

    def set_alphabet_floor_device(self, tensor):
        """1-element int32 CUDA tensor the table kernel reads the floor from when it runs (kept alive by the context object)."""
        self._floor_keep = tensor
        self._ck(self.d.hydamd_set_alphabet_floor_device(self.h, tensor.data_ptr() if tensor is not None else None))

    def blob_bound(self, num_slots: int) -> int:
        return int(self.d.hydamd_blob_bound(self.h, num_slots))

    def export_frame(self, num_slots: int, out_tensor):
        """Enqueue the blob of slots [0, num_slots) into a uint8 CUDA tensor (behind the entropy stage, no sync)."""
        self._ck(self.d.hydamd_export_frame(self.h, num_slots, out_tensor.data_ptr(), out_tensor.numel()))

    def export_frame_owned(self, num_slots: int):
        """Enqueue the blob of slots [0, num_slots) as a VIEW in the context's own small buffer (nothing of the frame's bulk
        is copied; for an assembler on the same device and stream).  Returns (device pointer, readable bytes)."""
        p, n = C.c_void_p(0), C.c_size_t(0)
        self._ck(self.d.hydamd_export_frame_owned(self.h, num_slots, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def sync(self):
        self._ck(self.d.hydamd_sync(self.h))

    # -- whole-image helpers -----------------------------------------------------------------------
    def encode_image_tensor(self, img, num_slots_check: bool = True):
        """Enqueue the hot path for every LF group of an interleaved (H, W, 3) torch CUDA tensor.

        The kernels read the tensor's memory asynchronously: the caller must keep it alive (and
        unmodified) until ``sync()``.  An Nv12 object goes the same way."""
        h, w, _ = img.shape
        fmt = sample_fmt_of(img)
        lfx, lfy = -(-w // 2048), -(-h // 2048)
        n = lfx * lfy
        if num_slots_check and n > self.max_lf_groups:
            raise ValueError("context has too few LF-group slots for this image")
        if isinstance(img, Nv12):
            self._ck(self.d.hydamd_encode_image(self.h, (C.c_void_p * 3)(*img.pointers()), img.pitch, img.pixel_stride, fmt, w, h))
            return n
        isz = img.element_size()
        if not getattr(self, "per_lf_group_calls", False):
            # one C call per frame (hydamd_encode_image): eighteen ctypes calls cost the host as much as the GPU needs
            base = img.data_ptr()
            arr = (C.c_void_p * 3)(base, base + isz, base + 2 * isz)
            self._ck(self.d.hydamd_encode_image(self.h, arr, 3 * w, 3, fmt, w, h))
            return n
        self.begin_frame(n)
        base = img.data_ptr()
        for ty in range(lfy):
            for tx in range(lfx):
                x0, y0 = tx * 2048, ty * 2048
                p = base + (y0 * w + x0) * 3 * isz
                self.encode_lf_group(ty * lfx + tx, [p, p + isz, p + 2 * isz], 3 * w, 3, fmt,
                                     min(2048, w - x0), min(2048, h - y0), ty * lfx + tx)
        self.finish_frame(n)
        return n

    def encode_image(self, ptrs: Sequence[int], row_stride: int, pixel_stride: int, fmt: int, width: int, height: int):
        """Enqueue a whole device-resident frame from three bare addresses and strides in samples (hydamd_encode_image):
        every LF group in raster order, slot = raster index = preset."""
        self._ck(self.d.hydamd_encode_image(self.h, (C.c_void_p * 3)(*ptrs), row_stride, pixel_stride, fmt, width, height))

    def encode_image_batch(self, imgs):
        """Enqueue a batch of interleaved (H, W, 3) torch CUDA tensors of one shape as one launch group
        (hydamd_encode_image_batch): frame k in slots k * n ... (k + 1) * n - 1.  Or of Nv12 objects of one shape, pitch
        and matrix."""
        h, w, _ = imgs[0].shape
        fmt = sample_fmt_of(imgs[0])
        n = (-(-w // 2048)) * (-(-h // 2048))
        if n * len(imgs) > self.max_lf_groups:
            raise ValueError("context has too few LF-group slots for this batch")
        ptrs = []
        if isinstance(imgs[0], Nv12):
            for t in imgs:
                assert isinstance(t, Nv12) and (t.shape, t.pitch, t.pixel_stride, t.sample_fmt) == (imgs[0].shape, imgs[0].pitch, imgs[0].pixel_stride, fmt)
                ptrs += t.pointers()
            arr = (C.c_void_p * len(ptrs))(*ptrs)
            self._ck(self.d.hydamd_encode_image_batch(self.h, len(imgs), arr, imgs[0].pitch, imgs[0].pixel_stride, fmt, w, h))
            return n * len(imgs)
        isz = imgs[0].element_size()
        for t in imgs:
            assert t.shape == imgs[0].shape and t.dtype == imgs[0].dtype
            b = t.data_ptr()
            ptrs += [b, b + isz, b + 2 * isz]
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._ck(self.d.hydamd_encode_image_batch(self.h, len(imgs), arr, 3 * w, 3, fmt, w, h))
        return n * len(imgs)

    def encode_image_host(self, img: np.ndarray):
        """Same from a host numpy image, through the pinned staging path."""
        h, w, _ = img.shape
        isz = img.dtype.itemsize
        fmt = FMT_OF_DTYPE[img.dtype]
        lfx, lfy = -(-w // 2048), -(-h // 2048)
        n = lfx * lfy
        self.begin_frame(n)
        base = img.ctypes.data
        for ty in range(lfy):
            for tx in range(lfx):
                x0, y0 = tx * 2048, ty * 2048
                p = base + (y0 * w + x0) * 3 * isz
                self.encode_lf_group(ty * lfx + tx, [p, p + isz, p + 2 * isz], 3 * w, 3, fmt,
                                     min(2048, w - x0), min(2048, h - y0), ty * lfx + tx, host=True)
        self.finish_frame(n)
        return n

    # -- results -----------------------------------------------------------------------------------
    def payload_size(self) -> int:
        return self.d.hydamd_payload_size(self.h)

    def payload_device_ptr(self) -> int:
        return self.d.hydamd_payload_device(self.h) or 0

    def _device_view(self, key: str, ptr: int, capacity: int):
        """uint8 CUDA tensor aliasing `capacity` bytes at `ptr`, made once per buffer: wrapping a raw
        pointer costs torch a pointer-attribute query (~0.5 ms), slicing the cached view nothing."""
        import torch

        cache = self.__dict__.setdefault("_views", {})
        hit = cache.get(key)
        if hit is None or hit[0] != ptr:
            class _View:
                __cuda_array_interface__ = {"shape": (capacity,), "typestr": "|u1", "data": (ptr, False), "version": 2}

            hit = cache[key] = (ptr, torch.as_tensor(_View(), device="cuda"))
        return hit[1]

    def payload_tensor(self):
        """Zero-copy torch uint8 view of the packed HF sections in HBM (valid until the next frame)."""
        cap = int(self.d.hydamd_payload_capacity(self.h))  # pointer and capacity change if a frame outgrew the buffers
        return self._device_view(("payload", cap), self.payload_device_ptr(), cap)[: self.payload_size()]

    def token_capacity(self) -> int:
        return int(self.d.hydamd_token_capacity(self.h))

    def grown_ahead(self) -> int:
        return int(self.d.hydamd_grown_ahead(self.h))

    def overflow_reruns(self) -> int:
        return int(self.d.hydamd_overflow_reruns(self.h))

    def read_payload(self) -> bytes:
        n = self.payload_size()
        buf = np.zeros(max(n, 1), np.uint8)
        self._ck(self.d.hydamd_read_payload(self.h, buf.ctypes.data, n))
        return buf[:n].tobytes()

    def read_sections(self, slot: int):
        bits = np.zeros(GROUPS_PER_LFG, np.uint32)
        offs = np.zeros(GROUPS_PER_LFG, np.uint64)
        self._ck(self.d.hydamd_read_sections(self.h, slot, bits.ctypes.data, offs.ctypes.data))
        return bits.astype(np.int64), offs.astype(np.int64)

    def read_tables(self, slot: int):
        freq = np.zeros((MAX_CLUSTERS, ALPHABET), np.uint32)
        alpha = np.zeros(MAX_CLUSTERS, np.uint32)
        la, rm = C.c_uint32(0), C.c_uint32(0)
        self._ck(self.d.hydamd_read_tables(self.h, slot, freq.ctypes.data, alpha.ctypes.data, C.byref(la), C.byref(rm)))
        return freq, alpha.astype(np.int64), la.value, rm.value

    def read_dc(self, slot: int, vbw: int, vbh: int) -> np.ndarray:
        out = np.zeros((3, vbh, vbw), np.int32)
        self._ck(self.d.hydamd_read_dc(self.h, slot, out.ctypes.data, vbw, vbh))
        return out

    def read_symbol_counts(self, slot: int) -> np.ndarray:
        out = np.zeros(GROUPS_PER_LFG, np.uint32)
        self._ck(self.d.hydamd_read_symbol_counts(self.h, slot, out.ctypes.data))
        return out.astype(np.int64)

    def read_tokens(self, slot: int, group: int, count: int) -> np.ndarray:
        out = np.zeros(max(count, 1), np.uint64)
        self._ck(self.d.hydamd_read_tokens(self.h, slot, group, out.ctypes.data, count))
        return out[:count]

    def read_debug_plane(self, which: int, pitch: int, rows: int) -> np.ndarray:
        out = np.zeros((3, rows, pitch), np.int32 if which == 2 else np.float32)
        self._ck(self.d.hydamd_read_debug_plane(self.h, which, out.ctypes.data, pitch, rows))
        return out

    def profile(self, enable: bool):
        self._ck(self.d.hydamd_profile(self.h, int(enable)))

    def profile_read(self):
        ms = (C.c_double * len(K_NAMES))()
        n = (C.c_uint64 * len(K_NAMES))()
        self._ck(self.d.hydamd_profile_read(self.h, ms, n))
        return {K_NAMES[i]: (ms[i], n[i]) for i in range(len(K_NAMES))}

    def submit_lf_group(self, slot: int):
        """Enqueue the transform stage of the LF group in `slot` now (slots in order) instead of at finish_frame."""
        self._ck(self.d.hydamd_submit_lf_group(self.h, slot))

    def run_lf_coder(self, num_slots: int, last: bool):
        """Enqueue the LF coder for the transformed slots below `num_slots` in the context's stream;
        `last` also packs the frame's LF streams so that sync_lf() can wait for just them."""
        self._ck(self.d.hydamd_run_lf_coder(self.h, num_slots, int(last)))

    def sync_lf(self):
        self._ck(self.d.hydamd_sync_lf(self.h))

    # ---- LF-group coder (csrc/hip/lf_coder.hip) ----
    def set_lf_coder(self, on_device):
        """False/0 off, True/1 on a side stream (lowest latency), 2 at the end of the main stream (throughput)."""
        self._ck(self.d.hydamd_set_lf_coder(self.h, int(on_device)))

    def lf_coder(self) -> bool:
        return bool(self.d.hydamd_lf_coder(self.h))

    def read_lf_stream(self, slot: int):
        """(lengths[384] u8, alphabet, run_pairs, bit_count) of the device-coded LF-coefficient stream."""
        lengths = np.zeros(LF_CODES, np.uint8)
        a, r, b = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._ck(self.d.hydamd_read_lf_stream(self.h, slot, lengths.ctypes.data, C.byref(a), C.byref(r), C.byref(b)))
        return lengths, a.value, r.value, b.value

    def read_lf_bits(self, slot: int, bit_count: int) -> np.ndarray:
        out = np.zeros(max((bit_count + 7) // 8, 1), np.uint8)
        self._ck(self.d.hydamd_read_lf_bits(self.h, slot, out.ctypes.data, (bit_count + 7) // 8))
        return out[: (bit_count + 7) // 8]

    def read_lf_streams(self, count: int, first: int = 0) -> np.ndarray:
        """Structured array of the per-slot LF stream records (bit_count, alphabet, run_pairs, error, offset, lengths)."""
        out = np.zeros(count, LF_INFO_DTYPE)
        self._ck(self.d.hydamd_read_lf_streams(self.h, first, count, out.ctypes.data))
        return out

    def lf_payload_size(self) -> int:
        return int(self.d.hydamd_lf_payload_size(self.h))

    def read_lf_payload(self) -> np.ndarray:
        n = self.lf_payload_size()
        out = np.zeros(max(n, 1), np.uint8)
        self._ck(self.d.hydamd_read_lf_payload(self.h, out.ctypes.data, n))
        return out[:n]

    def lf_payload_tensor(self):
        """The frame's packed LF symbol data as a CUDA uint8 tensor aliasing the context's buffer (valid after sync)."""
        import torch

        cap = self.max_lf_groups * LF_BITWORDS * 4
        return self._device_view("lf", int(self.d.hydamd_lf_payload_device(self.h) or 0), cap)[: self.lf_payload_size()]

    def shader_clock_mhz(self) -> float:
        v = C.c_double(0)
        self._ck(self.d.hydamd_debug_shader_clock_mhz(self.h, C.byref(v)))
        return v.value

    def transform_footprint(self, sample_fmt: int):
        """(static LDS bytes, registers per thread) of the transform kernel instance serving `sample_fmt` (0 u8, 1 u16, 2 f32, 3 f16, 4 bf16,
        16 ... 19 NV12, 32 ... 35 and 48 ... 51 NV12 with interpolated chroma, 80 ... 243 the P010 / P012 / P016 family)."""
        lds, regs = C.c_int(0), C.c_int(0)
        self._ck(self.d.hydamd_debug_transform_footprint(self.h, int(sample_fmt), C.byref(lds), C.byref(regs)))
        return lds.value, regs.value

    def debug_lf_code(self, hist: np.ndarray):
        """Device code construction for one histogram over the compact token space -> (lengths, codes, alphabet, error)."""
        hist = np.ascontiguousarray(hist, np.uint32)
        assert hist.shape == (LF_CODES,)
        lengths = np.zeros(LF_CODES, np.uint8)
        codes = np.zeros(LF_CODES, np.uint32)
        a, e = C.c_uint32(0), C.c_uint32(0)
        self._ck(self.d.hydamd_debug_lf_code(self.h, hist.ctypes.data, lengths.ctypes.data, codes.ctypes.data,
                                             C.byref(a), C.byref(e)))
        return lengths, codes, a.value, e.value


class HydAmdLfStream(C.Structure):
    _fields_ = [("lengths", C.c_void_p), ("alphabet", C.c_uint32), ("run_pairs", C.c_uint32), ("bits", C.c_void_p),
                ("bit_count", C.c_uint64)]


def frame_from_results(md: "api.HYDImageMetadata", tiles, dcs, freqs, alphabets, group_bits, max_alphabet: int,
                       payload: bytes, *, write_header=True, is_last=True, icc: Optional[bytes] = None,
                       lf_streams=None) -> bytes:
    """Codestream bytes from LF-group results in `tiles` order (host only).

    The LF coefficients come either as LF ints (``dcs``, hydamd_frame_from_results) or, when the GPU
    LF coder produced them, as ``lf_streams``: one (lengths, alphabet, run_pairs, bit_count, bits)
    tuple per LF group (hydamd_frame_from_streams)."""
    d = dll()
    n = len(tiles)
    tile_xy = np.ascontiguousarray(np.array(tiles, np.uint32).reshape(-1))
    freq = np.ascontiguousarray(np.stack(freqs).astype(np.uint32))
    alpha = np.ascontiguousarray(np.stack(alphabets).astype(np.uint32))
    bits = np.ascontiguousarray(np.stack(group_bits).astype(np.uint32))
    out, out_len, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p(None)
    tail = (freq.ctypes.data, alpha.ctypes.data, bits.ctypes.data, max_alphabet, payload, len(payload), icc,
            len(icc) if icc else 0, C.byref(out), C.byref(out_len), C.byref(err))
    if lf_streams is not None:
        keep = [(np.ascontiguousarray(l, np.uint8), np.ascontiguousarray(b, np.uint8)) for l, _, _, _, b in lf_streams]
        arr = (HydAmdLfStream * n)()
        for i, (_, a, r, nb, _) in enumerate(lf_streams):
            arr[i] = HydAmdLfStream(keep[i][0].ctypes.data, a, r, keep[i][1].ctypes.data if nb else None, nb)
        ret = d.hydamd_frame_from_streams(C.byref(md), int(write_header), int(is_last), n, tile_xy.ctypes.data, arr, *tail)
    else:
        dc_arrays = [np.ascontiguousarray(a, np.int32) for a in dcs]
        dcp = (C.c_void_p * n)(*[a.ctypes.data for a in dc_arrays])
        ret = d.hydamd_frame_from_results(C.byref(md), int(write_header), int(is_last), n, tile_xy.ctypes.data, dcp, *tail)
    if ret:
        raise DeviceError(ret, (err.value or b"").decode())
    data = C.string_at(out.value, out_len.value)
    d.hydamd_free(out)
    return data


BLOB_HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("num_slots", "<u4"), ("status", "<u4"),
                              ("hf_bytes", "<u8"), ("lf_bytes", "<u8"), ("total_bytes", "<u8"), ("lf_coded", "<u4"),
                              ("reserved", "<u4", (5,))])
BLOB_SLOT_DTYPE = np.dtype([("preset", "<u4"), ("running_max_alphabet", "<u4"), ("log_alphabet_size", "<u4"),
                            ("table_error", "<u4"), ("alphabet", "<u4", (MAX_CLUSTERS,)), ("reserved", "<u4", (3,)),
                            ("group_bits", "<u4", (GROUPS_PER_LFG,)), ("freq", "<u4", (MAX_CLUSTERS, ALPHABET)),
                            ("lf", LF_INFO_DTYPE)])
BLOB_MAGIC = 0x42445948
BLOB_RETRY = 0xE


def blob_header(blob) -> np.ndarray:
    """The header record of a blob held in a bytes-like / uint8 array."""
    return np.frombuffer(memoryview(blob)[:BLOB_HEADER_DTYPE.itemsize], BLOB_HEADER_DTYPE)[0]


def frame_from_blobs(md: "api.HYDImageMetadata", blobs, *, write_header=True, is_last=True, icc: Optional[bytes] = None,
                     lib=None, raw: bool = False):
    """One-frame codestream from the blobs of the contexts that coded its LF groups (host only)."""
    d = lib or dll()
    arrs = [np.ascontiguousarray(np.frombuffer(b, np.uint8)) for b in blobs]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    sizes = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
    out, out_len, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p(None)
    ret = d.hydamd_frame_from_blobs(C.byref(md), int(write_header), int(is_last), len(arrs), ptrs, sizes, icc,
                                    len(icc) if icc else 0, C.byref(out), C.byref(out_len), C.byref(err))
    if ret:
        raise DeviceError(ret, (err.value or b"").decode())
    if raw:  # the library's own buffer, no copy: (ctypes uint8 array, release())
        view = (C.c_uint8 * out_len.value).from_address(out.value)
        return view, (lambda: d.hydamd_free(out))
    data = C.string_at(out.value, out_len.value)
    d.hydamd_free(out)
    return data


class Assembler:
    """Device-side frame assembly (hydamd_assembler_*): shard blobs in device memory -> the finished one-frame
    codestream in one device-accessible buffer.  One assembler serves one frame at a time."""

    def __init__(self, device: int = 0):
        self.d = dll()
        st = C.c_int(0)
        self.h = self.d.hydamd_assembler_create(device, C.byref(st))
        if not self.h:
            raise DeviceError(st.value, "assembler could not be created")

    def close(self):
        if self.h:
            self.d.hydamd_assembler_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, code: int):
        if code != 0:
            raise DeviceError(code, (self.d.hydamd_assembler_error(self.h) or b"").decode())

    def plan(self, md: "api.HYDImageMetadata", blob_lf_ids, *, write_header=True, is_last=True, icc: Optional[bytes] = None):
        """blob_lf_ids[b] = raster ids of the LF groups blob b carries, in its slot order (cheap when it repeats)."""
        counts = np.array([len(ids) for ids in blob_lf_ids], np.uint32)
        flat = np.array([lf for ids in blob_lf_ids for lf in ids], np.uint32)
        self._ck(self.d.hydamd_assembler_plan(self.h, C.byref(md), int(write_header), int(is_last), len(counts), counts.ctypes.data,
                                              flat.ctypes.data, icc, len(icc) if icc else 0))
        self.nblobs = len(counts)

    def run(self, blob_ptrs, blob_caps, out_ptr: int, out_cap: int, stream_ptr: int):
        """Enqueue on `stream_ptr` (a hipStream_t): blob_ptrs are device pointers, out_ptr any device-accessible buffer."""
        n = len(blob_ptrs)
        ptrs = (C.c_void_p * n)(*blob_ptrs)
        caps = (C.c_size_t * n)(*blob_caps)
        self._ck(self.d.hydamd_assembler_run(self.h, ptrs, caps, stream_ptr, out_ptr, out_cap))

    def run_tensors(self, blobs, out, stream=None):
        import torch

        st = stream if stream is not None else torch.cuda.current_stream()
        self.run([b.data_ptr() for b in blobs], [b.numel() for b in blobs], out.data_ptr(), out.numel(), st.cuda_stream)

    def result(self) -> int:
        """After the stream has been synchronised: bytes of the frame (raises on a device-side failure)."""
        n = C.c_size_t(0)
        self._ck(self.d.hydamd_assembler_result(self.h, C.byref(n)))
        return int(n.value)


class MultiFrame:
    """One device-resident frame on N devices of this process, composed in C (hydamd_multi_*, csrc/host/multi.c):
    LF groups dealt in raster runs, floors by peer read, the file assembled on a shard of the caller's choice."""

    def __init__(self, devices: Sequence[int], width: int, height: int, linear_light: int = 0):
        self.d = dll()
        md = api.HYDImageMetadata(width, height, int(linear_light), -1, -1)
        arr = (C.c_int * len(devices))(*devices)
        st = C.c_int(0)
        self.h = self.d.hydamd_multi_create(len(devices), arr, C.byref(md), C.byref(st))
        if not self.h:
            raise DeviceError(st.value, "multi-device frame could not be created")
        self.n, self.width, self.height = len(devices), width, height

    def close(self):
        if self.h:
            self.d.hydamd_multi_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, code: int):
        if code != 0:
            raise DeviceError(code, (self.d.hydamd_multi_error(self.h) or b"").decode())

    def shard_lf_groups(self, shard: int):
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._ck(self.d.hydamd_multi_shard_lf_groups(self.h, shard, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def encode(self, origins, assembling_shard: int = 0):
        """origins[d]: an interleaved (H, W, 3) torch tensor on shard d's device holding (at least) that shard's LF
        groups at their place in the image — or an int: the device address pixel (0, 0) would have.  Asynchronous; the
        tensors must stay alive until result().  Or Nv12 objects of the image's size, one pitch and one matrix."""
        if origins and isinstance(origins[0], Nv12):
            flat, o0 = [], origins[0]
            for o in origins:
                if not isinstance(o, Nv12) or (o.pitch, o.pixel_stride, o.sample_fmt) != (o0.pitch, o0.pixel_stride, o0.sample_fmt):
                    raise ValueError("the shards of a frame share one layout and sample format")
                flat += o.pointers()
            arr = (C.c_void_p * len(flat))(*flat)
            self._ck(self.d.hydamd_encode_image_multi(self.h, arr, o0.pitch, o0.pixel_stride, o0.sample_fmt, assembling_shard))
            return
        ptrs, isz, fmt = [], None, None
        for o in origins:
            if hasattr(o, "data_ptr"):
                isz, fmt = o.element_size(), sample_fmt_of(o)
                b = o.data_ptr()
            else:
                b = int(o)
            ptrs.append(b)
        isz = isz or getattr(self, "sample_bytes", 1)
        if fmt is None:
            fmt = {1: 0, 2: 1, 4: 2}[isz]  # bare addresses: sample_bytes names an integer format or float32
        flat = []
        for b in ptrs:
            flat += [b, b + isz, b + 2 * isz]
        arr = (C.c_void_p * len(flat))(*flat)
        self._ck(self.d.hydamd_encode_image_multi(self.h, arr, 3 * self.width, 3, fmt, assembling_shard))

    def result(self) -> int:
        n = C.c_size_t(0)
        self._ck(self.d.hydamd_multi_result(self.h, C.byref(n)))
        return int(n.value)

    def read(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        size = self.result()
        buf = out if out is not None and out.nbytes >= size else np.empty(size, np.uint8)
        self._ck(self.d.hydamd_multi_read(self.h, buf.ctypes.data, buf.nbytes))
        return buf[:size]

    def context_overflow_reruns(self, shard: int) -> int:
        return int(self.d.hydamd_overflow_reruns(self.d.hydamd_multi_context(self.h, shard)))


def _read_image(img, row_stride: Optional[int] = None, pixel_stride: Optional[int] = None, sample_fmt: Optional[int] = None):
    """One image as (ptrs, row_stride, pixel_stride, height, width, sample_fmt), strides in samples: an Nv12 object, an
    interleaved (H, W, C >= 3) tensor, a triple of (H, W) plane tensors — these say everything themselves — or device
    addresses: three of them, with the caller's strides and format and no size (height and width None), or
    (ptrs, row_stride, pixel_stride, width, height) with the caller's format."""
    if isinstance(img, Nv12):  # V one byte behind U, pixel stride 1, the pitch of both planes (PlanarYuv: the chroma planes' pitch)
        return img.pointers(), img.pitch, img.pixel_stride, img.height, img.width, img.sample_fmt
    if hasattr(img, "data_ptr"):
        p, isz, shape = img.data_ptr(), img.element_size(), img.shape
        return [p, p + isz, p + 2 * isz], img.stride(0), img.stride(1), shape[0], shape[1], sample_fmt_of(img)
    if hasattr(img[0], "data_ptr"):  # planes keep their shape: the size is theirs, never a bare pointer's
        rs, ps, (h, w) = img[0].stride(0), img[0].stride(1), img[0].shape[:2]
        if any(tuple(p.shape[:2]) != (h, w) or (p.stride(0), p.stride(1)) != (rs, ps) for p in img):
            raise ValueError("the three planes of an image share one shape and one layout")
        return [p.data_ptr() for p in img], rs, ps, h, w, sample_fmt_of(img[0])
    if hasattr(img[0], "__len__"):
        ptrs, row_stride, pixel_stride, w, h = img
        if sample_fmt is None:
            raise ValueError("device addresses need sample_fmt")
    else:
        ptrs, h, w = img, None, None
        if row_stride is None or pixel_stride is None or sample_fmt is None:
            raise ValueError("device addresses need row_stride, pixel_stride and sample_fmt")
    return [int(p) if p is not None else None for p in ptrs], row_stride, pixel_stride, h, w, sample_fmt


class TiledImage:
    """A tile-mode image (every tile a frame of its own) from device-resident pixels, frames built on the GPU
    (hydamd_tiled_*, csrc/host/tiled.c): tiles coded in launch groups of up to ``tiles_per_launch`` (0: the default, 32),
    the finished file left in device memory."""

    def __init__(self, width: int, height: int, shift_x: int, shift_y: int, linear_light: int = 0, device: int = 0,
                 tiles_per_launch: int = 0):
        self.d = dll()
        md = api.HYDImageMetadata(width, height, int(linear_light), shift_x, shift_y)
        st = C.c_int(0)
        self.h = self.d.hydamd_tiled_create(device, C.byref(md), tiles_per_launch, C.byref(st))
        if not self.h:
            raise DeviceError(st.value, (self.d.hydamd_tiled_error(None) or b"").decode() or "tiled image could not be created")
        self.width, self.height = width, height
        self._keep = None

    def close(self):
        if self.h:
            self.d.hydamd_tiled_destroy(self.h)
            self.h = None
        self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, code: int):
        if code != 0:
            raise DeviceError(code, (self.d.hydamd_tiled_error(self.h) or b"").decode())

    def encode(self, img, row_stride: Optional[int] = None, pixel_stride: Optional[int] = None, sample_fmt: Optional[int] = None):
        """img: an interleaved (H, W, C >= 3) torch tensor on the object's device (C > 3: the first three channels,
        pixel stride C), three (H, W) plane tensors, or three device addresses (then the strides, in samples, and the
        sample format are the caller's), or an Nv12 object.  Asynchronous: the pixels must stay alive and unchanged until
        result()."""
        ptrs, row_stride, pixel_stride, _, _, sample_fmt = _read_image(img, row_stride, pixel_stride, sample_fmt)
        self._keep = img
        arr = (C.c_void_p * 3)(*ptrs)
        self._ck(self.d.hydamd_encode_image_tiled(self.h, arr, row_stride, pixel_stride, sample_fmt))

    def result(self) -> int:
        n = C.c_size_t(0)
        self._ck(self.d.hydamd_tiled_result(self.h, C.byref(n)))
        self._keep = None
        return int(n.value)

    def read(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        size = self.result()
        buf = out if out is not None and out.nbytes >= size else np.empty(size, np.uint8)
        self._ck(self.d.hydamd_tiled_read(self.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.nbytes))
        return buf[:size]

    def device_ptr(self) -> int:
        p = self.d.hydamd_tiled_device(self.h)
        return C.cast(p, C.c_void_p).value or 0

    def overflow_reruns(self) -> int:
        return int(self.d.hydamd_tiled_overflow_reruns(self.h))

    def device_bytes(self) -> int:
        return int(self.d.hydamd_tiled_device_bytes(self.h))


class _DeviceBatch:
    """What FrameBatch and MixedBatch share — everything but their constructors and encode(): the calls of one protocol
    (csrc/host/batchrun.c), exported as hydamd_<_prefix>_*."""

    _prefix = ""

    def _c(self, name: str):
        return getattr(self.d, f"hydamd_{self._prefix}_{name}")

    def close(self):
        if self.h:
            self._c("destroy")(self.h)
            self.h = None
        self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, code: int):
        if code != 0:
            raise DeviceError(code, (self._c("error")(self.h) or b"").decode())

    def result(self) -> int:
        """Waits for the batch; bytes of all its files."""
        n = C.c_size_t(0)
        try:
            self._ck(self._c("result")(self.h, C.byref(n)))
        finally:
            self._keep = None
        return int(n.value)

    def offsets(self) -> np.ndarray:
        """uint64[frames + 1]: file k is bytes offsets[k] .. offsets[k + 1] of the device buffer."""
        self.result()
        out = np.zeros(self.frames + 1, np.uint64)
        self._ck(self._c("offsets")(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def read(self, k: Optional[int] = None):
        """File k as a uint8 array; None: the list of all files (one copy from the device)."""
        off = self.offsets()
        if k is None:
            buf = np.empty(max(int(off[-1]), 1), np.uint8)
            self._ck(self._c("read")(self.h, -1, buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.nbytes))
            return [buf[int(off[i]):int(off[i + 1])] for i in range(self.frames)]
        if not 0 <= k < self.frames:
            raise IndexError("no such frame in the batch")
        buf = np.empty(max(int(off[k + 1] - off[k]), 1), np.uint8)
        self._ck(self._c("read")(self.h, k, buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.nbytes))
        return buf[: int(off[k + 1] - off[k])]

    def device_ptr(self) -> int:
        return C.cast(self._c("device")(self.h), C.c_void_p).value or 0

    def offsets_device_ptr(self) -> int:
        return C.cast(self._c("offsets_device")(self.h), C.c_void_p).value or 0

    def set_image_errors(self, on: bool):
        """An outcome per image (status()): an image with a non-finite float sample yields no bytes, the others their
        files; off, such a sample fails the whole batch.  Not while a batch is in flight."""
        self._ck(self._c("set_image_errors")(self.h, int(bool(on))))

    def status(self) -> np.ndarray:
        """uint32[frames]: 0 a file, IMAGE_BAD_SAMPLE a non-finite sample and no bytes."""
        self.result()
        out = np.zeros(max(self.frames, 1), np.uint32)
        self._ck(self._c("image_status")(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[: self.frames]

    def status_device_ptr(self) -> int:
        return C.cast(self._c("image_status_device")(self.h), C.c_void_p).value or 0

    def overflow_reruns(self) -> int:
        return int(self._c("overflow_reruns")(self.h))


class FrameBatch(_DeviceBatch):
    """Batches of up to ``max_frames`` one-frame images of one shape from device-resident pixels, every one a finished
    file built on the GPU (hydamd_batch_*, csrc/host/batch.c): the files back to back in one device buffer, the table of
    their offsets beside it."""

    _prefix = "batch"

    def __init__(self, width: int, height: int, max_frames: int, linear_light: int = 0, device: int = 0,
                 icc: Optional[bytes] = None, image_errors: bool = False):
        self.d = dll()
        md = api.HYDImageMetadata(width, height, int(linear_light), -1, -1)
        st = C.c_int(0)
        self.h = self.d.hydamd_batch_create(device, C.byref(md), max_frames, icc, len(icc) if icc else 0, C.byref(st))
        if not self.h:
            raise DeviceError(st.value, (self.d.hydamd_batch_error(None) or b"").decode() or "frame batch could not be created")
        self.width, self.height, self.max_frames = width, height, max_frames
        self.frames = 0
        self._keep = None
        if image_errors:
            self.set_image_errors(True)

    def encode(self, imgs, row_stride: Optional[int] = None, pixel_stride: Optional[int] = None, sample_fmt: Optional[int] = None):
        """imgs: one entry per frame, all of one layout — interleaved (H, W, C >= 3) torch tensors on the object's device
        (C > 3: the first three channels, pixel stride C), triples of (H, W) plane tensors, or triples of device addresses
        (then the strides, in samples, and the sample format are the caller's).  Asynchronous: the pixels must stay alive
        and unchanged until result()."""
        ptrs = []
        for img in imgs:  # (Nv12: one pitch and one matrix for all)
            p, rs, ps, _, _, fmt = _read_image(img, row_stride, pixel_stride, sample_fmt)
            ptrs += p
            layout = (rs, ps, fmt)
            if (row_stride, pixel_stride, sample_fmt) == (None, None, None):
                row_stride, pixel_stride, sample_fmt = layout
            elif layout != (row_stride, pixel_stride, sample_fmt):
                raise ValueError("the frames of a batch share one layout and sample format")
        self._keep = imgs
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        self._ck(self.d.hydamd_encode_batch(self.h, len(imgs), arr, row_stride or 0, pixel_stride or 0,
                                            sample_fmt if sample_fmt is not None else -1))
        self.frames = len(imgs)


IMAGE_BAD_SAMPLE = 1  # include/hydrium_amd.h, HYDAMD_IMAGE_BAD_SAMPLE


def mixed_descriptors(imgs, sample_fmt: Optional[int] = None, sample_fmts=None):
    """MixedBatch.encode's reading of its arguments, without a device: (HydAmdImageDesc array, [format of image k]).

    sample_fmts None: one format for all — sample_fmt, else the tensors' common dtype (ValueError when they differ, or
    when address tuples come without sample_fmt).  "each": every tensor's own dtype (address tuples: sample_fmt).  A
    sequence: image k's format, which a tensor's dtype must agree with (a value that is no format goes through to the
    library, which refuses the batch)."""
    if sample_fmts is not None and not isinstance(sample_fmts, str):
        sample_fmts = [int(f) for f in sample_fmts]
        if len(sample_fmts) != len(imgs):
            raise ValueError("sample_fmts names one format per image")
    elif sample_fmts is not None and sample_fmts != "each":
        raise ValueError('sample_fmts is None, "each" or one format per image')
    descs = (HydAmdImageDesc * max(len(imgs), 1))()
    fmts = []
    for k, img in enumerate(imgs):
        given = sample_fmts[k] if isinstance(sample_fmts, list) else sample_fmt
        ptrs, rs, ps, h, w, fmt = _read_image(img, sample_fmt=given)
        if sample_fmts is None:
            if sample_fmt is None:
                sample_fmt = fmt
            elif fmt != sample_fmt:
                raise ValueError("the images of a batch share one sample format")
        elif isinstance(sample_fmts, list) and fmt != given:
            if given in (0, 1, 2, FLOAT16, BFLOAT16) + NV12_FAMILY + P016_FAMILY + PLANAR_FAMILY + PLANAR16_FAMILY:
                raise ValueError("sample_fmts disagrees with a tensor's dtype")
            fmt = given  # not a format at all: the library refuses it (HYD_API_ERROR), nothing is enqueued
        fmts.append(fmt)
        descs[k] = HydAmdImageDesc((C.c_void_p * 3)(*ptrs), int(rs), int(ps), int(w), int(h))
    return descs, fmts


class MixedBatch(_DeviceBatch):
    """Batches of up to ``max_frames`` (0: the default, 32) one-frame images, EACH OF ITS OWN SIZE up to 2048 x 2048, from
    device-resident pixels, every one a finished file built on the GPU (hydamd_mixed_*, csrc/host/mixed.c): the files back
    to back in one device buffer, the table of their offsets beside it.  Conventions as FrameBatch's.

    ``max_lf_groups`` (max_frames..255; None: as above, a slot per image): the LF-group slots of the object's context — an
    image may then hold up to 28 LF groups of 2048 x 2048 pixels, a batch up to max_lf_groups of them in all
    (hydamd_mixed_create_slots)."""

    _prefix = "mixed"

    def __init__(self, max_frames: int = 0, linear_light: int = 0, device: int = 0, max_lf_groups: Optional[int] = None,
                 image_errors: bool = False):
        self.d = dll()
        st = C.c_int(0)
        if max_lf_groups is None:
            self.h = self.d.hydamd_mixed_create(device, max_frames, int(linear_light), C.byref(st))
        else:
            self.h = self.d.hydamd_mixed_create_slots(device, max_frames, int(max_lf_groups), int(linear_light), C.byref(st))
        if not self.h:
            raise DeviceError(st.value, (self.d.hydamd_mixed_error(None) or b"").decode() or "mixed batch could not be created")
        self.max_frames = max_frames or 32
        self.max_lf_groups = max_lf_groups
        self.frames = 0
        self._keep = None
        if image_errors:
            self.set_image_errors(True)

    def encode(self, imgs, sample_fmt: Optional[int] = None, sample_fmts=None):
        """imgs: one entry per image, each of its own size and layout — an interleaved (H, W, C >= 3) torch tensor on the
        object's device (any row pitch; C > 3: the first three channels, pixel stride C), a triple of (H, W) plane
        tensors, an Nv12 object, or (ptrs, row_stride, pixel_stride, width, height) with three device addresses and strides
        in samples (then sample_fmt is the caller's).  One sample format per call, unless sample_fmts says otherwise: "each" takes
        every tensor's own dtype, a list names image k's format (0 / 1 / 2: 8-bit, 16-bit, float; what address tuples
        need).  Asynchronous: the pixels must stay alive and unchanged until result()."""
        descs, fmts = mixed_descriptors(imgs, sample_fmt, sample_fmts)
        self._keep = imgs
        if sample_fmts is None:
            self._ck(self.d.hydamd_encode_mixed(self.h, len(imgs), descs, fmts[0] if fmts else -1))
        else:
            self._ck(self.d.hydamd_encode_mixed_formats(self.h, len(imgs), descs, (C.c_int * max(len(fmts), 1))(*fmts)))
        self.frames = len(imgs)


def decode_token_records(rec: np.ndarray):
    """Split device token records into (token, local cluster, residue_bits, residue) arrays."""
    lo = (rec & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return lo & 0xFF, (lo >> 8) & 0xF, (lo >> 16) & 0x3F, (rec >> np.uint64(32)).astype(np.uint32)
