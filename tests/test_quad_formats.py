"""CPU-only: the formats whose pixel is one group of four samples (HYDAMD_AYUV_*, HYDAMD_Y412_*, HYDAMD_Y416_*) where no device is
needed — the descriptor, the refusals and the origins of csrc/hyd_sample_fmt.h and the round trip of csrc/hip/hydk_store.h against a
model written from the prose, with every older number's description unchanged; the per-pixel definition (csrc/hip/hydk_quad.h) as
plain C++ under address and UB sanitizers, and as the probe library's host build, against quad_model.py; device.Ayuv's and
device.Y416's reading of their surface; the drop-in API's refusal; the header's names; and what the six new instances of the
transform kernel ask of a compute unit.  Every test here fails on the parent, where 524296 is "Invalid Sample Format"."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import dword_model as dm
import format_dump
import format_model as fm
import p016_model as p16
import packed16_model as p6
import packed_model as pkm
import planar16_model as p16m
import planar_model as plm
import quad_model as qm
import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 7, 8, 9, 33)
HEIGHT = 3
LO, HI = 524000, 524801
NONE = [0] * 12 + [0, -1, 0, 0, 0, 0]


def random_pixels(fmt, w, h, seed=524288):
    """h rows of w random pixels, every bit random: the fourth sample set, all three codes far out of range"""
    raw = np.random.default_rng(seed + 100 * w + h + fmt).integers(0, 2 ** 64, (h, w), dtype=np.uint64)
    return (raw >> np.uint64(64 - 8 * qm.pixel_bytes(fmt))).astype(qm.dtype_of(fmt))


def all_ones(fmt, w, h):
    return np.full((h, w), 2 ** (8 * qm.pixel_bytes(fmt)) - 1, qm.dtype_of(fmt))


def check_definition(to_rgb, widths=WIDTHS, height=HEIGHT):
    """to_rgb(depth, matrix, pixels, w, h) -> (h, w, 3) uint8 or uint16, held to the model over all twelve formats on random pixels,
    all zeros and all ones (the ends of the range: nothing may wrap).  Shared with the on-device test."""
    for w in widths:
        for fmt in qm.FAMILY:
            for pixels in (random_pixels(fmt, w, height), np.zeros((height, w), qm.dtype_of(fmt)), all_ones(fmt, w, height)):
                got, want = to_rgb(qm.depth_of(fmt), qm.matrix_of(fmt), pixels, w, height), qm.expected_rgb(pixels, fmt)
                assert got.dtype == want.dtype and got.shape == want.shape == (height, w, 3)
                wrong = np.argwhere(got != want)
                assert wrong.size == 0, (fmt, w, [(tuple(p), int(got[tuple(p)]), int(want[tuple(p)])) for p in wrong[:8]])


def hook(fn, *device):
    """a probe-flavour quad entry as to_rgb(depth, matrix, pixels, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def to_rgb(depth, matrix, pixels, w, h):
        pixels = np.ascontiguousarray(pixels)
        assert pixels.itemsize == (8 if depth else 4)
        out = np.full((h, w, 3), 0xA5A5 if depth else 0xA5, np.uint16 if depth else np.uint8)
        assert fn(*device, depth, matrix, pixels.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return to_rgb


@pytest.fixture(scope="module")
def program():
    """tests/c/quad_formats.cc: hyd_sample_fmt.h, hydk_store.h and hydk_quad.h with g++ under address and UB sanitizers, no HIP
    header, no warning"""
    return format_dump.sanitized_program("quad_formats")


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


def table_of(program, lo, hi):
    return program("describe", lo, hi).view(np.int32).reshape(hi - lo, 18).tolist()


def pixels_of(program, cases):
    """cases: (fmt, pixels (h, w), pitch, flip) -> the program's pictures.  The surface handed over ends with the last pixel of its
    last row, 0x5A in the pitch's slack"""
    blob = []
    for fmt, rows, pitch, flip in cases:
        h, w = rows.shape
        surface = np.full(pitch * (h - 1) + w, 0x5A5A5A5A5A5A5A5A >> (64 - 8 * qm.pixel_bytes(fmt)), qm.dtype_of(fmt))
        for r in range(h):
            at = pitch * (h - 1 - r if flip else r)
            surface[at:at + w] = rows[r]
        blob.append(struct.pack("<6I", qm.depth_of(fmt), qm.matrix_of(fmt), w, h, pitch, flip) + surface.tobytes())
    got = program("pixels", data=struct.pack("<I", len(cases)) + b"".join(blob))
    out, at = [], 0
    for fmt, rows, _, _ in cases:
        h, w = rows.shape
        n = h * w * 3 * (2 if qm.depth_of(fmt) else 1)
        out.append(got[at:at + n].view(np.uint16 if qm.depth_of(fmt) else np.uint8).reshape(h, w, 3))
        at += n
    assert at == got.size
    return out


# ---- the model ----
def test_the_model_takes_apart_what_it_put_together():
    rng = np.random.default_rng(1)
    for fmt in qm.FAMILY:
        top = 65536 if qm.depth_of(fmt) else 256
        y, u, v, a = (rng.integers(0, top, (HEIGHT, 9)) for _ in range(4))
        d = qm.pack(y, u, v, a, fmt)
        assert d.dtype == qm.dtype_of(fmt) and all(np.array_equal(p, q) for p, q in zip(qm.samples(d, fmt), (y, u, v, a)))
    assert qm.pack([[3]], [[2]], [[1]], 4, 524296).tolist() == [[1 | 2 << 8 | 3 << 16 | 4 << 24]]  # bytes V, U, Y, A
    assert qm.pack([[2]], [[1]], [[3]], 4, 524488).tolist() == [[1 | 2 << 16 | 3 << 32 | 4 << 48]]  # words U, Y, V, A
    assert [qm.public_name(f) for f in (524296, 524427, 524490)] == ["AYUV_BT709", "Y412_BT601_FULL", "Y416_BT601"]
    assert [qm.as_planar(f) for f in (524297, 524424, 524491)] == [521, 2184, 2251]


# ---- the descriptor ----
def test_the_descriptor_of_every_number_from_524000_to_524800(program):
    table = table_of(program, LO, HI)
    formats = []
    for fmt, row in zip(range(LO, HI), table):
        got, job = qm.Fmt(*row[:12]), tuple(row[12:])
        assert got == qm.describe(fmt), (fmt, got)
        assert job == qm.job(fmt), (fmt, job)  # hydk_decode_fmt, and hydk_encode_fmt back to the number
        if got.device:
            formats.append(fmt)
            d = (fmt - 524288) >> 6
            assert (got.device, got.host, got.is_float, got.layout, got.filter, got.sub, got.sx, got.sy) == (1, 0, 0, 5, 0, 2, 0, 0)
            assert (got.bytes, got.bits, got.depth) == {0: (4, 8, 0), 2: (8, 12, 2), 3: (8, 16, 3)}[d]
    assert formats == sorted(qm.FAMILY) == [524296, 524297, 524298, 524299, 524424, 524425, 524426, 524427, 524488, 524489, 524490, 524491]
    by_number = dict(zip(range(LO, HI), table))
    nothing = [524288, 524289, 524291, 524292, 524295, 524300, 524304, 524312, 524328, 524344,  # subsampling != 2, filter bits, matrix overflow
               524360, 524361, 524362, 524363,  # depth 1: the 10-bit surface is Y410
               524352, 524416, 524420, 524423, 524428, 524432, 524440, 524456, 524480, 524484, 524487, 524492, 524496, 524504, 524520,
               524552, 524553, 524616, 524680, 524744]  # depth 4 and up
    for fmt in nothing:
        assert by_number[fmt] == NONE, fmt
    for lo, hi in ((393100, 393300), (786300, 786600), (1048500, 1048700), (2097100, 2097200), (2 ** 31 - 200, 2 ** 31 - 1)):
        assert all(row == NONE for row in table_of(program, lo, hi)), (lo, hi)


def test_every_older_number_is_described_as_before(program):
    """-8 ... 4100 against format_model and the older program's print, 8150 ... 8500 against packed_model, 32700 ... 33100 against
    packed16_model, 130900 ... 131400 against dword_model, job fields included; and nothing in the gaps"""
    rows, _ = format_dump.formats()
    for fmt, row in zip(range(fm.LO, fm.HI), table_of(program, fm.LO, fm.HI)):
        assert fm.Fmt(*row[:12]) == fm.describe(fmt), fmt
        assert (fm.Fmt(*row[:12]), tuple(row[12:])) == rows[fmt], fmt
        cls, storage, variant = fm.storage_of(fmt)
        assert (row[14], row[15], row[17]) == (cls, storage, variant), fmt
    assert fm.LO <= -8 and fm.HI > 4100
    lo, hi = 8150, 8501
    for fmt, row in zip(range(lo, hi), table_of(program, lo, hi)):
        want = pkm.describe(fmt)
        assert pkm.Fmt(*row[:12]) == want, fmt
        assert tuple(row[12:]) == ((1, fmt, 0, 11 + int(want.filter != 0), want.matrix, 2048 << int(want.filter != 0)) if want.device else (0, -1, 0, 0, 0, 0))
    lo, hi = 32700, 33101
    for fmt, row in zip(range(lo, hi), table_of(program, lo, hi)):
        want = p6.describe(fmt)
        assert p6.Fmt(*row[:12]) == want, fmt
        interp = int(want.filter != 0)
        assert tuple(row[12:]) == ((1, fmt, 1, 13 + interp, want.matrix + 4 * want.depth, 8192 << interp) if want.device else (0, -1, 0, 0, 0, 0)), fmt
    lo, hi = 130900, 131401
    seen = []
    for fmt, row in zip(range(lo, hi), table_of(program, lo, hi)):
        assert dm.Fmt(*row[:12]) == dm.describe(fmt) and tuple(row[12:]) == dm.job(fmt), fmt
        seen += [fmt] * row[0]
    assert seen == [131072, 131073, 131144, 131145, 131146, 131147]
    gaps = ((4101, 4300), (33101, 33600), (130400, 130900), (131401, 131700), (196500, 196700), (262100, 262300), (523700, 524000), (524801, 525100))
    for lo, hi in gaps:
        assert all(row == NONE for row in table_of(program, lo, hi)), (lo, hi)


AYUV0, Y412_0, Y416_0 = 524296, 524424, 524488
REFUSAL_CASES = [
    # (fmt, y, du, dv, pixel_stride, no_src, width), the three offsets in BYTES from a 16-byte boundary -> message
    *[((fmt, y, 0, 0, 1, 0, width), None) for fmt in qm.FAMILY for y, width in ((0, 200), (8, 0), (-16, 1))],
    *[((fmt, 4, 0, 0, 1, 0, 200), None) for fmt in qm.AYUV],  # AYUV sits on any dword
    *[((fmt, -12, 0, 0, 1, 0, 200), None) for fmt in qm.AYUV],
    *[((fmt, 0, du, dv, 1, 0, 200), qm.LAYOUT_MSG) for fmt in (524296, 524299, 524424, 524491)
      for du, dv in ((8, 16), (8, 8), (0, 8), (8, 0), (-8, 0), (1, 2), (2, 4), (1000, 2000))],  # unequal pointers
    *[((fmt, y, 0, 0, 1, 0, 200), qm.LAYOUT_MSG) for fmt in (524296, 524298) for y in (1, 2, 3, 5, 6, 7, -1, -2, -3)],  # AYUV off the dword
    *[((fmt, y, 0, 0, 1, 0, 200), qm.LAYOUT_MSG) for fmt in (524424, 524427, 524488, 524490)
      for y in (4, 2, 6, 1, 3, 12, -4, -2, 20)],  # Y412 / Y416 off the qword: + 4 in particular, which a dword test would let through
    *[((fmt, 0, 0, 0, ps, 0, 200), qm.LAYOUT_MSG) for fmt in (524296, 524425, 524489) for ps in (0, 2, 4, -1, 3, 8)],
    ((524296, 1, 4, 8, 3, 1, 200), None),               # src NULL: the layout is not looked at
    ((524488, 4, 0, 0, 0, 1, 0), None),
    ((524427, 3, 2, 1, 2, 1, 200), None),
    *[((fmt, 0, 0, 0, 1, 0, 200), "Invalid Sample Format") for fmt in (524287, 524288, 524292, 524300, 524312, 524360, 524363, 524428, 524492, 524552, 786440, 1048584)],
    ((524360, 0, 0, 0, 1, 1, 200), "Invalid Sample Format"),
    # the other families keep their rules and their messages
    ((131072, 0, 0, 0, 1, 0, 200), None),
    ((131144, 4, 0, 0, 1, 0, 200), None),
    ((131144, 2, 0, 0, 1, 0, 200), dm.LAYOUT_MSG),
    ((131073, 0, 0, 0, 2, 0, 200), dm.LAYOUT_MSG),
    ((32832, 0, 2, 6, 2, 0, 200), None),
    ((32832, 0, 0, 0, 1, 0, 200), p6.LAYOUT_MSG),
    ((8192, 0, 1, 3, 2, 0, 200), None),
    ((8192, 0, 0, 0, 1, 0, 200), pkm.LAYOUT_MSG),
    ((2112, 1, 1000, 2000, 100, 0, 200), "planar YCbCr of 16-bit words wants its three planes on 2-byte boundaries"),
    ((519, 0, 1, 3, 2, 0, 200), "planar YCbCr wants the chroma planes' pitch in pixel_stride"),
    ((80, 0, 2, 6, 1, 0, 200), "P010/P016 wants pixel_stride 1 and V one sample behind U"),
    ((16, 0, 1, 3, 2, 0, 200), "NV12 wants pixel_stride 1 and V one byte behind U"),
    ((1, 1, 0, 0, 1, 0, 200), None),
    ((0, 3, 1, 2, 3, 0, 200), None),
]


def test_the_refusals(program):
    data = struct.pack("<I", len(REFUSAL_CASES)) + b"".join(struct.pack("<7i", *case) for case, _ in REFUSAL_CASES)
    got = program("refusals", data=data).reshape(len(REFUSAL_CASES), 96)
    for field, (case, want) in zip(got, REFUSAL_CASES):
        message = bytes(field).split(b"\0")[0].decode()
        assert message == (want or ""), (case, message)
    fmt_h = open(os.path.join(hbuild.CSRC, "hyd_sample_fmt.h")).read()
    assert fmt_h.count('"' + qm.LAYOUT_MSG + '"') == 1 and "HYD_FMT_QUAD_LAYOUT_MSG" in fmt_h  # one new message
    for old in (dm.LAYOUT_MSG, p6.LAYOUT_MSG, pkm.LAYOUT_MSG):
        assert fmt_h.count('"' + old + '"') == 1  # the old ones kept
    header = " ".join(open(os.path.join(ROOT, "include", "hydrium_amd.h")).read().replace("\n *", " ").split())
    assert qm.LAYOUT_MSG in header


def test_the_origins(program):
    cases = [(fmt, pitch, x0, y0) for fmt in (524296, 524299, 524424, 524491) for pitch in (4096, -4096, 4099, -4099)
             for x0, y0 in ((256, 256), (2048, 0), (0, 0), (0, 768), (1, 1), (257, 3), (33, 511))]
    data = struct.pack("<I", len(cases)) + b"".join(struct.pack("<4i", *c) for c in cases)
    got = program("origins", data=data).view(np.int64).reshape(len(cases), 3)
    for row, (fmt, pitch, x0, y0) in zip(got.tolist(), cases):
        # y0 rows and x0 PIXELS, added to all three pointers (bytes here: four or eight a pixel): any x0 and y0
        assert row == [qm.pixel_bytes(fmt) * (y0 * pitch + x0)] * 3, (fmt, pitch, x0, y0, row)


# ---- the definition ----
def test_every_byte_value_in_every_position_of_an_ayuv_dword(program, probe):
    """all 256 values of each byte in each of the four positions under all four matrices, the other bytes random, against the
    model of hydk_yuv_to_rgb; the fourth position changes nothing"""
    rng = np.random.default_rng(10)
    v = np.arange(256, dtype=np.uint32).reshape(1, 256)
    host = hook(probe.hydt_quad_to_rgb_host)
    cases, wants = [], []
    for pos in range(4):
        others = [rng.integers(0, 256, (1, 256), dtype=np.uint32) for _ in range(4)]
        others[pos] = v
        d = (others[0] | others[1] << 8 | others[2] << 16 | others[3] << 24).astype(np.uint32)
        for fmt in qm.AYUV:
            m = qm.matrix_of(fmt)
            want = ym.yuv_to_rgb(m, others[2].astype(np.uint8), others[1].astype(np.uint8), others[0].astype(np.uint8))  # Y, U, V = bytes 2, 1, 0
            assert want.dtype == np.uint8 and np.array_equal(want, qm.expected_rgb(d, fmt))
            assert np.array_equal(host(0, m, d, 256, 1), want)
            if pos == 3:
                assert np.array_equal(want, qm.expected_rgb(d & 0xFFFFFF, fmt)) and np.array_equal(host(0, m, d | 0xFF000000, 256, 1), want)
            cases.append((fmt, d, 256, 0))
            wants.append(want)
    for got, want in zip(pixels_of(program, cases), wants):
        assert np.array_equal(got, want)
    assert len({qm.expected_rgb(cases[0][1], f).tobytes() for f in qm.AYUV}) == 4  # the matrices are four pictures


def test_an_ayuv_picture_is_the_i444_picture_of_its_bytes():
    for w in WIDTHS:
        for fmt in qm.AYUV:
            for pixels in (random_pixels(fmt, w, HEIGHT), all_ones(fmt, w, HEIGHT)):
                y, u, v, _ = qm.samples(pixels, fmt)
                assert plm.is_format(qm.as_planar(fmt)) and plm.name_of(qm.as_planar(fmt)).startswith("i444")
                assert np.array_equal(qm.expected_rgb(pixels, fmt), plm.expected_rgb((y, u, v), qm.matrix_of(fmt), plm.S444, 0))


def test_a_y416_picture_is_the_i416_picture_of_its_words_and_y412_the_i412_picture_of_the_words_shifted():
    for w in WIDTHS:
        for fmt in qm.Y416:
            pixels = random_pixels(fmt, w, HEIGHT)
            y, u, v, _ = qm.samples(pixels, fmt)
            assert p16m.public_name(qm.as_planar(fmt)).startswith("I416_")
            assert np.array_equal(qm.expected_rgb(pixels, fmt), p16m.expected_rgb((y, u, v), qm.as_planar(fmt)))
        for fmt in qm.Y412:
            pixels = random_pixels(fmt, w, HEIGHT)
            zero_low = pixels & np.uint64(0xFFF0FFF0FFF0FFF0)
            y, u, v, _ = qm.samples(zero_low, fmt)
            assert p16m.public_name(qm.as_planar(fmt)).startswith("I412_")
            assert np.array_equal(qm.expected_rgb(zero_low, fmt), p16m.expected_rgb((y >> 4, u >> 4, v >> 4), qm.as_planar(fmt)))
            # non-zero low bits: the P012 rule on the words as stored — they count
            y, u, v, _ = qm.samples(pixels, fmt)
            assert np.array_equal(qm.expected_rgb(pixels, fmt), p16.yuv_to_rgb(2, qm.matrix_of(fmt), y, u, v))
    pixels = random_pixels(524424, 33, HEIGHT)
    assert not np.array_equal(qm.expected_rgb(pixels, 524424), qm.expected_rgb(pixels & np.uint64(0xFFF0FFF0FFF0FFF0), 524424))
    assert len({qm.expected_rgb(pixels, f).tobytes() for f in qm.Y416}) == 4  # the matrices are four pictures


def test_the_fourth_sample_never_matters(program, probe):
    host = hook(probe.hydt_quad_to_rgb_host)
    cases, wants = [], []
    for fmt in qm.FAMILY:
        pixels = random_pixels(fmt, 33, HEIGHT, 77)
        y, u, v, a = qm.samples(pixels, fmt)
        want = qm.expected_rgb(pixels, fmt)
        for fourth in (a, 0, 65535 if qm.depth_of(fmt) else 255):
            d = qm.pack(y, u, v, fourth, fmt)
            assert np.array_equal(qm.expected_rgb(d, fmt), want)
            assert np.array_equal(host(qm.depth_of(fmt), qm.matrix_of(fmt), d, 33, HEIGHT), want)
            cases.append((fmt, d, 33, 0))
            wants.append(want)
    for got, want in zip(pixels_of(program, cases), wants):
        assert np.array_equal(got, want)


def test_the_definition_under_sanitizers_stays_inside_rows_between_guard_words(program):
    """every surface a malloc that ends with the last pixel of its last row, rows of random pixels with 0x5A bytes between them,
    top-down and bottom-up, widths 1 ... 9 and 33: the sanitizer is the bounds check, the guard words tell a read beyond a row's W
    pixels"""
    cases, wants = [], []
    for w in tuple(range(1, 10)) + (33,):
        for fmt in qm.FAMILY:
            for n, (pitch, flip) in enumerate(((w, 0), (w + 5, 0), (w + 3, 1))):
                rows = random_pixels(fmt, w, HEIGHT, 99 + n) if n or fmt % 2 else all_ones(fmt, w, HEIGHT)
                cases.append((fmt, rows, pitch, flip))
                wants.append(qm.expected_rgb(rows, fmt))
    for (fmt, rows, pitch, flip), got, want in zip(cases, pixels_of(program, cases), wants):
        assert got.dtype == want.dtype and np.array_equal(got, want), (fmt, rows.shape, pitch, flip)
    for fmt in qm.FAMILY:
        other = random_pixels(fmt, 33, HEIGHT, 99)
        guard = other.copy()
        guard[:, -1] = 0x5A5A5A5A5A5A5A5A >> (64 - 8 * qm.pixel_bytes(fmt))
        assert not np.array_equal(qm.expected_rgb(other, fmt), qm.expected_rgb(guard, fmt))  # the guard would have shown


def test_the_host_build_of_the_definition_equals_the_model(probe):
    check_definition(hook(probe.hydt_quad_to_rgb_host))
    one, out = np.zeros((1, 1), np.uint64), np.zeros((1, 1, 3), np.uint16)
    fn = probe.hydt_quad_to_rgb_host
    for depth, matrix in ((-1, 0), (1, 0), (4, 0), (0, 4), (0, -1), (3, 4), (2, -1)):
        assert fn(depth, matrix, one.ctypes.data, out.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_quad_to_rgb_host", b"hydt_quad_to_rgb_device"):
        assert name in probe and name not in shipped


# ---- names ----
def test_the_headers_names_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    body = re.search(r"\nenum \{\n\s*HYDAMD_AYUV_BT709 = (.*?)\n\};\n", text, re.S)
    assert body, "the twelve names sit in an anonymous enum"
    flat = " ".join(("HYDAMD_AYUV_BT709 = " + body.group(1)).split())
    assert flat == ("HYDAMD_AYUV_BT709 = 524288 + 4 * 2, HYDAMD_AYUV_BT709_FULL, HYDAMD_AYUV_BT601, HYDAMD_AYUV_BT601_FULL, "
                    "HYDAMD_Y412_BT709 = 524288 + 4 * 2 + 64 * 2, HYDAMD_Y412_BT709_FULL, HYDAMD_Y412_BT601, HYDAMD_Y412_BT601_FULL, "
                    "HYDAMD_Y416_BT709 = 524288 + 4 * 2 + 64 * 3, HYDAMD_Y416_BT709_FULL, HYDAMD_Y416_BT601, HYDAMD_Y416_BT601_FULL")
    want = {"HYDAMD_" + qm.public_name(fmt): fmt for fmt in qm.FAMILY}
    assert len(want) == 12 and want["HYDAMD_AYUV_BT709"] == 524296 and want["HYDAMD_Y412_BT601"] == 524426 and want["HYDAMD_Y416_BT601_FULL"] == 524491
    for name, fmt in want.items():
        assert getattr(device, name[len("HYDAMD_"):]) == fmt and name in text  # (the C side: tests/c/quad_formats.cc's static_assert)
    assert device.QUAD_FAMILY == qm.FAMILY and (device.AYUV_FORMATS, device.Y412_FORMATS, device.Y416_FORMATS) == (qm.AYUV, qm.Y412, qm.Y416)
    for fmt in qm.FAMILY:
        assert device.ycbcr_fields(fmt) == (524288, qm.matrix_of(fmt), 2, 0, qm.depth_of(fmt))
        assert device.ycbcr_fmt(524288, qm.matrix_of(fmt), 2, 0, qm.depth_of(fmt)) == fmt
    older = set(device.NV12_FAMILY) | set(device.P016_FAMILY) | set(device.PLANAR_FAMILY) | set(device.PLANAR16_FAMILY) | set(device.PACKED_FAMILY) | \
        set(device.PACKED16_FAMILY) | set(device.DWORD_FAMILY)
    assert not set(device.QUAD_FAMILY) & older and len(older) == 214
    assert "AYUV" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    # none of them is a numbered #define: the header's count of those is what it was
    assert not re.findall(r"^#define HYDAMD_(AYUV|Y412|Y416)\w* +-?\d+\s*$", text, re.M)
    assert len(re.findall(r"^#define HYDAMD_\w+ +-?\d+\s*$", text, re.M)) == 176
    # the older names keep their numbers
    assert (device.NV12_BT709, device.P016L_BT601_FULL, device.I420_BT709, device.I410_BT709, device.I416_BT601_FULL, device.YUY2_BT709,
            device.YUY2L_BT601_FULL, device.Y210_BT709, device.Y216L_BT601_FULL, device.RGB10A2, device.BGR10A2, device.Y410_BT709,
            device.Y410_BT601_FULL) == (16, 243, 512, 2120, 2251, 8192, 8227, 32832, 32995, 131072, 131073, 131144, 131147)
    for fmt in dm.Y410:
        assert device.ycbcr_fields(fmt) == (131072, dm.matrix_of(fmt), 2, 0, 1)


def test_the_family_is_struck_from_the_older_out_of_scope_lists_and_says_its_own():
    for path in (os.path.join(ROOT, "include", "hydrium_amd.h"), os.path.join(ROOT, "DESIGN.md"), os.path.join(ROOT, "INTEGRATION.md")):
        text = " ".join(open(path).read().replace("\n *", " ").split())
        scopes = re.findall(r"(?:Out of scope|Not covered):.*?\.(?= [A-Z(#`]| \*/|$)", text)
        assert len(scopes) >= 9, path
        own = [s for s in scopes if "ayuv64le" in s]
        assert len(own) == 1, (path, own)
        for word in ("uyva", "vyu444", "alpha", "v210", "NV16 / NV24 / P210", "host-pointer input", "PQ / HLG / BT.2020"):
            assert word in own[0], (path, word)
        for scope in scopes:
            if scope is not own[0]:
                assert "AYUV" not in scope and "Y416" not in scope, (path, scope)
        assert "131072" in text and "Y416" in text and "R11G11B10F" in text, path
    header = " ".join(open(os.path.join(ROOT, "include", "hydrium_amd.h")).read().replace("\n *", " ").split())
    assert "every other number from 131072 up to 524287 names nothing" in header and "every other number from 131072 up names nothing" not in header


def test_ayuv_and_y416_name_their_format_and_fill_a_descriptor():
    import torch
    from hydrium_amd import device

    for w, h in ((1, 5), (8, 8), (33, 9), (200, 120)):
        for cls, group, dtypes, sample_dtypes, kw, fmts in (
                (device.Ayuv, 4, (torch.int32, torch.uint32), (torch.uint8, torch.int8), {}, qm.AYUV),
                (device.Y416, 8, (torch.int64, torch.uint64), (torch.int16, torch.uint16), {"depth": 16}, qm.Y416),
                (device.Y416, 8, (torch.int64,), (torch.uint16,), {"depth": 12}, qm.Y412)):
            for dtype in dtypes:  # a pixel an element
                buf = torch.zeros(h * (w + 6) + 4, dtype=dtype)
                surface = buf.as_strided((h, w), (w + 6, 1), 4)
                pics = [cls(surface, w, 16 + m, **kw) for m in ym.MATRICES] + [cls(surface, w, f, **kw) for f in fmts]
                for pic, fmt in zip(pics, fmts + fmts):
                    assert isinstance(pic, device.Ayuv) and isinstance(pic, device.Nv12)
                    assert device.sample_fmt_of(pic) == fmt == pic.sample_fmt and pic.shape == (h, w, 3)
                    assert (pic.pitch, pic.pixel_stride) == (w + 6, 1)  # in pixels
                    assert pic.pointers() == [buf.data_ptr() + 4 * group] * 3
                    descs, got = device.mixed_descriptors([pic])
                    d = descs[0]
                    assert got == [fmt] and (d.row_stride, d.pixel_stride, d.width, d.height) == (w + 6, 1, w, h)
                    assert [d.src[0], d.src[1], d.src[2]] == pic.pointers()
            for dtype in sample_dtypes:  # four samples a pixel
                buf = torch.zeros((h * (w + 6) + 4) * 4, dtype=dtype)
                surface = buf.as_strided((h, w, 4), ((w + 6) * 4, 4, 1), 16)
                pic = cls(surface, w, **kw)
                assert (pic.sample_fmt, pic.pitch, pic.pixel_stride, pic.shape) == (fmts[0], w + 6, 1, (h, w, 3))
                assert pic.pointers() == [buf.data_ptr() + 4 * group] * 3
    surface = torch.zeros((120, 200), dtype=torch.int32)
    assert device.Ayuv(surface, 200).sample_fmt == device.AYUV_BT709 == 524296
    assert device.Ayuv(surface, 199).width == 199 and device.Ayuv(surface, 57).pitch == 200  # a wider surface
    crop = device.Ayuv(surface[3:, 5:], 100, device.NV12_BT601)  # any x0 and y0, odd ones too
    assert crop.pointers() == [surface.data_ptr() + 4 * (3 * 200 + 5)] * 3 and (crop.height, crop.pitch, crop.sample_fmt) == (117, 200, 524298)
    words = torch.zeros((120, 200, 4), dtype=torch.int16)
    deep = device.Y416(words[7:, 11:], 100, depth=12)
    assert deep.pointers() == [words.data_ptr() + 8 * (7 * 200 + 11)] * 3 and (deep.height, deep.pitch, deep.sample_fmt, deep.depth) == (113, 200, 524424, 12)
    assert device.Y416(words, 200).sample_fmt == device.Y416_BT709 == 524488
    rgb16 = torch.zeros((120, 200, 3), dtype=torch.int16)
    y210 = device.PackedYuv16(torch.zeros((120, 400), dtype=torch.int16), 200)
    y410 = device.Y410(surface, 200)
    got = device.mixed_descriptors([crop, rgb16, y210, y410, deep, device.Rgb10(surface, 200, "bgr")], sample_fmts="each")[1]
    assert got == [524298, 1, 32832, 131144, 524424, 131073]


def test_ayuv_and_y416_refuse_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    surface = torch.zeros((10, 36), dtype=torch.int32)
    qwords = torch.zeros((10, 36), dtype=torch.int64)
    with pytest.raises(ValueError, match="width pixels"):  # a row too short for the width
        device.Ayuv(surface, 37)
    with pytest.raises(ValueError, match="width pixels"):
        device.Y416(qwords, 0)
    with pytest.raises(ValueError, match="unit element stride"):
        device.Ayuv(torch.zeros((10, 72), dtype=torch.int32)[:, ::2], 18)
    with pytest.raises(ValueError, match="unit element stride"):
        device.Y416(torch.zeros((10, 72), dtype=torch.int64)[:, ::2], 18)
    for other in (torch.uint8, torch.int16, torch.float16, torch.float32, torch.int64, torch.float64):  # wrong dtype
        with pytest.raises(ValueError, match="4-byte integer"):
            device.Ayuv(torch.zeros((10, 36), dtype=other), 18)
    for other in (torch.uint8, torch.int16, torch.int32, torch.float32, torch.float64):
        with pytest.raises(ValueError, match="8-byte integer"):
            device.Y416(torch.zeros((10, 36), dtype=other), 18)
    for other in (torch.int16, torch.int32, torch.float16):  # four samples a pixel: bytes for AYUV, words for Y416
        with pytest.raises(ValueError, match="1-byte integer"):
            device.Ayuv(torch.zeros((10, 36, 4), dtype=other), 18)
    for other in (torch.uint8, torch.int32, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="2-byte integer"):
            device.Y416(torch.zeros((10, 36, 4), dtype=other), 18)
    with pytest.raises(ValueError, match="four to a pixel"):
        device.Ayuv(torch.zeros((10, 36, 3), dtype=torch.uint8), 18)
    with pytest.raises(ValueError, match="four to a pixel"):  # a non-unit sample stride
        device.Y416(torch.zeros((10, 36, 8), dtype=torch.int16)[:, :, ::2], 18)
    with pytest.raises(ValueError, match="four to a pixel"):  # a pixel stride that is not the group
        device.Ayuv(torch.zeros((10, 72, 4), dtype=torch.uint8)[:, ::2], 18)
    with pytest.raises(ValueError, match="whole number of pixels"):  # a pitch that is no whole pixels
        device.Ayuv(torch.zeros(10 * 150, dtype=torch.uint8).as_strided((10, 36, 4), (146, 4, 1)), 36)
    with pytest.raises(ValueError, match="whole number of pixels"):
        device.Y416(torch.zeros(10 * 150, dtype=torch.int16).as_strided((10, 36, 4), (146, 4, 1)), 36)
    with pytest.raises(ValueError, match="4-byte boundary"):  # a misaligned base
        device.Ayuv(torch.zeros(10 * 144 + 8, dtype=torch.uint8).as_strided((10, 36, 4), (144, 4, 1), 2), 36)
    for off in (1, 2, 3):  # words off the qword: + 2, + 4 and + 6 bytes
        with pytest.raises(ValueError, match="8-byte boundary"):
            device.Y416(torch.zeros(10 * 144 + 8, dtype=torch.int16).as_strided((10, 36, 4), (144, 4, 1), off), 36)
    for bad in (0, 1, 32, 80, 520, 2248, 8192, 32832, 131072, 131144, 524288, 524360, 524300, 524424, 524488):  # one of the four matrices, or an AYUV number
        with pytest.raises(ValueError):
            device.Ayuv(surface, 18, bad)
    for bad in (0, 524296, 524360, 524424, 524492, 131144):  # ... or a number of that depth
        with pytest.raises(ValueError):
            device.Y416(qwords, 18, bad, depth=16)
    with pytest.raises(ValueError):
        device.Y416(qwords, 18, 524488, depth=12)
    for bad in (10, 8, 0, 14, 32):  # 10 bits are Y410's
        with pytest.raises(ValueError, match="depth"):
            device.Y416(qwords, 18, depth=bad)
    for cls in (device.Ayuv, device.Y416):
        with pytest.raises(TypeError):
            cls.from_surface(surface, 18, 10, 36, 0)
    with pytest.raises(ValueError, match="4-byte integer"):  # and the dword family keeps to dwords
        device.Y410(qwords, 18)


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((24, 16), np.uint64)
    for fmt in qm.FAMILY:
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p, p], 0, 0, 16, 1, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_six_new_instances_have_symbols_of_their_own_and_keep_the_transform_kernels_contract():
    """k_transform_tokenize_quad<mode, HYDK_STORE_AYUV | _Y416>: none under an older symbol name, the older kernels' counts as they
    are, no scratch, group_segment_fixed_size <= 31 856 and next_free_vgpr <= 128"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_quad" in k}
    assert sorted(re.match(r"_Z25k_transform_tokenize_quadILi(\d)ELi(\d+)EE", k).groups() for k in new) == \
        [(mode, store) for mode in "012" for store in ("17", "18")], sorted(res)
    older = ("k_transform_tokenize_planar", "k_transform_tokenize_p016", "k_transform_tokenize_yuvp16", "k_transform_tokenize_yuy2", "k_transform_tokenize_y216",
             "k_transform_tokenize_dword", "_Z20k_transform_tokenizeI")
    assert not any(o in k for k in new for o in older)
    count = lambda stem: sum(stem in k for k in res)
    assert [count(o) for o in older] == [6, 6, 6, 6, 6, 6, 19]
    for name, d in sorted(new.items()):
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 31856, (name, d)
        assert d["next_free_vgpr"] <= 128, (name, d)
