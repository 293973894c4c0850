"""CPU-only: the float render targets whose pixel is one dword of three unsigned floats (HYDAMD_R11G11B10F, HYDAMD_RGB9E5) where no
device is needed — the widening of every pattern (csrc/hip/hydk_ufloat.h) against exact arithmetic, as plain C++ under address and UB
sanitizers and as the probe library's host build; the descriptor, the refusals and the origins of csrc/hyd_sample_fmt.h and the round
trip of csrc/hip/hydk_store.h against ufloat_model.py, with every older number's description unchanged; device.R11g11b10f's and
device.Rgb9e5's reading of their surface; the drop-in API's refusal; the header's names and prose; and what the two new instances of
the transform kernel ask of a compute unit.  On the parent 8388608 is "Invalid Sample Format" and every test here fails, except the
three that need nothing of the library's new code: the model's own test, the exponent-31 test and the drop-in API's refusal."""
import ctypes as C
import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

import dword_model as dm
import format_dump
import format_model as fm
import packed16_model as p6
import packed_model as pkm
import quad_model as qm
import ufloat_model as um
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 8388608
LO, HI = BASE - 300, BASE + 501
NONE = [0] * 12 + [0, -1, 0, 0, 0, 0]
HEIGHT = 3
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def program():
    """tests/c/ufloat_formats.cc: hyd_sample_fmt.h, hydk_store.h and hydk_ufloat.h with g++ under address and UB sanitizers, no HIP
    header, no warning"""
    return format_dump.sanitized_program("ufloat_formats")


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


def table_of(program, lo, hi):
    return program("describe", lo, hi).view(np.int32).reshape(hi - lo, 18).tolist()


def random_dwords(w, h, seed=23):
    """h rows of w dwords, every bit random: R11G11B10F fields of exponent 31 among them"""
    return np.random.default_rng(seed + 100 * w + h).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


def same_bits(got, want):
    return got.dtype == want.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want)


# ---- exact arithmetic ----
def exact_field(v, mbits):
    """the value of a field as a Fraction, "inf" or "nan": the issue's three rules"""
    e, m = v >> mbits, v & ((1 << mbits) - 1)
    if e == 31:
        return "inf" if m == 0 else "nan"
    if e == 0:
        return Fraction(m, 2 ** (14 + mbits))
    return Fraction(2) ** (e - 15) * (1 + Fraction(m, 2 ** mbits))


def exact_f32(bits):
    """the value of float32 bits that are a normal or zero, as a Fraction; None for anything else (subnormal, Inf, NaN, negative)"""
    sign, e, m = bits >> 31, (bits >> 23) & 0xFF, bits & 0x7FFFFF
    if sign or e == 255 or (e == 0 and m):
        return None
    return Fraction(0) if e == 0 else Fraction(2) ** (e - 127) * (1 + Fraction(m, 2 ** 23))


def check_widening(fields11, fields10, e5):
    """uint32 arrays of 2048, 1024 and (32, 512) float32 bits, held to exact arithmetic; shared with the on-device test"""
    assert fields11.shape == (2048,) and fields10.shape == (1024,) and e5.shape == (32, 512)
    for got, mbits in ((fields11, 6), (fields10, 5)):
        for v, bits in enumerate(got.tolist()):
            want = exact_field(v, mbits)
            if want == "inf":
                assert bits == 0x7F800000, (mbits, v, hex(bits))
            elif want == "nan":  # a NaN that keeps its mantissa bits, at the top of the float32 mantissa
                assert bits == 0x7F800000 | (v & ((1 << mbits) - 1)) << (23 - mbits), (mbits, v, hex(bits))
            else:
                assert exact_f32(bits) == want, (mbits, v, hex(bits))  # a float32 normal or zero, never a subnormal
    assert exact_f32(int(fields11[1])) == Fraction(1, 2 ** 20) and exact_f32(int(fields10[1])) == Fraction(1, 2 ** 19)
    assert fields11[15 << 6] == fields10[15 << 5] == np.float32(1).view(np.uint32)
    for e in range(32):
        for m, bits in enumerate(e5[e].tolist()):
            assert exact_f32(bits) == Fraction(m) * Fraction(2) ** (e - 24), (e, m, hex(bits))  # every pattern finite
    assert exact_f32(int(e5[0, 1])) == Fraction(1, 2 ** 24) and exact_f32(int(e5[31, 511])) == 511 * 128


def widen_hook(fn, *device):
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]

    def widen(kind, values):
        values = np.ascontiguousarray(values, np.uint32)
        out = np.full(values.size, 0xDEADBEEF, np.uint32)
        assert fn(*device, kind, values.ctypes.data, out.ctypes.data, values.size) == 0
        return out

    return widen


def every_pattern_through(widen):
    """the three tables of check_widening through a hydt_ufloat_widen_* hook"""
    pairs = (np.arange(32, dtype=np.uint32)[:, None] << 9 | np.arange(512, dtype=np.uint32)[None, :]).reshape(-1)
    return widen(0, np.arange(2048)), widen(1, np.arange(1024)), widen(2, pairs).reshape(32, 512)


def surface_hook(fn, *device):
    """a probe-flavour surface entry as to_bits(which, dwords) -> (h, w, 3) uint32"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def to_bits(which, dwords):
        dwords = np.ascontiguousarray(dwords, np.uint32)
        h, w = dwords.shape
        out = np.full((h, w, 3), 0xA5A5A5A5, np.uint32)
        assert fn(*device, which, dwords.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return to_bits


def check_definition(to_bits, widths=(1, 2, 7, 8, 9, 33)):
    """held to the model on random dwords, all zeros and all ones; shared with the on-device test"""
    for w in widths:
        for fmt in um.FAMILY:
            for d in (random_dwords(w, HEIGHT), np.zeros((HEIGHT, w), np.uint32), np.full((HEIGHT, w), 0xFFFFFFFF, np.uint32)):
                got, want = to_bits(um.which_of(fmt), d), um.expected_bits(d, fmt)
                assert same_bits(got, want), (fmt, w)


def pixels_of(program, cases):
    """cases: (fmt, dwords (h, w), pitch, flip) -> the program's pictures.  The surface handed over ends with the last dword of its
    last row, guard words in the pitch's slack"""
    blob = []
    for fmt, rows, pitch, flip in cases:
        h, w = rows.shape
        surface = np.full(pitch * (h - 1) + w, GUARD, np.uint32)
        for r in range(h):
            at = pitch * (h - 1 - r if flip else r)
            surface[at:at + w] = rows[r]
        blob.append(struct.pack("<5I", um.which_of(fmt), w, h, pitch, flip) + surface.tobytes())
    got = program("pixels", data=struct.pack("<I", len(cases)) + b"".join(blob))
    out, at = [], 0
    for _, rows, _, _ in cases:
        n = rows.size * 12
        out.append(got[at:at + n].view(np.uint32).reshape(rows.shape + (3,)))
        at += n
    assert at == got.size
    return out


# ---- the model ----
def test_the_model_widens_as_exact_arithmetic_does_and_packs_to_the_nearest_field():
    check_widening(um.widen_field(np.arange(2048), 6), um.widen_field(np.arange(1024), 5),
                   um.widen_e5(np.arange(512)[None, :], np.arange(32)[:, None]))
    for mbits, codes in ((6, 31 << 6), (5, 31 << 5)):  # every finite value packs to its own code
        v = np.arange(codes)
        assert np.array_equal(um.pack_field(um.field_value(v, mbits), mbits), v)
    assert um.pack_field(np.array([-1.0, 0.0, 1.0, 1e9, np.nan]), 6).tolist() == [0, 0, 15 << 6, (31 << 6) - 1, 0]
    rgb = np.random.default_rng(3).random((5, 9, 3)) * 4
    for fmt, bound in ((um.R11G11B10F, 2.0 ** -5), (um.RGB9E5, 2.0 ** -7)):  # half a step of the coarsest field below 4
        d = um.pack(rgb, fmt)
        back = um.expected_f32(d, fmt)
        assert d.dtype == np.uint32 and d.shape == (5, 9) and np.abs(back - rgb).max() <= bound
        assert np.array_equal(um.pack(back, fmt), d)  # a representable picture packs to itself
    assert um.pack_rgb9e5(np.array([[[1.0, 0.5, 0.25]]])).tolist() == [[256 | 128 << 9 | 64 << 18 | 16 << 27]]
    assert [um.public_name(f) for f in um.FAMILY] == ["R11G11B10F", "RGB9E5"]


# ---- the widening ----
def test_every_pattern_widens_exactly_under_sanitizers(program):
    got = program("widen").view(np.uint32)
    assert got.size == 2048 + 1024 + 32 * 512
    check_widening(got[:2048], got[2048:3072], got[3072:].reshape(32, 512))


def test_every_pattern_widens_exactly_in_the_host_build(probe):
    tables = every_pattern_through(widen_hook(probe.hydt_ufloat_widen_host))
    check_widening(*tables)
    for got, want in zip(tables, (um.widen_field(np.arange(2048), 6), um.widen_field(np.arange(1024), 5),
                                  um.widen_e5(np.arange(512)[None, :], np.arange(32)[:, None]))):
        assert np.array_equal(got, want)
    one, out = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    fn = probe.hydt_ufloat_widen_host
    for kind, n in ((-1, 1), (3, 1), (0, 0), (0, 65537)):
        assert fn(kind, one.ctypes.data, out.ctypes.data, n) == api.HYD_API_ERROR
    assert fn(0, None, out.ctypes.data, 1) == api.HYD_API_ERROR and fn(0, one.ctypes.data, None, 1) == api.HYD_API_ERROR


def test_only_exponent_31_is_non_finite_and_no_rgb9e5_dword_is():
    f11, f10 = um.widen_field(np.arange(2048), 6).view(np.float32), um.widen_field(np.arange(1024), 5).view(np.float32)
    for f, mbits in ((f11, 6), (f10, 5)):
        v = np.arange(f.size)
        assert np.array_equal(~np.isfinite(f), v >> mbits == 31)
        assert np.array_equal(np.isinf(f), v == 31 << mbits) and (f[np.isinf(f)] > 0).all()
        assert np.array_equal(np.isnan(f), v > 31 << mbits)
    assert np.isfinite(um.expected_f32(random_dwords(257, 9), um.RGB9E5)).all()
    assert np.isfinite(um.expected_f32(np.full((1, 1), 0xFFFFFFFF, np.uint32), um.RGB9E5)).all()
    assert np.isnan(um.expected_f32(np.full((1, 1), 0xFFFFFFFF, np.uint32), um.R11G11B10F)).all()


# ---- the descriptor ----
def test_the_descriptor_of_every_number_from_base_minus_300_to_base_plus_500(program):
    formats = []
    for fmt, row in zip(range(LO, HI), table_of(program, LO, HI)):
        got, job = um.Fmt(*row[:12]), tuple(row[12:])
        assert got == um.describe(fmt), (fmt, got)
        assert job == um.job(fmt), (fmt, job)  # hydk_decode_fmt, and hydk_encode_fmt back to the number
        if got.device:
            formats.append(fmt)
            assert (got.is_float, got.bytes, got.host, got.layout) == (1, 4, 0, 6)
            assert job == (1, fmt, 2, 19 + fmt - BASE, 0, 0)
    assert formats == list(um.FAMILY) == [8388608, 8388609]
    # what the older tests hold to naming nothing still does, and so does the neighbourhood of every power of two above
    for lo, hi in ((393100, 393300), (786300, 786600), (1048500, 1048700), (2097100, 2097200), (2 ** 31 - 200, 2 ** 31 - 1),
                   (4194200, 4194400), (16777100, 16777300), (2 ** 30 - 100, 2 ** 30 + 100), (-300, 0)):
        assert all(row == NONE for row in table_of(program, lo, hi)), (lo, hi)


def test_every_older_number_is_described_as_before(program):
    """-8 ... 4100 against format_model and the older program's print, 8150 ... 8500 against packed_model, 32700 ... 33100 against
    packed16_model, 130900 ... 131400 against dword_model, 524000 ... 524800 against quad_model, job fields included; and nothing in
    the gaps"""
    rows, _ = format_dump.formats()
    for fmt, row in zip(range(fm.LO, fm.HI), table_of(program, fm.LO, fm.HI)):
        assert fm.Fmt(*row[:12]) == fm.describe(fmt), fmt
        assert (fm.Fmt(*row[:12]), tuple(row[12:])) == rows[fmt], fmt
        cls, storage, variant = fm.storage_of(fmt)
        assert (row[14], row[15], row[17]) == (cls, storage, variant), fmt
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
    for fmt, row in zip(range(lo, hi), table_of(program, lo, hi)):
        assert dm.Fmt(*row[:12]) == dm.describe(fmt) and tuple(row[12:]) == dm.job(fmt), fmt
    lo, hi = 524000, 524801
    seen = []
    for fmt, row in zip(range(lo, hi), table_of(program, lo, hi)):
        assert qm.Fmt(*row[:12]) == qm.describe(fmt) and tuple(row[12:]) == qm.job(fmt), fmt
        seen += [fmt] * row[0]
    assert seen == sorted(qm.FAMILY)
    gaps = ((4101, 4300), (33101, 33600), (130400, 130900), (131401, 131700), (196500, 196700), (262100, 262300), (523700, 524000), (524801, 525100))
    for lo, hi in gaps:
        assert all(row == NONE for row in table_of(program, lo, hi)), (lo, hi)


R11, E5 = um.R11G11B10F, um.RGB9E5
REFUSAL_CASES = [
    # (fmt, y, du, dv, pixel_stride, no_src, width), the three offsets in BYTES from a 16-byte boundary -> message
    *[((fmt, y, 0, 0, 1, 0, width), None) for fmt in um.FAMILY for y, width in ((0, 200), (4, 0), (-12, 1), (8, 200))],  # any dword; width 0
    *[((fmt, 0, du, dv, 1, 0, 200), um.LAYOUT_MSG) for fmt in um.FAMILY
      for du, dv in ((4, 8), (4, 4), (0, 4), (4, 0), (-4, 0), (1, 2), (1000, 2000))],  # unequal pointers
    *[((fmt, y, 0, 0, 1, 0, 200), um.LAYOUT_MSG) for fmt in um.FAMILY for y in (1, 2, 3, 5, 6, 7, -1, -2, -3)],  # off the dword
    *[((fmt, 0, 0, 0, ps, 0, 200), um.LAYOUT_MSG) for fmt in um.FAMILY for ps in (0, 2, 3, 4, -1)],
    ((R11, 1, 4, 8, 3, 1, 200), None),               # src NULL: the layout is not looked at
    ((E5, 3, 0, 0, 0, 1, 0), None),
    *[((fmt, 0, 0, 0, 1, 0, 200), "Invalid Sample Format") for fmt in (BASE - 1, BASE + 2, BASE + 3, BASE + 8, BASE + 64, BASE + 72, 2097152, 4194304, 16777216, 2 * BASE)],
    ((BASE + 2, 0, 0, 0, 1, 1, 200), "Invalid Sample Format"),
    # the other families keep their rules and their messages
    ((524296, 0, 0, 0, 1, 0, 200), None),
    ((524488, 4, 0, 0, 1, 0, 200), qm.LAYOUT_MSG),
    ((131072, 0, 0, 0, 1, 0, 200), None),
    ((131144, 2, 0, 0, 1, 0, 200), dm.LAYOUT_MSG),
    ((131073, 0, 0, 0, 2, 0, 200), dm.LAYOUT_MSG),
    ((32832, 0, 0, 0, 1, 0, 200), p6.LAYOUT_MSG),
    ((8192, 0, 0, 0, 1, 0, 200), pkm.LAYOUT_MSG),
    ((2112, 1, 1000, 2000, 100, 0, 200), "planar YCbCr of 16-bit words wants its three planes on 2-byte boundaries"),
    ((519, 0, 1, 3, 2, 0, 200), "planar YCbCr wants the chroma planes' pitch in pixel_stride"),
    ((80, 0, 2, 6, 1, 0, 200), "P010/P016 wants pixel_stride 1 and V one sample behind U"),
    ((16, 0, 1, 3, 2, 0, 200), "NV12 wants pixel_stride 1 and V one byte behind U"),
    ((2, 1, 0, 0, 1, 0, 200), None),
    ((3, 3, 1, 2, 3, 0, 200), None),
]


def test_the_refusals(program):
    data = struct.pack("<I", len(REFUSAL_CASES)) + b"".join(struct.pack("<7i", *case) for case, _ in REFUSAL_CASES)
    got = program("refusals", data=data).reshape(len(REFUSAL_CASES), 96)
    for field, (case, want) in zip(got, REFUSAL_CASES):
        message = bytes(field).split(b"\0")[0].decode()
        assert message == (want or ""), (case, message)
    fmt_h = open(os.path.join(hbuild.CSRC, "hyd_sample_fmt.h")).read()
    assert fmt_h.count('"' + um.LAYOUT_MSG + '"') == 1 and "HYD_FMT_UFLOAT_LAYOUT_MSG" in fmt_h  # one new message
    for old in (qm.LAYOUT_MSG, dm.LAYOUT_MSG, p6.LAYOUT_MSG, pkm.LAYOUT_MSG):
        assert fmt_h.count('"' + old + '"') == 1  # the old ones kept
    header = " ".join(open(os.path.join(ROOT, "include", "hydrium_amd.h")).read().replace("\n *", " ").split())
    assert um.LAYOUT_MSG in header
    assert "2097152" in fmt_h  # the header says why the next base of the sequence was passed over


def test_the_origins(program):
    cases = [(fmt, pitch, x0, y0) for fmt in um.FAMILY for pitch in (4096, -4096, 4099, -4099)
             for x0, y0 in ((0, 0), (256, 256), (1, 1), (257, 3), (33, 511))]
    data = struct.pack("<I", len(cases)) + b"".join(struct.pack("<4i", *c) for c in cases)
    got = program("origins", data=data).view(np.int64).reshape(len(cases), 3)
    for row, (fmt, pitch, x0, y0) in zip(got.tolist(), cases):
        assert row == [4 * (y0 * pitch + x0)] * 3, (fmt, pitch, x0, y0, row)  # y0 rows and x0 dwords, all three pointers: any x0 and y0


# ---- the definition ----
def test_the_definition_under_sanitizers_stays_inside_rows_between_guard_words(program):
    """every surface a malloc that ends with the last dword of its last row, rows of random dwords with guard words between them,
    top-down and bottom-up, widths 1 ... 9 and 33: the sanitizer is the bounds check, the guard words tell a read beyond a row's W
    dwords"""
    cases, wants = [], []
    for w in tuple(range(1, 10)) + (33,):
        for fmt in um.FAMILY:
            for n, (pitch, flip) in enumerate(((w, 0), (w + 5, 0), (w + 3, 1))):
                rows = random_dwords(w, HEIGHT, 99 + n)
                cases.append((fmt, rows, pitch, flip))
                wants.append(um.expected_bits(rows, fmt))
    for (fmt, rows, pitch, flip), got, want in zip(cases, pixels_of(program, cases), wants):
        assert same_bits(got, want), (fmt, rows.shape, pitch, flip)
    for fmt in um.FAMILY:
        other = random_dwords(33, HEIGHT, 99)
        guard = other.copy()
        guard[:, -1] = GUARD
        assert not np.array_equal(um.expected_bits(other, fmt), um.expected_bits(guard, fmt))  # the guard would have shown


def test_the_host_build_of_the_definition_equals_the_model(probe):
    check_definition(surface_hook(probe.hydt_ufloat_to_rgb_host))
    one, out = np.zeros((1, 1), np.uint32), np.zeros((1, 1, 3), np.uint32)
    fn = probe.hydt_ufloat_to_rgb_host
    for which, w, h in ((-1, 1, 1), (2, 1, 1), (0, 0, 1), (1, 1, 0), (0, 4097, 1)):
        assert fn(which, one.ctypes.data, out.ctypes.data, w, h) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_ufloat_widen_host", b"hydt_ufloat_widen_device", b"hydt_ufloat_to_rgb_host", b"hydt_ufloat_to_rgb_device"):
        assert name in probe and name not in shipped


# ---- names ----
def test_the_headers_names_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    body = re.search(r"\nenum \{\n\s*HYDAMD_R11G11B10F = (.*?)\n\};\n", text, re.S)
    assert body, "the two names sit in an anonymous enum"
    assert " ".join(("HYDAMD_R11G11B10F = " + body.group(1)).split()) == "HYDAMD_R11G11B10F = 8388608, HYDAMD_RGB9E5 = 8388609"
    assert (device.R11G11B10F, device.RGB9E5) == um.FAMILY == device.UFLOAT_FAMILY
    older = set(device.NV12_FAMILY) | set(device.P016_FAMILY) | set(device.PLANAR_FAMILY) | set(device.PLANAR16_FAMILY) | set(device.PACKED_FAMILY) | \
        set(device.PACKED16_FAMILY) | set(device.DWORD_FAMILY) | set(device.QUAD_FAMILY)
    assert not set(device.UFLOAT_FAMILY) & older and len(older) == 226 and len(device.DWORD_FAMILY) == 6 and len(device.QUAD_FAMILY) == 12
    assert "R11G11B10F" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    # neither is a numbered #define: the header's count of those is what it was
    assert not re.findall(r"^#define HYDAMD_(R11G11B10F|RGB9E5)\w* +-?\d+\s*$", text, re.M)
    assert len(re.findall(r"^#define HYDAMD_\w+ +-?\d+\s*$", text, re.M)) == 176
    # the older names keep their numbers
    assert (device.FLOAT16, device.BFLOAT16, device.NV12_BT709, device.I416_BT601_FULL, device.YUY2_BT709, device.Y216L_BT601_FULL, device.RGB10A2,
            device.Y410_BT601_FULL, device.AYUV_BT709, device.Y416_BT601_FULL) == (3, 4, 16, 2251, 8192, 32995, 131072, 131147, 524296, 524491)


def test_r11g11b10f_is_struck_from_the_dword_sections_out_of_scope_lists_and_has_a_section_of_its_own():
    for path in (os.path.join(ROOT, "include", "hydrium_amd.h"), os.path.join(ROOT, "DESIGN.md"), os.path.join(ROOT, "INTEGRATION.md")):
        text = " ".join(open(path).read().replace("\n *", " ").split())
        scopes = re.findall(r"(?:Out of scope|Not covered):.*?\.(?= [A-Z(#`]| \*/|$)", text)
        assert len(scopes) >= 10, path
        dword = [s for s in scopes if "bits 30" in s]  # the dword section's list: it no longer calls the format out of scope
        assert len(dword) == 1 and "R11G11B10F" not in dword[0], (path, dword)
        own = [s for s in scopes if "16-bit-per-channel float" in s]
        assert len(own) == 1, (path, own)
        for word in ("signed", "alpha", "PQ / HLG / BT.2020", "host-pointer input"):
            assert word in own[0], (path, word)
        for word in ("AYUV", "Y416", "ayuv64le"):  # the quad section's list stays the only one with these
            assert word not in own[0], (path, word)
        for word in ("R11G11B10F", "RGB9E5", "8388608", "8388609", "R11G11B10_FLOAT", "R9G9B9E5_SHAREDEXP", "B10G11R11_UFLOAT_PACK32", "E5B9G9R9_UFLOAT_PACK32"):
            assert word in text, (path, word)
    header = " ".join(open(os.path.join(ROOT, "include", "hydrium_amd.h")).read().replace("\n *", " ").split())
    assert "every other number from 8388608 up names nothing" in header and "from 524288 up to 8388607" in header


def test_the_wrappers_name_their_format_and_fill_a_descriptor():
    import torch
    from hydrium_amd import device

    for w, h in ((1, 5), (8, 8), (33, 9), (200, 120)):
        for dtype in (torch.int32, torch.uint32):
            buf = torch.zeros(h * (w + 6) + 3, dtype=dtype)
            surface = buf.as_strided((h, w), (w + 6, 1), 3)
            for cls, fmt in ((device.R11g11b10f, um.R11G11B10F), (device.Rgb9e5, um.RGB9E5)):
                pic = cls(surface, w)
                assert isinstance(pic, device.Nv12) and device.sample_fmt_of(pic) == fmt == pic.sample_fmt and pic.shape == (h, w, 3)
                assert (pic.pitch, pic.pixel_stride) == (w + 6, 1)  # in dwords
                assert pic.pointers() == [buf.data_ptr() + 12] * 3
                descs, got = device.mixed_descriptors([pic])
                d = descs[0]
                assert got == [fmt] and (d.row_stride, d.pixel_stride, d.width, d.height) == (w + 6, 1, w, h)
                assert [d.src[0], d.src[1], d.src[2]] == pic.pointers()
    surface = torch.zeros((120, 200), dtype=torch.int32)
    assert device.R11g11b10f(surface, 199).width == 199 and device.Rgb9e5(surface, 57).pitch == 200  # a wider surface
    crop = device.R11g11b10f(surface[3:, 5:], 100)  # any x0 and y0, odd ones too
    assert crop.pointers() == [surface.data_ptr() + 4 * (3 * 200 + 5)] * 3 and (crop.height, crop.pitch, crop.sample_fmt) == (117, 200, 8388608)
    f32 = torch.zeros((120, 200, 3), dtype=torch.float32)
    f16 = torch.zeros((120, 200, 3), dtype=torch.float16)
    got = device.mixed_descriptors([crop, f32, device.Rgb9e5(surface, 200), f16, device.Rgb10(surface, 200, "bgr"), device.Ayuv(surface, 200)],
                                   sample_fmts="each")[1]
    assert got == [8388608, 2, 8388609, 3, 131073, 524296]


def test_the_wrappers_refuse_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    surface = torch.zeros((10, 36), dtype=torch.int32)
    for cls in (device.R11g11b10f, device.Rgb9e5):
        with pytest.raises(ValueError, match="width dwords"):  # a row too short for the width
            cls(surface, 37)
        with pytest.raises(ValueError, match="width dwords"):
            cls(surface, 0)
        with pytest.raises(ValueError, match="unit element stride"):
            cls(torch.zeros((10, 72), dtype=torch.int32)[:, ::2], 18)
        for other in (torch.uint8, torch.int16, torch.float16, torch.float32, torch.int64, torch.float64):  # wrong dtype: a float32 tensor is no packed surface
            with pytest.raises(ValueError, match="4-byte integer"):
                cls(torch.zeros((10, 36), dtype=other), 18)
        with pytest.raises(ValueError, match="4-byte integer"):
            cls(torch.zeros((10, 36, 1), dtype=torch.int32), 18)
        with pytest.raises(TypeError):
            cls.from_surface(surface, 18, 10, 36, 0)
        with pytest.raises(TypeError):  # no order and no matrix to name
            cls(surface, 18, "bgr")


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((24, 16), np.uint32)
    for fmt in um.FAMILY:
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p, p], 0, 0, 16, 1, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_two_new_instances_have_a_symbol_of_their_own_and_the_float32_instances_footprint():
    """k_transform_tokenize_ufloat<HYDK_STORE_R11G11B10F | _RGB9E5>: none under an older symbol name, the older kernels' counts as they
    are, no scratch and no more LDS than the float32 instance (the register count is printed, not held to a number)"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_ufloat" in k}
    assert sorted(re.match(r"_Z27k_transform_tokenize_ufloatILi(\d+)EE", k).group(1) for k in new) == ["19", "20"], sorted(res)
    older = ("k_transform_tokenize_planar", "k_transform_tokenize_p016", "k_transform_tokenize_yuvp16", "k_transform_tokenize_yuy2", "k_transform_tokenize_y216",
             "k_transform_tokenize_dword", "k_transform_tokenize_quad", "_Z20k_transform_tokenizeI")
    assert not any(o in k for k in new for o in older)
    count = lambda stem: sum(stem in k for k in res)
    assert [count(o) for o in older] == [6, 6, 6, 6, 6, 6, 6, 19]
    float32 = [v for k, v in res.items() if k.startswith("_Z20k_transform_tokenizeILi2ELi1ELi0EE")]
    assert len(float32) == 1
    for name, d in sorted(new.items()):
        print(name, d, "float32:", float32[0])
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= float32[0]["group_segment_fixed_size"], (name, d)
