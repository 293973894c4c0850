"""CPU-only: the formats whose pixel is one dword of three 10-bit fields (HYDAMD_RGB10A2, HYDAMD_BGR10A2, HYDAMD_Y410_*) where no
device is needed — the descriptor, the refusals and the origins of csrc/hyd_sample_fmt.h and the round trip of csrc/hip/hydk_store.h
against a model written from the prose, with every older number's description unchanged; the per-pixel definition
(csrc/hip/hydk_rgb10.h) as plain C++ under address and UB sanitizers, and as the probe library's host build, against dword_model.py;
device.Rgb10's and device.Y410's reading of their surface; the drop-in API's refusal; the header's names; and what the six new
instances of the transform kernel ask of a compute unit.  Every test here fails on the parent, where 131072 is "Invalid Sample
Format"."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import dword_model as dm
import format_dump
import format_model as fm
import packed16_model as p6
import packed_model as pkm
import planar16_model as p16m
import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 7, 8, 9, 33)
HEIGHT = 3
LO, HI = 130900, 131401
# (ycbcr, which) of the C side for each of the six numbers: the RGB order, or Y410's matrix
FORMS = {131072: (0, 0), 131073: (0, 1), **{f: (1, dm.matrix_of(f)) for f in dm.Y410}}


def random_dwords(w, h, seed=131072):
    """h rows of w random dwords, all 32 bits random: the spare bits set, YCbCr codes far out of range"""
    return np.random.default_rng(seed + 100 * w + h).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


def check_definition(to_rgb, widths=WIDTHS, height=HEIGHT):
    """to_rgb(ycbcr, which, dwords, w, h) -> (h, w, 3) uint16, held to the model over all six formats on random dwords and on
    all-ones (the top of the range: nothing may wrap).  Shared with the on-device test."""
    for w in widths:
        for fmt, (ycbcr, which) in FORMS.items():
            for dwords in (random_dwords(w, height, fmt), np.full((height, w), 0xFFFFFFFF, np.uint32)):
                got, want = to_rgb(ycbcr, which, dwords, w, height), dm.expected_rgb(dwords, fmt)
                assert got.dtype == np.uint16 and got.shape == want.shape == (height, w, 3)
                wrong = np.argwhere(got != want)
                assert wrong.size == 0, (fmt, w, [(tuple(p), int(got[tuple(p)]), int(want[tuple(p)])) for p in wrong[:8]])


def hook(fn, *device):
    """a probe-flavour dword entry as to_rgb(ycbcr, which, dwords, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def to_rgb(ycbcr, which, dwords, w, h):
        dwords = np.ascontiguousarray(dwords)
        out = np.full((h, w, 3), 0xA5A5, np.uint16)
        assert fn(*device, ycbcr, which, dwords.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return to_rgb


@pytest.fixture(scope="module")
def program():
    """tests/c/dword_formats.cc: hyd_sample_fmt.h, hydk_store.h and hydk_rgb10.h with g++ under address and UB sanitizers, no HIP
    header, no warning"""
    return format_dump.sanitized_program("dword_formats")


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


def table_of(program, lo, hi):
    return program("describe", lo, hi).view(np.int32).reshape(hi - lo, 18).tolist()


# ---- the model ----
def test_the_model_takes_apart_what_it_put_together():
    rng = np.random.default_rng(1)
    f = [rng.integers(0, 1024, (HEIGHT, 9), dtype=np.uint16) for _ in range(3)]
    for spare in range(4):
        d = dm.pack(*f, spare)
        assert d.dtype == np.uint32 and all(np.array_equal(a, b) for a, b in zip(dm.fields(d), f))
        assert np.array_equal(d >> 30, np.full(d.shape, spare))
    assert dm.pack([1], [2], [3]).tolist() == [1 | 2 << 10 | 3 << 20]
    assert dm.widen([0, 1, 9, 511, 512, 1023]).tolist() == [0, 64, 577, 32735, 32800, 65535]
    # no v lands on a tie: 2 * ((v * 65535) mod 1023) is never 1023
    assert all((2 * ((v * 65535) % 1023)) != 1023 for v in range(1024))


# ---- the descriptor ----
def test_the_descriptor_of_every_number_from_130900_to_131400(program):
    table = table_of(program, LO, HI)
    formats = []
    for fmt, row in zip(range(LO, HI), table):
        got, job = dm.Fmt(*row[:12]), tuple(row[12:])
        assert got == dm.describe(fmt), (fmt, got)
        assert job == dm.job(fmt), (fmt, job)
        if got.device:
            formats.append(fmt)
            assert (got.device, got.host, got.is_float, got.bytes, got.bits, got.layout, got.filter, got.sx, got.sy) == (1, 0, 0, 4, 10, 4, 0, 0, 0)
    assert formats == sorted(dm.FAMILY) == [131072, 131073, 131144, 131145, 131146, 131147]  # exactly six
    by_number = dict(zip(range(LO, HI), table))
    for fmt in (131074, 131076, 131088, 131136, 131143, 131148, 131152, 131160, 131208, 131272):
        assert by_number[fmt] == [0] * 12 + [0, -1, 0, 0, 0, 0], fmt
    for lo, hi in ((131401, 131700), (196500, 196700), (262100, 262300), (2 ** 31 - 200, 2 ** 31 - 1)):
        assert all(row == [0] * 12 + [0, -1, 0, 0, 0, 0] for row in table_of(program, lo, hi)), (lo, hi)


def test_every_older_number_is_described_as_before(program):
    """-8 ... 4100 against format_model and the older program's print, 8150 ... 8500 against packed_model, 32700 ... 33100 against
    packed16_model, job fields included; and nothing in the gaps"""
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
    seen = 0
    for fmt, row in zip(range(lo, hi), table_of(program, lo, hi)):
        want = p6.describe(fmt)
        assert p6.Fmt(*row[:12]) == want, fmt
        interp = int(want.filter != 0)
        assert tuple(row[12:]) == ((1, fmt, 1, 13 + interp, want.matrix + 4 * want.depth, 8192 << interp) if want.device else (0, -1, 0, 0, 0, 0)), fmt
        seen += want.device
    assert seen == 36 and p6.describe(32995).device and not p6.describe(32996).device  # the Y216 family ends at 32995
    gaps = ((4101, 4300), (12200, 12400), (16300, 16500), (24500, 24700), (32600, 32700), (33101, 33300), (65400, 65700), (2 ** 31 - 200, 2 ** 31 - 1),
            (33101, 33600), (130400, 130900))  # (the last two: both ends of 33101 ... 130899)
    for lo, hi in gaps:
        assert all(row == [0] * 12 + [0, -1, 0, 0, 0, 0] for row in table_of(program, lo, hi)), (lo, hi)


REFUSAL_CASES = [
    # (fmt, y, du, dv, pixel_stride, no_src, width), the three offsets in BYTES -> message
    *[((fmt, y, 0, 0, 1, 0, width), None) for fmt in dm.FAMILY for y, width in ((0, 200), (4, 0), (-8, 1))],
    *[((fmt, 0, du, dv, 1, 0, 200), dm.LAYOUT_MSG) for fmt in (131072, 131073, 131144, 131147)
      for du, dv in ((4, 8), (4, 4), (0, 4), (4, 0), (-4, 0), (1, 2), (2, 4), (1000, 2000))],  # unequal pointers
    *[((fmt, y, 0, 0, 1, 0, 200), dm.LAYOUT_MSG) for fmt in (131072, 131145) for y in (1, 2, 3, 5, -1, -2)],  # an address off the dword
    *[((fmt, 0, 0, 0, ps, 0, 200), dm.LAYOUT_MSG) for fmt in (131072, 131073, 131146) for ps in (0, 2, 3, -1, 4)],
    ((131072, 1, 4, 8, 3, 1, 200), None),               # src NULL: the layout is not looked at
    ((131147, 3, 0, 0, 0, 1, 0), None),
    *[((fmt, 0, 0, 0, 1, 0, 200), "Invalid Sample Format") for fmt in (131071, 131074, 131076, 131143, 131148, 131208, 131272, 262144)],
    ((131074, 0, 0, 0, 1, 1, 200), "Invalid Sample Format"),
    # the other families keep their rules and their messages
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
    assert fmt_h.count('"' + dm.LAYOUT_MSG + '"') == 1 and "HYD_FMT_DWORD_LAYOUT_MSG" in fmt_h  # one new message
    assert fmt_h.count('"' + p6.LAYOUT_MSG + '"') == 1 and fmt_h.count('"' + pkm.LAYOUT_MSG + '"') == 1  # the old ones kept
    header = " ".join(open(os.path.join(ROOT, "include", "hydrium_amd.h")).read().replace("\n *", " ").split())
    assert dm.LAYOUT_MSG in header


def test_the_origins(program):
    cases = [(fmt, pitch, x0, y0) for fmt in (131072, 131073, 131144, 131147) for pitch in (4096, -4096, 4099, -4099)
             for x0, y0 in ((256, 256), (2048, 0), (0, 0), (0, 768), (1, 1), (257, 3), (33, 511))]
    data = struct.pack("<I", len(cases)) + b"".join(struct.pack("<4i", *c) for c in cases)
    got = program("origins", data=data).view(np.int64).reshape(len(cases), 3)
    for row, (fmt, pitch, x0, y0) in zip(got.tolist(), cases):
        # y0 rows and x0 DWORDS, added to all three pointers (bytes here: four a dword): any x0 and y0
        assert row == [4 * (y0 * pitch + x0)] * 3, (fmt, pitch, x0, y0, row)


# ---- the definition ----
def test_all_1024_field_values_widen_to_the_nearest_sixteen_bit_sample(program):
    got = program("widen").view(np.uint32).reshape(1024, 2)
    want = [(v * 65535 + 511) // 1023 for v in range(1024)]
    assert got[:, 0].tolist() == want and got[:, 1].tolist() == want  # the cheaper formula is held to the division on every value
    assert want[0] == 0 and want[1023] == 65535 and want[9] != (9 << 6 | 9 >> 4)  # bit replication is another function
    assert all(abs(s / 65535 - v / 1023) <= 0.5 / 65535 for v, s in enumerate(want))


def test_every_field_value_in_every_position_in_both_orders(program, probe):
    """all 1024 values in each of the three positions, the other fields random; the spare bits at 0 and at 3 give the same pixels"""
    rng = np.random.default_rng(10)
    v = np.arange(1024, dtype=np.uint32).reshape(1, 1024)
    host = hook(probe.hydt_dword_to_rgb_host)
    cases, blob, wants = [], [], []
    for pos in range(3):
        others = [rng.integers(0, 1024, (1, 1024), dtype=np.uint32) for _ in range(3)]
        others[pos] = v
        for order, fmt in enumerate(dm.RGB_FORMS):
            channel = pos if order == 0 else 2 - pos
            pics = []
            for spare in (0, 3):
                d = dm.pack(*others, spare)
                want = dm.expected_rgb(d, fmt)
                assert want[0, :, channel].tolist() == [(x * 65535 + 511) // 1023 for x in range(1024)]
                assert np.array_equal(host(0, order, d, 1024, 1), want)
                cases.append(want)
                blob.append(struct.pack("<6I", 0, order, 1024, 1, 1024, 0) + d.tobytes())
                pics.append(want)
            assert np.array_equal(pics[0], pics[1])
    got = program("pixels", data=struct.pack("<I", len(cases)) + b"".join(blob)).view(np.uint16).reshape(len(cases), 1, 1024, 3)
    for g, want in zip(got, cases):
        assert np.array_equal(g, want)


def test_a_y410_picture_is_the_i410_picture_of_its_fields():
    for w in WIDTHS:
        for fmt in dm.Y410:
            m = dm.matrix_of(fmt)
            for dwords in (random_dwords(w, HEIGHT, 5 + m), np.full((HEIGHT, w), 0xFFFFFFFF, np.uint32)):
                u, y, v = dm.fields(dwords)
                assert y.shape == u.shape == v.shape == (HEIGHT, w) and int(max(y.max(), u.max(), v.max())) < 1024
                assert p16m.is_format(2120 + m) and p16m.public_name(2120 + m).startswith("I410_")
                assert np.array_equal(dm.expected_rgb(dwords, fmt), p16m.expected_rgb((y, u, v), 2120 + m))
                assert np.array_equal(dm.expected_rgb(dwords, fmt), dm.expected_rgb(dwords & 0x3FFFFFFF, fmt))  # bits 30, 31 never matter
    # and the matrices are four pictures
    d = random_dwords(33, HEIGHT, 6)
    assert len({dm.expected_rgb(d, f).tobytes() for f in dm.Y410}) == 4


def test_the_definition_under_sanitizers_stays_inside_rows_between_guard_dwords(program):
    """every surface a malloc that ends with the last dword of its last row, rows of random dwords with 0x5A5A5A5A between them,
    top-down and bottom-up: the sanitizer is the bounds check, the guard dwords tell a read beyond a row's W dwords"""
    cases, blob = [], []
    for w in WIDTHS:
        for fmt, (ycbcr, which) in FORMS.items():
            for n, (pitch, flip) in enumerate(((w, 0), (w + 5, 0), (w + 3, 1))):
                rows = random_dwords(w, HEIGHT, 99 + fmt) if n else np.full((HEIGHT, w), 0xFFFFFFFF, np.uint32)
                if n == 0 and fmt % 2:  # the packed pitch sees random dwords too
                    rows = random_dwords(w, HEIGHT, 7 + fmt)
                want = dm.expected_rgb(rows, fmt)
                surface = np.full(pitch * (HEIGHT - 1) + w, 0x5A5A5A5A, np.uint32)
                for r in range(HEIGHT):
                    at = pitch * (HEIGHT - 1 - r if flip else r)
                    surface[at:at + w] = rows[r]
                cases.append((fmt, w, want))
                blob.append(struct.pack("<6I", ycbcr, which, w, HEIGHT, pitch, flip) + surface.tobytes())
    got = program("pixels", data=struct.pack("<I", len(cases)) + b"".join(blob)).view(np.uint16)
    at = 0
    for fmt, w, want in cases:
        n = HEIGHT * w * 3
        assert np.array_equal(got[at:at + n].reshape(HEIGHT, w, 3), want), (fmt, w)
        at += n
    assert at == got.size
    other = random_dwords(33, HEIGHT, 99)
    guard = other.copy()
    guard[:, -1] = 0x5A5A5A5A
    assert all(not np.array_equal(dm.expected_rgb(other, f), dm.expected_rgb(guard, f)) for f in dm.FAMILY)  # the guard would have shown


def test_the_host_build_of_the_definition_equals_the_model(probe):
    check_definition(hook(probe.hydt_dword_to_rgb_host))
    one, out = np.zeros((1, 1), np.uint32), np.zeros((1, 1, 3), np.uint16)
    fn = probe.hydt_dword_to_rgb_host
    for ycbcr, which in ((-1, 0), (2, 0), (0, 2), (0, -1), (1, 4), (1, -1)):
        assert fn(ycbcr, which, one.ctypes.data, out.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_dword_to_rgb_host", b"hydt_dword_to_rgb_device"):
        assert name in probe and name not in shipped


# ---- names ----
def test_the_headers_names_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    body = re.search(r"\nenum \{\n\s*HYDAMD_RGB10A2 = (.*?)\n\};\n", text, re.S)
    assert body, "the six names sit in an anonymous enum"
    flat = " ".join(("HYDAMD_RGB10A2 = " + body.group(1)).split())
    assert flat == ("HYDAMD_RGB10A2 = 131072, HYDAMD_BGR10A2 = 131073, HYDAMD_Y410_BT709 = 131072 + 4 * 2 + 64 * 1, HYDAMD_Y410_BT709_FULL, "
                    "HYDAMD_Y410_BT601, HYDAMD_Y410_BT601_FULL")
    want = {"HYDAMD_" + dm.public_name(fmt): fmt for fmt in dm.FAMILY}
    assert want == {"HYDAMD_RGB10A2": 131072, "HYDAMD_BGR10A2": 131073, "HYDAMD_Y410_BT709": 131144, "HYDAMD_Y410_BT709_FULL": 131145,
                    "HYDAMD_Y410_BT601": 131146, "HYDAMD_Y410_BT601_FULL": 131147}
    for name, fmt in want.items():
        assert getattr(device, name[len("HYDAMD_"):]) == fmt and name in text
    assert device.DWORD_FAMILY == dm.FAMILY and device.Y410_FORMATS == dm.Y410
    for fmt in dm.Y410:
        assert device.ycbcr_fields(fmt) == (131072, dm.matrix_of(fmt), 2, 0, 1)
    older = set(device.NV12_FAMILY) | set(device.P016_FAMILY) | set(device.PLANAR_FAMILY) | set(device.PLANAR16_FAMILY) | set(device.PACKED_FAMILY) | \
        set(device.PACKED16_FAMILY)
    assert not set(device.DWORD_FAMILY) & older and len(older) == 208
    assert "RGB10" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    # none of them is a numbered #define: the header's count of those is what it was
    assert not re.findall(r"^#define HYDAMD_(RGB10|BGR10|Y410)\w* +-?\d+\s*$", text, re.M)
    assert len(re.findall(r"^#define HYDAMD_\w+ +-?\d+\s*$", text, re.M)) == 176
    # the older names keep their numbers
    assert (device.NV12_BT709, device.P016L_BT601_FULL, device.I420_BT709, device.I410_BT709, device.I416_BT601_FULL, device.YUY2_BT709,
            device.YUY2L_BT601_FULL, device.Y210_BT709, device.Y216L_BT601_FULL) == (16, 243, 512, 2120, 2251, 8192, 8227, 32832, 32995)
    for fmt in p6.FAMILY:
        assert device.ycbcr_fields(fmt) == (32768, p6.matrix_of(fmt), 0, p6.filter_of(fmt), p6.depth_of(fmt))


def test_y410_is_struck_from_the_older_out_of_scope_lists():
    for path in (os.path.join(ROOT, "include", "hydrium_amd.h"), os.path.join(ROOT, "DESIGN.md"), os.path.join(ROOT, "INTEGRATION.md")):
        text = " ".join(open(path).read().replace("\n *", " ").split())
        for scope in re.findall(r"Out of scope[^.]*\.", text):
            assert "Y410 /" not in scope and "/ Y410" not in scope and "AYUV / Y410" not in scope, (path, scope)
        assert "131072" in text and "Y416" in text and "R11G11B10F" in text, path


def test_rgb10_and_y410_name_their_format_and_fill_a_descriptor():
    import torch
    from hydrium_amd import device

    for w, h in ((1, 5), (8, 8), (33, 9), (200, 120)):
        for dtype in (torch.int32, torch.uint32):
            buf = torch.zeros(h * (w + 6) + 3, dtype=dtype)
            surface = buf.as_strided((h, w), (w + 6, 1), 3)
            pics = [device.Rgb10(surface, w), device.Rgb10(surface, w, "bgr"), device.Rgb10(surface, w, order="RGB")] + \
                [device.Y410(surface, w, 16 + m) for m in ym.MATRICES] + [device.Y410(surface, w, f) for f in dm.Y410]
            fmts = [131072, 131073, 131072, 131144, 131145, 131146, 131147, 131144, 131145, 131146, 131147]
            for pic, fmt in zip(pics, fmts):
                assert isinstance(pic, device.Rgb10) and isinstance(pic, device.Nv12)
                assert device.sample_fmt_of(pic) == fmt == pic.sample_fmt and pic.shape == (h, w, 3)
                assert (pic.pitch, pic.pixel_stride) == (w + 6, 1)  # in dwords
                assert pic.pointers() == [buf.data_ptr() + 12] * 3
                descs, got = device.mixed_descriptors([pic])
                d = descs[0]
                assert got == [fmt] and (d.row_stride, d.pixel_stride, d.width, d.height) == (w + 6, 1, w, h)
                assert [d.src[0], d.src[1], d.src[2]] == pic.pointers()
    surface = torch.zeros((120, 200), dtype=torch.int32)
    assert device.Rgb10(surface, 200).order == "rgb" and device.Y410(surface, 200).sample_fmt == device.Y410_BT709 == 131144
    assert device.Rgb10(surface, 199).width == 199 and device.Rgb10(surface, 57).pitch == 200  # a wider surface
    crop = device.Y410(surface[3:, 5:], 100)  # any x0 and y0
    assert crop.pointers() == [surface.data_ptr() + 4 * (3 * 200 + 5)] * 3 and (crop.height, crop.pitch) == (117, 200)
    rgb16 = torch.zeros((120, 200, 3), dtype=torch.int16)
    y210 = device.PackedYuv16(torch.zeros((120, 400), dtype=torch.int16), 200)
    assert device.mixed_descriptors([device.Rgb10(surface, 200, "bgr"), rgb16, y210, crop], sample_fmts="each")[1] == [131073, 1, 32832, 131144]


def test_rgb10_and_y410_refuse_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    surface = torch.zeros((10, 36), dtype=torch.int32)
    with pytest.raises(ValueError, match="width dwords"):  # a row too short for the width
        device.Rgb10(surface, 37)
    with pytest.raises(ValueError, match="width dwords"):
        device.Y410(surface, 0)
    with pytest.raises(ValueError, match="unit element stride"):
        device.Rgb10(torch.zeros((10, 72), dtype=torch.int32)[:, ::2], 18)
    for other in (torch.uint8, torch.int16, torch.float16, torch.float32, torch.int64):
        for cls in (device.Rgb10, device.Y410):
            with pytest.raises(ValueError, match="4-byte integer"):
                cls(torch.zeros((10, 36), dtype=other), 18)
    with pytest.raises(ValueError, match="4-byte integer"):
        device.Rgb10(torch.zeros((10, 18, 2), dtype=torch.int32), 18)
    for bad in ("rbg", "argb", 0):
        with pytest.raises(ValueError, match="order"):
            device.Rgb10(surface, 18, order=bad)
    for bad in (0, 1, 32, 80, 2120, 8192, 32832, 131072, 131073, 131148):  # one of the four matrices, or one of the four numbers
        with pytest.raises(ValueError):
            device.Y410(surface, 18, bad)
    for cls in (device.Rgb10, device.Y410):
        with pytest.raises(TypeError):
            cls.from_surface(surface, 18, 10, 36, 0)
    with pytest.raises(ValueError, match="2-byte integer"):  # and the 16-bit family keeps to words
        device.PackedYuv16(surface, 9)


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((24, 16), np.uint32)
    for fmt in dm.FAMILY:
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p, p], 0, 0, 16, 1, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_six_new_instances_have_symbols_of_their_own_and_keep_the_transform_kernels_contract():
    """k_transform_tokenize_dword<mode, HYDK_STORE_RGB10 | _Y410>: none under an older symbol name, no scratch, no more LDS than the
    Y216 instances, and the register line every family is held to"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_dword" in k}
    assert sorted(re.match(r"_Z26k_transform_tokenize_dwordILi(\d)ELi(\d+)EE", k).groups() for k in new) == \
        [(mode, store) for mode in "012" for store in ("15", "16")], sorted(res)
    older = ("k_transform_tokenize_planar", "k_transform_tokenize_p016", "k_transform_tokenize_yuvp16", "k_transform_tokenize_yuy2", "k_transform_tokenize_y216",
             "_Z20k_transform_tokenizeI")
    assert not any(o in k for k in new for o in older)
    count = lambda stem: sum(stem in k for k in res)
    assert [count(o) for o in older] == [6, 6, 6, 6, 6, 19]
    y216_lds = max(d["group_segment_fixed_size"] for k, d in res.items() if "k_transform_tokenize_y216" in k)
    assert y216_lds == 31856
    for name, d in sorted(new.items()):
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= y216_lds and d["next_free_vgpr"] <= 128, (name, d)
