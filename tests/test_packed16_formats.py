"""CPU-only: the packed 4:2:2 YCbCr formats of 16-bit words (HYDAMD_Y210_*, HYDAMD_Y212_*, HYDAMD_Y216_* and their C / L forms: four
word orders by the pointers) where no device is needed — the descriptor, the refusals and the origins of csrc/hyd_sample_fmt.h and
the round trip of csrc/hip/hydk_store.h against a model written from the prose, with every older number's description unchanged;
the per-pixel definition (csrc/hip/hydk_y216.h) as plain C++ under address and UB sanitizers, and as the probe library's host build,
against packed16_model.py; device.PackedYuv16's reading of its surface; the drop-in API's refusal; the header's names; and what the
six new instances of the transform kernel ask of a compute unit.  Every test here fails on the parent, where 32832 is "Invalid
Sample Format"."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import chroma_model as cm
import format_dump
import format_model as fm
import packed16_model as p6
import packed_model as pkm
import planar16_model as p16m
import planar_model as plm
import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 7, 8, 9, 33)
HEIGHT = 3
LO, HI = 32700, 33101


def random_rows(w, h, seed=32768):
    """h rows of 4 * ceil(w / 2) random full 16-bit words: low bits set at every depth"""
    return np.random.default_rng(seed + 100 * w + h).integers(0, 65536, (h, 4 * ((w + 1) // 2)), dtype=np.uint16)


def check_definition(to_rgb, widths=WIDTHS, height=HEIGHT):
    """to_rgb(order index, filter, depth, matrix, rows, w, h) -> (h, w, 3) uint16, held to the model over every word order x filter x
    depth x matrix on random full words and on all-65535 (the top of the range: nothing may wrap).  Shared with the on-device test."""
    for w in widths:
        for k, order in enumerate(p6.ORDER_NAMES):
            for filt in cm.FILTERS:
                for d in p6.DEPTHS:
                    for m in ym.MATRICES:
                        for rows in (random_rows(w, height, 32768 + k), np.full((height, 4 * ((w + 1) // 2)), 65535, np.uint16)):
                            got, want = to_rgb(k, filt, d, m, rows, w, height), p6.expected_rgb(rows, order, w, p6.sample_fmt(m, filt, d))
                            assert got.dtype == np.uint16 and got.shape == want.shape == (height, w, 3)
                            wrong = np.argwhere(got != want)
                            assert wrong.size == 0, (order, cm.FILTER_NAMES[filt], d, m, w,
                                                     [(tuple(p), int(got[tuple(p)]), int(want[tuple(p)])) for p in wrong[:8]])


def hook(fn, *device):
    """a probe-flavour packed16 entry as to_rgb(order, filter, depth, matrix, rows, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def to_rgb(order, filt, d, m, rows, w, h):
        rows = np.ascontiguousarray(rows)
        out = np.full((h, w, 3), 0xA5A5, np.uint16)
        assert fn(*device, order, filt, d, m, rows.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return to_rgb


@pytest.fixture(scope="module")
def program():
    """tests/c/packed16_formats.cc: hyd_sample_fmt.h, hydk_store.h and hydk_y216.h with g++ under address and UB sanitizers, no HIP
    header, no warning"""
    return format_dump.sanitized_program("packed16_formats")


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


# ---- the model ----
def test_the_model_takes_apart_what_it_put_together_and_the_orders_are_the_headers():
    assert p6.ORDERS == pkm.ORDERS == {"yuyv": (1, 3), "yvyu": (3, 1), "uyvy": (-1, 1), "vyuy": (1, -1)}
    rng = np.random.default_rng(1)
    for w in WIDTHS:
        cw = (w + 1) // 2
        planes = tuple(rng.integers(0, 65536, s, dtype=np.uint16) for s in ((HEIGHT, w), (HEIGHT, cw), (HEIGHT, cw)))
        seen = set()
        for order in p6.ORDER_NAMES:
            rows = p6.interleave(planes, order, w)
            assert rows.shape == (HEIGHT, 4 * cw) and rows.dtype == np.uint16
            assert all(np.array_equal(a, b) for a, b in zip(p6.deinterleave(rows, order, w), planes))
            seen.add(rows.tobytes())
        assert len(seen) == 4
    one = (np.array([[1, 2]], np.uint16), np.array([[3]], np.uint16), np.array([[4]], np.uint16))
    assert p6.interleave(one, "yuyv", 2).tolist() == [[1, 3, 2, 4]]  # Y210 as everybody writes it: Y0 U Y1 V
    assert p6.interleave(one, "uyvy", 2).tolist() == [[3, 1, 4, 2]]
    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    assert "(1, 3) Y210's own order Y U Y V, (3, 1) Y V Y U, (-1, 1) U Y V Y, (1, -1) V Y U Y" in text


def test_the_consequences_the_picture_is_the_i216_picture_and_the_shifted_i210_picture():
    for w in WIDTHS:
        rows = random_rows(w, HEIGHT, 5)
        for order in p6.ORDER_NAMES:
            planes = p6.deinterleave(rows, order, w)
            for fmt in p6.FAMILY:
                planar = p6.as_i2xx(fmt)
                assert p16m.is_format(planar) and p16m.sub_of(planar) == plm.S422 and p16m.depth_of(planar) == p6.depth_of(fmt)
                shift = 16 - p6.bits_of(fmt)
                clean = (rows >> shift) << shift  # the low bits zero: the LSB-aligned planes of the words >> shift are this picture
                assert np.array_equal(p6.expected_rgb(clean, order, w, fmt),
                                      p16m.expected_rgb(tuple(p >> shift for p in p6.deinterleave(clean, order, w)), planar))
                if shift == 0:
                    assert np.array_equal(p6.expected_rgb(rows, order, w, fmt), p16m.expected_rgb(planes, planar))
    # and the low bits count: the same words with them set are another picture
    rows = random_rows(33, HEIGHT, 6) | 0x3F
    assert not np.array_equal(p6.expected_rgb(rows, "yuyv", 33, 32832), p6.expected_rgb(rows & 0xFFC0, "yuyv", 33, 32832))


# ---- the descriptor ----
def test_the_descriptor_of_every_number_from_32700_to_33100(program):
    table = program("describe", LO, HI).view(np.int32).reshape(HI - LO, 18).tolist()
    formats = []
    for fmt, row in zip(range(LO, HI), table):
        got, job = p6.Fmt(*row[:12]), tuple(row[12:])
        want = p6.describe(fmt)
        assert got == want, (fmt, got, want)
        if want.device:
            formats.append(fmt)
            assert (got.bytes, got.sub, got.sx, got.sy, got.device, got.host, got.layout) == (2, 1, 1, 0, 1, 0, 3)
            assert got.depth in (1, 2, 3) and got.bits == {1: 10, 2: 12, 3: 16}[got.depth]
            # 16-bit class, storage form 13 (nearest) or 14 (interpolated), variant bits 8192 and 16384, a job's matrix = matrix + 4 *
            # depth as for P016; and the number comes back
            interp = int(got.filter != 0)
            assert job == (1, fmt, 1, 13 + interp, got.matrix + 4 * got.depth, 8192 << interp), (fmt, job)
        else:
            assert job == (0, -1, 0, 0, 0, 0), (fmt, job)
    want = [base + 16 * f + m for base in (32832, 32896, 32960) for f in range(3) for m in range(4)]
    assert formats == want == sorted(p6.FAMILY) and len(formats) == 36 and formats[-1] == 32995
    by_number = dict(zip(range(LO, HI), table))
    for fmt in list(range(32700, 32832)) + [32836, 32847, 32880, 32895, 32944, 33008, 33023, 33024, 33100]:
        assert by_number[fmt][:12] == [0] * 12, fmt  # below the base and depth 0; the subsampling bits; filter 3; depth 4


def test_every_older_number_is_described_as_before(program):
    """-8 ... 4100 against format_model, 8150 ... 8500 against packed_model, job fields included; and a few between the families"""
    table = program("describe", fm.LO, fm.HI).view(np.int32).reshape(fm.HI - fm.LO, 18).tolist()
    rows, _ = format_dump.formats()
    for fmt, row in zip(range(fm.LO, fm.HI), table):
        assert fm.Fmt(*row[:12]) == fm.describe(fmt), fmt
        assert (fm.Fmt(*row[:12]), tuple(row[12:])) == rows[fmt], fmt  # what the older program prints of the same headers
        cls, storage, variant = fm.storage_of(fmt)
        assert (row[14], row[15], row[17]) == (cls, storage, variant), fmt
    lo, hi = 8150, 8501
    table = program("describe", lo, hi).view(np.int32).reshape(hi - lo, 18).tolist()
    for fmt, row in zip(range(lo, hi), table):
        want = pkm.describe(fmt)
        assert pkm.Fmt(*row[:12]) == want, fmt
        assert tuple(row[12:]) == ((1, fmt, 0, 11 + int(want.filter != 0), want.matrix, 2048 << int(want.filter != 0)) if want.device else (0, -1, 0, 0, 0, 0))
    for lo, hi in ((4101, 4300), (12200, 12400), (16300, 16500), (24500, 24700), (32600, 32700), (33101, 33300), (65400, 65700), (2 ** 31 - 200, 2 ** 31 - 1)):
        table = program("describe", lo, hi).view(np.int32).reshape(hi - lo, 18).tolist()
        assert all(row == [0] * 12 + [0, -1, 0, 0, 0, 0] for row in table), (lo, hi)


REFUSAL_CASES = [
    # (fmt, y, du, dv, pixel_stride, no_src, width), the three offsets in BYTES -> message
    *[((32832, 0, 2 * du, 2 * dv, 2, 0, 200), None) for du, dv in p6.ORDERS.values()],  # each of the four orders
    *[((32913, 2, 2 * du, 2 * dv, 2, 0, 0), None) for du, dv in p6.ORDERS.values()],
    *[((32992, 6, 2 * du, 2 * dv, 2, 0, 1), None) for du, dv in p6.ORDERS.values()],
    ((32832, 0, 2, 6, 1, 0, 200), p6.LAYOUT_MSG),       # pixel_stride 1
    ((32832, 0, 2, 6, 3, 0, 200), p6.LAYOUT_MSG),       # 3, what RGB16 has
    ((32832, 0, 2, 6, 4, 0, 200), p6.LAYOUT_MSG),       # 4, the distance in bytes
    ((32832, 0, 2, 6, -2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 0, -2, 2, -2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 0, 1, 3, 2, 0, 200), p6.LAYOUT_MSG),       # YUY2's differences: (1, 3) in BYTES
    ((32832, 0, 3, 1, 2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 1, -1, 1, 2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 1, 2, 6, 2, 0, 200), p6.LAYOUT_MSG),       # an odd address, the differences right
    ((32960, 3, -2, 2, 2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 0, 3, 6, 2, 0, 200), p6.LAYOUT_MSG),       # only U odd
    ((32832, 0, 2, 7, 2, 0, 200), p6.LAYOUT_MSG),       # only V odd
    ((32832, 0, 0, 0, 2, 0, 200), p6.LAYOUT_MSG),       # equal pointers
    ((32832, 0, 2, 2, 2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 0, -2, -2, 2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 0, 2, 4, 2, 0, 200), p6.LAYOUT_MSG),       # RGB16's, P010's
    ((32832, 0, 4, 12, 2, 0, 200), p6.LAYOUT_MSG),      # the right shape at twice the distance
    ((32832, 0, -2, -6, 2, 0, 200), p6.LAYOUT_MSG),
    ((32832, 0, 6, -2, 2, 0, 200), p6.LAYOUT_MSG),
    ((32849, 0, 1000, 2000, 2, 0, 200), p6.LAYOUT_MSG),  # planar-style pointers far apart
    ((32849, 0, 1000, 2000, 100, 0, 200), p6.LAYOUT_MSG),
    ((32832, 0, 1000, 2000, 1, 1, 200), None),          # src NULL: the layout is not looked at, and there is no pitch to hold
    ((32995, 1, 0, 0, 0, 1, 0), None),
    *[((fmt, 0, 2, 6, 2, 0, 200), "Invalid Sample Format") for fmt in (32767, 32768, 32831, 32836, 32880, 33024, 32996)],
    ((32768, 0, 2, 6, 2, 1, 200), "Invalid Sample Format"),
    # the other families keep their rules and their messages
    ((8192, 0, 1, 3, 2, 0, 200), None),
    ((8192, 1, 1, 3, 2, 0, 200), None),                 # bytes sit anywhere
    ((8192, 0, 2, 6, 2, 0, 200), pkm.LAYOUT_MSG),
    ((8192, 0, 1, 3, 1, 0, 200), pkm.LAYOUT_MSG),
    ((2112, 1, 1000, 2000, 100, 0, 200), "planar YCbCr of 16-bit words wants its three planes on 2-byte boundaries"),
    ((519, 0, 1, 3, 2, 0, 200), "planar YCbCr wants the chroma planes' pitch in pixel_stride"),
    ((80, 0, 2, 6, 1, 0, 200), "P010/P016 wants pixel_stride 1 and V one sample behind U"),
    ((16, 0, 1, 3, 2, 0, 200), "NV12 wants pixel_stride 1 and V one byte behind U"),
    ((1, 1, 1, 3, 2, 0, 200), None),
]


def test_the_refusals(program):
    data = struct.pack("<I", len(REFUSAL_CASES)) + b"".join(struct.pack("<7i", *case) for case, _ in REFUSAL_CASES)
    got = program("refusals", data=data).reshape(len(REFUSAL_CASES), 96)
    for field, (case, want) in zip(got, REFUSAL_CASES):
        message = bytes(field).split(b"\0")[0].decode()
        assert message == (want or ""), (case, message)
    fmt_h = open(os.path.join(hbuild.CSRC, "hyd_sample_fmt.h")).read()
    assert fmt_h.count('"' + p6.LAYOUT_MSG + '"') == 1 and fmt_h.count('"' + pkm.LAYOUT_MSG + '"') == 1  # one new message, the old one kept
    assert "HYD_FMT_PACKED16_LAYOUT_MSG" in fmt_h
    header = " ".join(open(os.path.join(ROOT, "include", "hydrium_amd.h")).read().replace("\n *", " ").split())
    assert p6.LAYOUT_MSG in header


def test_the_origins(program):
    cases = [(fmt, du, dv, pitch, x0, y0) for fmt in (32832, 32913, 32992) for du, dv in p6.ORDERS.values() for pitch in (8192, -8192, 8199)
             for x0, y0 in ((256, 256), (2048, 0), (0, 0), (0, 768))]
    data = struct.pack("<I", len(cases)) + b"".join(struct.pack("<6i", *c) for c in cases)
    got = program("origins", data=data).view(np.int64).reshape(len(cases), 4)
    for row, (fmt, du, dv, pitch, x0, y0) in zip(got.tolist(), cases):
        # y0 rows and 2 x0 WORDS, added to ALL THREE pointers (bytes here: two a word): they still spell the word order
        assert row[:3] == [2 * (y0 * pitch + 2 * x0)] * 3, (fmt, du, dv, pitch, x0, y0, row)
        assert row[3] == list(p6.ORDERS.values()).index((du, dv))


# ---- the definition ----
def test_the_definition_under_sanitizers_stays_inside_rows_between_guard_words(program):
    """every surface a malloc that ends with the last group of its last row, rows of random words with 0x5A5A between them, top-down
    and bottom-up: the sanitizer is the bounds check, the guard words tell a read beyond a row's 4 * ceil(W / 2) words.  Random full
    words, and all-65535 where nothing may wrap"""
    cases, blob = [], []
    for w in WIDTHS:
        row = 4 * ((w + 1) // 2)
        for k, order in enumerate(p6.ORDER_NAMES):
            for filt in cm.FILTERS:
                for d in p6.DEPTHS:
                    for m in ym.MATRICES:
                        for n, (pitch, flip) in enumerate(((row, 0), (row + 5, 0), (row + 3, 1))):
                            rows = random_rows(w, HEIGHT, 99 + k) if n else np.full((HEIGHT, row), 65535, np.uint16)
                            if n == 0 and (d + m + filt) % 2:  # the packed pitch sees random words too
                                rows = random_rows(w, HEIGHT, 7 + k)
                            want = p6.expected_rgb(rows, order, w, p6.sample_fmt(m, filt, d))
                            surface = np.full(pitch * (HEIGHT - 1) + row, 0x5A5A, np.uint16)
                            for r in range(HEIGHT):
                                at = pitch * (HEIGHT - 1 - r if flip else r)
                                surface[at:at + row] = rows[r]
                            cases.append((order, filt, d, m, w, want))
                            blob.append(struct.pack("<8I", k, filt, d, m, w, HEIGHT, pitch, flip) + surface.tobytes())
    got = program("pixels", data=struct.pack("<I", len(cases)) + b"".join(blob)).view(np.uint16)
    at = 0
    for order, filt, d, m, w, want in cases:
        n = HEIGHT * w * 3
        assert np.array_equal(got[at:at + n].reshape(HEIGHT, w, 3), want), (order, cm.FILTER_NAMES[filt], d, m, w)
        at += n
    assert at == got.size
    # the guard words would have shown: a model fed the guard instead of a row's last word gives another picture
    rows = random_rows(33, HEIGHT, 99)
    other = rows.copy()
    other[:, -1] = 0x5A5A
    assert not np.array_equal(p6.expected_rgb(rows, "yuyv", 33, 32832), p6.expected_rgb(other, "yuyv", 33, 32832))


def test_the_depth_changes_the_full_range_matrices_only():
    rows = random_rows(33, HEIGHT, 11)
    for filt in cm.FILTERS:
        for m in ym.MATRICES:
            pics = [p6.expected_rgb(rows, "uyvy", 33, p6.sample_fmt(m, filt, d)) for d in p6.DEPTHS]
            same = np.array_equal(pics[0], pics[1]) and np.array_equal(pics[1], pics[2])
            assert same == bool(ym.LIMITED[m]), (filt, m)


def test_the_host_build_of_the_definition_equals_the_model(probe):
    check_definition(hook(probe.hydt_packed16_to_rgb_host))
    one, out = np.zeros((1, 4), np.uint16), np.zeros((1, 1, 3), np.uint16)
    fn = probe.hydt_packed16_to_rgb_host
    for order, filt, d, m in ((-1, 0, 1, 0), (4, 0, 1, 0), (0, 3, 1, 0), (0, -1, 1, 0), (0, 0, 0, 0), (0, 0, 4, 0), (0, 0, 1, 4), (0, 0, 1, -1)):
        assert fn(order, filt, d, m, one.ctypes.data, out.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_packed16_to_rgb_host", b"hydt_packed16_to_rgb_device"):
        assert name in probe and name not in shipped


# ---- names ----
def header_names():
    """{HYDAMD_Y21x name: value} parsed from the public header's enum: STEM(P, F, D) names P_BT709 = 32768 + 16 F + 64 D and the
    three that follow it"""
    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    rule = re.search(r"#define HYDAMD_PACKED16_STEM\(P, F, D\) \\\n\s*HYDAMD_##P##_BT709 = (\d+) \+ 16 \* \(F\) \+ 64 \* \(D\), HYDAMD_##P##_BT709_FULL, "
                     r"HYDAMD_##P##_BT601, HYDAMD_##P##_BT601_FULL\n", text)
    assert rule and int(rule.group(1)) == 32768
    body = re.search(r"\nenum \{\n(.*?)\n\};\n#undef HYDAMD_PACKED16_STEM\n", text, re.S).group(1)
    found = {}
    for stem, f, d in re.findall(r"HYDAMD_PACKED16_STEM\((\w+), (\d), (\d)\)", body):
        for m, name in enumerate(fm.MATRIX_NAMES):
            assert f"HYDAMD_{stem}_{name}" not in found
            found[f"HYDAMD_{stem}_{name}"] = 32768 + 16 * int(f) + 64 * int(d) + m
    assert re.sub(r"HYDAMD_PACKED16_STEM\(\w+, \d, \d\)", "", body).replace(",", "").split() == []  # nothing else in the enum
    return found, text


def test_the_headers_names_are_the_python_layers():
    from hydrium_amd import device

    found, text = header_names()
    want = {"HYDAMD_" + p6.public_name(fmt): fmt for fmt in p6.FAMILY}
    assert found == want and len(want) == 36
    for name, fmt in want.items():
        assert getattr(device, name[len("HYDAMD_"):]) == fmt
        assert device.ycbcr_fields(fmt) == (32768, p6.matrix_of(fmt), 0, p6.filter_of(fmt), p6.depth_of(fmt))
    assert sorted(device.PACKED16_FAMILY) == sorted(p6.FAMILY)
    assert (device.Y210_BT709, device.Y210L_BT601, device.Y212C_BT709_FULL, device.Y216_BT709, device.Y216L_BT601_FULL) == (32832, 32866, 32913, 32960, 32995)
    older = set(device.NV12_FAMILY) | set(device.P016_FAMILY) | set(device.PLANAR_FAMILY) | set(device.PLANAR16_FAMILY) | set(device.PACKED_FAMILY)
    assert not set(device.PACKED16_FAMILY) & older and len(older) == 172
    assert "Y21" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    # none of them is a numbered #define: the header's count of those is what it was
    assert not re.findall(r"^#define HYDAMD_Y21\w* +-?\d+\s*$", text, re.M)
    assert len(re.findall(r"^#define HYDAMD_\w+ +-?\d+\s*$", text, re.M)) == 176
    # the older names keep their numbers
    assert (device.NV12_BT709, device.P016L_BT601_FULL, device.I420_BT709, device.I422L_BT601_FULL, device.I010_BT709, device.I416_BT601_FULL,
            device.YUY2_BT709, device.YUY2L_BT601_FULL) == (16, 243, 512, 551, 2112, 2251, 8192, 8227)
    for fmt in pkm.FAMILY:
        assert device.ycbcr_fields(fmt) == (8192, pkm.matrix_of(fmt), 0, pkm.filter_of(fmt), 0)


def test_the_remarks_that_left_the_depth_bits_of_8192_free_are_gone():
    for path in (os.path.join(hbuild.CSRC, "hyd_sample_fmt.h"), os.path.join(ROOT, "include", "hydrium_amd.h"), os.path.join(ROOT, "DESIGN.md")):
        text = " ".join(open(path).read().split())
        assert "left free for Y210" not in text and "reserved for them" not in text, path
        assert "32768" in text, path


def test_packed_yuv16_names_its_format_and_fills_a_descriptor():
    import torch
    from hydrium_amd import device

    for w, h in ((1, 5), (8, 8), (33, 9), (200, 120)):
        row = 4 * ((w + 1) // 2)
        for fmt in p6.FAMILY:
            for order, (du, dv) in p6.ORDERS.items():
                buf = torch.zeros(h * (row + 6), dtype=torch.int16)
                surface = buf.as_strided((h, row), (row + 6, 1))
                pic = device.PackedYuv16(surface, w, 16 + p6.matrix_of(fmt), order, cm.FILTER_NAMES[p6.filter_of(fmt)], p6.bits_of(fmt))
                assert isinstance(pic, device.PackedYuv) and isinstance(pic, device.Nv12)
                assert device.sample_fmt_of(pic) == fmt == pic.sample_fmt and pic.shape == (h, w, 3)
                assert (pic.pitch, pic.pixel_stride) == (row + 6, 2)  # in words
                y = buf.data_ptr() + 2 * p6.y_offset(order)
                assert pic.pointers() == [y, y + 2 * du, y + 2 * dv] and min(pic.pointers()) == buf.data_ptr()
                assert device.PackedYuv16(surface, w, fmt, order).sample_fmt == fmt  # the number itself for the matrix
                assert device.PackedYuv16(surface, w, fmt, order, depth=p6.bits_of(fmt)).sample_fmt == fmt
                descs, fmts = device.mixed_descriptors([pic])
                d = descs[0]
                assert fmts == [fmt] and (d.row_stride, d.pixel_stride, d.width, d.height) == (row + 6, 2, w, h)
                assert [d.src[0], d.src[1], d.src[2]] == pic.pointers()
    surface = torch.zeros((120, 400), dtype=torch.uint16)
    pic = device.PackedYuv16(surface, 200)
    assert device.sample_fmt_of(pic) == device.Y210_BT709 == 32832 and pic.order == "yuyv"  # the defaults: Y210, nearest, BT.709
    assert device.PackedYuv16(surface, 200, depth=16).sample_fmt == device.Y216_BT709
    assert device.PackedYuv16(surface, 200, device.NV12_BT601, chroma="left", depth=12).sample_fmt == device.Y212L_BT601 == 32930
    assert device.PackedYuv16(surface, 199).width == 199 and device.PackedYuv16(surface, 57).pitch == 400  # a wider surface
    assert device.PackedYuv16(surface, 200, order="Y210").pointers() == pic.pointers()
    rgb16 = torch.zeros((120, 200, 3), dtype=torch.int16)
    yuy2 = device.PackedYuv(torch.zeros((120, 400), dtype=torch.uint8), 200)
    assert device.mixed_descriptors([pic, rgb16, yuy2], sample_fmts="each")[1] == [32832, 1, 8192]


def test_packed_yuv16_refuses_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    surface = torch.zeros((10, 36), dtype=torch.int16)
    assert device.PackedYuv16(surface, 18).pixel_stride == 2 and device.PackedYuv16(surface, 17).width == 17
    with pytest.raises(ValueError, match="4 \\* ceil"):  # a row too short for the width
        device.PackedYuv16(surface, 19)
    with pytest.raises(ValueError, match="4 \\* ceil"):
        device.PackedYuv16(surface, 0)
    with pytest.raises(ValueError, match="unit element stride"):
        device.PackedYuv16(torch.zeros((10, 72), dtype=torch.int16)[:, ::2], 18)
    for other in (torch.uint8, torch.float16, torch.bfloat16, torch.int32, torch.float32):
        with pytest.raises(ValueError, match="2-byte integer"):
            device.PackedYuv16(torch.zeros((10, 36), dtype=other), 18)
    with pytest.raises(ValueError, match="2-byte integer"):
        device.PackedYuv16(torch.zeros((10, 18, 2), dtype=torch.int16), 18)
    with pytest.raises(ValueError, match="order"):
        device.PackedYuv16(surface, 18, order="yyuv")
    with pytest.raises(ValueError, match="order"):
        device.PackedYuv16(surface, 18, order="yuy2")  # the 8-bit format's name
    with pytest.raises(ValueError):
        device.PackedYuv16(surface, 18, chroma="bilinear")
    with pytest.raises(ValueError, match="depth"):
        device.PackedYuv16(surface, 18, depth=8)
    with pytest.raises(ValueError, match="another chroma filter"):
        device.PackedYuv16(surface, 18, device.Y210C_BT709, chroma="left")
    with pytest.raises(ValueError, match="another depth"):
        device.PackedYuv16(surface, 18, device.Y210_BT709, depth=16)
    for bad in (0, 1, 32, 80, 512, 2112, 8192, 32768, 32836, 32880, 33024):  # one of the four matrices, or one of the 36 numbers
        with pytest.raises(ValueError):
            device.PackedYuv16(surface, 18, bad)
    with pytest.raises(TypeError):
        device.PackedYuv16.from_surface(surface, 18, 10, 36, 0)
    with pytest.raises(ValueError, match="8-bit"):  # and the 8-bit class keeps to bytes
        device.PackedYuv(surface, 18)


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((24, 16), np.uint16)
    for fmt in p6.FAMILY:
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 2, p + 6], 0, 0, 16, 2, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_six_new_instances_have_symbols_of_their_own_and_keep_the_transform_kernels_contract():
    """k_transform_tokenize_y216<mode, HYDK_STORE_Y216 | _Y216I>: none under an older symbol name, no scratch, and the co-residency
    line every family is held to (26 granules of 1280 bytes of static LDS, 128 registers)"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_y216" in k}
    assert sorted(re.match(r"_Z25k_transform_tokenize_y216ILi(\d)ELi(\d+)EE", k).groups() for k in new) == \
        [(mode, store) for mode in "012" for store in ("13", "14")], sorted(res)
    older = ("k_transform_tokenize_planar", "k_transform_tokenize_p016", "k_transform_tokenize_yuvp16", "k_transform_tokenize_yuy2", "_Z20k_transform_tokenizeI")
    assert not any(o in k for k in new for o in older)
    count = lambda stem: sum(stem in k for k in res)
    assert (count("k_transform_tokenize_planar"), count("k_transform_tokenize_p016"), count("k_transform_tokenize_yuvp16"), count("k_transform_tokenize_yuy2"),
            count("_Z20k_transform_tokenizeI")) == (6, 6, 6, 6, 19)
    for name, d in sorted(new.items()):
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 26 * 1280 and d["next_free_vgpr"] <= 128, (name, d)
