"""CPU-only: the packed 4:2:2 YCbCr formats (HYDAMD_YUY2_*, HYDAMD_YUY2C_*, HYDAMD_YUY2L_*: YUYV, UYVY, YVYU and VYUY by the
pointers) where no device is needed — the descriptor, the refusals and the origins of csrc/hyd_sample_fmt.h and the round trip of
csrc/hip/hydk_store.h against a model written from the prose; the per-pixel definition (csrc/hip/hydk_yuy2.h) as plain C++ under
address and UB sanitizers, and as the probe library's host build, against packed_model.py; device.PackedYuv's reading of its
surface; the drop-in API's refusal; the header's constants; and what the six new instances of the transform kernel ask of a
compute unit.  Every test here fails on the parent, where 8192 is "Invalid Sample Format"."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import chroma_model as cm
import format_dump
import packed_model as pkm
import planar_model as plm
import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 7, 8, 9, 33)
HEIGHT = 3
LO, HI = 8150, 8501


def random_rows(w, h, seed=8192):
    """h rows of 4 * ceil(w / 2) random bytes"""
    return np.random.default_rng(seed + 100 * w + h).integers(0, 256, (h, 4 * ((w + 1) // 2)), dtype=np.uint8)


def check_definition(to_rgb, widths=WIDTHS, height=HEIGHT):
    """to_rgb(order index, filter, matrix, rows, w, h) -> (h, w, 3) uint8, held to the model over every byte order x filter x matrix
    on random rows and on all-255 (the top of the range: nothing may wrap).  Shared with the on-device test."""
    for w in widths:
        for k, order in enumerate(pkm.ORDER_NAMES):
            for filt in cm.FILTERS:
                for m in ym.MATRICES:
                    for rows in (random_rows(w, height, 8192 + k), np.full((height, 4 * ((w + 1) // 2)), 255, np.uint8)):
                        got, want = to_rgb(k, filt, m, rows, w, height), pkm.expected_rgb(rows, order, w, m, filt)
                        assert got.dtype == np.uint8 and got.shape == want.shape == (height, w, 3)
                        wrong = np.argwhere(got != want)
                        assert wrong.size == 0, (order, cm.FILTER_NAMES[filt], m, w, [(tuple(p), int(got[tuple(p)]), int(want[tuple(p)])) for p in wrong[:8]])


def hook(fn, *device):
    """a probe-flavour packed entry as to_rgb(order, filter, matrix, rows, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def to_rgb(order, filt, m, rows, w, h):
        rows = np.ascontiguousarray(rows)
        out = np.full((h, w, 3), 0xA5, np.uint8)
        assert fn(*device, order, filt, m, rows.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return to_rgb


@pytest.fixture(scope="module")
def program():
    """tests/c/packed_formats.cc: hyd_sample_fmt.h, hydk_store.h and hydk_yuy2.h with g++ under address and UB sanitizers, no HIP
    header, no warning"""
    return format_dump.sanitized_program("packed_formats")


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


# ---- the model ----
def test_the_model_takes_apart_what_it_put_together_and_the_orders_are_the_headers():
    assert pkm.ORDERS == {"yuyv": (1, 3), "yvyu": (3, 1), "uyvy": (-1, 1), "vyuy": (1, -1)}
    rng = np.random.default_rng(1)
    for w in WIDTHS:
        cw = (w + 1) // 2
        planes = tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((HEIGHT, w), (HEIGHT, cw), (HEIGHT, cw)))
        seen = set()
        for order in pkm.ORDER_NAMES:
            rows = pkm.interleave(planes, order, w)
            assert rows.shape == (HEIGHT, 4 * cw)
            assert all(np.array_equal(a, b) for a, b in zip(pkm.deinterleave(rows, order, w), planes))
            seen.add(rows.tobytes())
        assert len(seen) == 4
    # YUYV as everybody writes it: Y0 U Y1 V
    rows = pkm.interleave((np.array([[1, 2]], np.uint8), np.array([[3]], np.uint8), np.array([[4]], np.uint8)), "yuyv", 2)
    assert rows.tolist() == [[1, 3, 2, 4]]
    assert pkm.interleave((np.array([[1, 2]], np.uint8), np.array([[3]], np.uint8), np.array([[4]], np.uint8)), "uyvy", 2).tolist() == [[3, 1, 4, 2]]


# ---- the descriptor ----
def test_the_descriptor_of_every_number_from_8150_to_8500(program):
    table = program("describe", LO, HI).view(np.int32).reshape(HI - LO, 18).tolist()
    formats = []
    for fmt, row in zip(range(LO, HI), table):
        got, job = pkm.Fmt(*row[:12]), tuple(row[12:])
        want = pkm.describe(fmt)
        assert got == want, (fmt, got, want)
        if want.device:
            formats.append(fmt)
            assert (got.bytes, got.bits, got.sub, got.sx, got.sy, got.device, got.host, got.layout) == (1, 8, 1, 1, 0, 1, 0, 3)
            # 8-bit class, storage form 11 (nearest) or 12 (interpolated), variant bits 2048 and 4096; and the number comes back
            interp = int(got.filter != 0)
            assert job == (1, fmt, 0, 11 + interp, got.matrix, 2048 << interp), (fmt, job)
        else:
            assert job == (0, -1, 0, 0, 0, 0), (fmt, job)
    assert formats == list(range(8192, 8196)) + list(range(8208, 8212)) + list(range(8224, 8228)) == sorted(pkm.FAMILY) and len(formats) == 12
    by_number = dict(zip(range(LO, HI), table))
    for fmt in list(range(8196, 8208)) + [8212, 8223, 8228, 8239]:  # the subsampling bits are set
        assert by_number[fmt][:12] == [0] * 12, fmt
    for fmt in (8240, 8243, 8255, 8256, 8259, 8320, 8384, 8500, 8191, 8150):  # filter 3, then depth; and below the base
        assert by_number[fmt][:12] == [0] * 12, fmt


REFUSAL_CASES = [
    # (fmt, du, dv, pixel_stride, no_src, width) -> message
    *[((8192, du, dv, 2, 0, 200), None) for du, dv in pkm.ORDERS.values()],
    *[((8211, du, dv, 2, 0, 0), None) for du, dv in pkm.ORDERS.values()],
    *[((8224, du, dv, 2, 0, 1), None) for du, dv in pkm.ORDERS.values()],
    ((8192, 1, 3, 1, 0, 200), pkm.LAYOUT_MSG),      # pixel_stride 1
    ((8192, 1, 3, 4, 0, 200), pkm.LAYOUT_MSG),      # and 4
    ((8192, 1, 3, 3, 0, 200), pkm.LAYOUT_MSG),      # what RGB8 has
    ((8192, -1, 1, -2, 0, 200), pkm.LAYOUT_MSG),
    ((8192, 1, -1, 0, 0, 200), pkm.LAYOUT_MSG),
    ((8192, -1, -3, 2, 0, 200), pkm.LAYOUT_MSG),    # V two bytes from U on the wrong side
    ((8192, 3, 5, 2, 0, 200), pkm.LAYOUT_MSG),
    ((8192, -1, -1, 2, 0, 200), pkm.LAYOUT_MSG),    # src[1] == src[2]
    ((8192, 1, 1, 2, 0, 200), pkm.LAYOUT_MSG),
    ((8192, 0, 0, 2, 0, 200), pkm.LAYOUT_MSG),      # a grey picture's three equal pointers
    ((8192, 1, 2, 2, 0, 200), pkm.LAYOUT_MSG),      # RGB8's
    ((8192, 3, -1, 2, 0, 200), pkm.LAYOUT_MSG),
    ((8192, -1, 3, 2, 0, 200), pkm.LAYOUT_MSG),
    ((8192, -3, -1, 2, 0, 200), pkm.LAYOUT_MSG),
    ((8209, 1000, 2000, 2, 0, 200), pkm.LAYOUT_MSG),  # planar-style pointers far apart
    ((8209, 1000, 2000, 100, 0, 200), pkm.LAYOUT_MSG),
    ((8226, 2, 3, 1, 0, 200), pkm.LAYOUT_MSG),      # NV12's
    ((8192, 1000, 2000, 1, 1, 200), None),          # src NULL: the layout is not looked at, and there is no pitch to hold
    ((8227, 0, 0, 0, 1, 0), None),
    ((8191, 1, 3, 2, 0, 200), "Invalid Sample Format"),
    ((8196, 1, 3, 2, 0, 200), "Invalid Sample Format"),
    ((8240, 1, 3, 2, 0, 200), "Invalid Sample Format"),
    ((8256, 1, 3, 2, 1, 200), "Invalid Sample Format"),
    ((12288, 1, 3, 2, 0, 200), "Invalid Sample Format"),
    # the other families keep their rules
    ((519, 1, 3, 2, 0, 200), "planar YCbCr wants the chroma planes' pitch in pixel_stride"),
    ((16, 1, 3, 2, 0, 200), "NV12 wants pixel_stride 1 and V one byte behind U"),
    ((0, 1, 3, 2, 0, 200), None),
]


def test_the_refusals(program):
    data = struct.pack("<I", len(REFUSAL_CASES)) + b"".join(struct.pack("<6i", *case) for case, _ in REFUSAL_CASES)
    got = program("refusals", data=data).reshape(len(REFUSAL_CASES), 96)
    for field, (case, want) in zip(got, REFUSAL_CASES):
        message = bytes(field).split(b"\0")[0].decode()
        assert message == (want or ""), (case, message)
    fmt_h = open(os.path.join(hbuild.CSRC, "hyd_sample_fmt.h")).read()
    assert fmt_h.count('"' + pkm.LAYOUT_MSG + '"') == 1
    assert pkm.LAYOUT_MSG in open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()


def test_the_origins(program):
    cases = [(fmt, du, dv, pitch, x0, y0) for fmt in (8192, 8211, 8224) for du, dv in pkm.ORDERS.values() for pitch in (8192, -8192, 8199)
             for x0, y0 in ((256, 256), (2048, 0), (0, 0), (0, 768))]
    data = struct.pack("<I", len(cases)) + b"".join(struct.pack("<6i", *c) for c in cases)
    got = program("origins", data=data).view(np.int64).reshape(len(cases), 4)
    for row, (fmt, du, dv, pitch, x0, y0) in zip(got.tolist(), cases):
        # y0 rows and 2 x0 bytes, added to ALL THREE pointers: they still spell the byte order
        assert row[:3] == [y0 * pitch + 2 * x0] * 3, (fmt, du, dv, pitch, x0, y0, row)
        assert row[3] == list(pkm.ORDERS.values()).index((du, dv))


# ---- the definition ----
def test_the_definition_under_sanitizers_stays_inside_rows_between_guard_bytes(program):
    """every surface a malloc that ends with the last group of its last row, rows of random bytes with 0x5A between them,
    top-down and bottom-up: the sanitizer is the bounds check, the guard bytes tell a read beyond a row's 4 * ceil(W / 2) bytes"""
    cases, blob = [], []
    for w in WIDTHS:
        row = 4 * ((w + 1) // 2)
        for k, order in enumerate(pkm.ORDER_NAMES):
            for filt in cm.FILTERS:
                for m in ym.MATRICES:
                    for pitch, flip in ((row, 0), (row + 5, 0), (row + 3, 1)):
                        rows = random_rows(w, HEIGHT, 99 + k)
                        want = pkm.expected_rgb(rows, order, w, m, filt)
                        surface = np.full(pitch * (HEIGHT - 1) + row, 0x5A, np.uint8)
                        for r in range(HEIGHT):
                            at = pitch * (HEIGHT - 1 - r if flip else r)
                            surface[at:at + row] = rows[r]
                        cases.append((order, filt, m, w, want))
                        blob.append(struct.pack("<7I", k, filt, m, w, HEIGHT, pitch, flip) + surface.tobytes())
    got = program("pixels", data=struct.pack("<I", len(cases)) + b"".join(blob))
    at = 0
    for order, filt, m, w, want in cases:
        n = HEIGHT * w * 3
        assert np.array_equal(got[at:at + n].reshape(HEIGHT, w, 3), want), (order, cm.FILTER_NAMES[filt], m, w)
        at += n
    assert at == got.size
    # the guard bytes would have shown: a model fed the guard instead of a row's last byte gives another picture
    rows = random_rows(33, HEIGHT, 99)
    other = rows.copy()
    other[:, -1] = 0x5A
    assert not np.array_equal(pkm.expected_rgb(rows, "yuyv", 33, 0, cm.NEAREST), pkm.expected_rgb(other, "yuyv", 33, 0, cm.NEAREST))


def test_the_picture_is_the_i422_picture_of_the_same_planes():
    for w in WIDTHS:
        rows = random_rows(w, HEIGHT, 5)
        for order in pkm.ORDER_NAMES:
            planes = pkm.deinterleave(rows, order, w)
            for fmt in pkm.FAMILY:
                i422 = pkm.as_i422(fmt)
                assert plm.is_format(i422) and plm.sub_of(i422) == plm.S422
                assert np.array_equal(pkm.expected_rgb(rows, order, w, pkm.matrix_of(fmt), pkm.filter_of(fmt)),
                                      plm.expected_rgb(planes, plm.matrix_of(i422), plm.S422, plm.filter_of(i422)))


def test_the_host_build_of_the_definition_equals_the_model(probe):
    check_definition(hook(probe.hydt_packed_to_rgb_host))
    one, out = np.zeros((1, 4), np.uint8), np.zeros((1, 1, 3), np.uint8)
    fn = probe.hydt_packed_to_rgb_host
    for order, filt, m in ((-1, 0, 0), (4, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 4), (0, 0, -1)):
        assert fn(order, filt, m, one.ctypes.data, out.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_packed_to_rgb_host", b"hydt_packed_to_rgb_device"):
        assert name in probe and name not in shipped


# ---- names ----
def test_the_headers_constants_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define (HYDAMD_YUY2[CL]?_\w+) (\d+)\s*$", text, re.M)}
    want = {}
    for filt in cm.FILTERS:
        for m, name in enumerate(("BT709", "BT709_FULL", "BT601", "BT601_FULL")):
            stem = f"YUY2{('', 'C', 'L')[filt]}_{name}"
            assert getattr(device, stem) == pkm.sample_fmt(m, filt)
            want["HYDAMD_" + stem] = pkm.sample_fmt(m, filt)
    assert found == want and len(want) == 12
    assert sorted(device.PACKED_FAMILY) == sorted(pkm.FAMILY) == sorted(want.values())
    assert device.YUY2_BT709 == 8192 and device.YUY2C_BT601_FULL == 8211 and device.YUY2L_BT601_FULL == 8227
    assert not set(device.PACKED_FAMILY) & (set(device.NV12_FAMILY) | set(device.P016_FAMILY) | set(device.PLANAR_FAMILY) | set(device.PLANAR16_FAMILY))
    assert "YUY2" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    for fmt in pkm.FAMILY:
        assert device.ycbcr_fields(fmt) == (8192, pkm.matrix_of(fmt), 0, pkm.filter_of(fmt), 0)
    # the header's numbered constants of before are all still there (164 of them, 160 YCbCr names among them), and twelve more
    assert len(re.findall(r"^#define HYDAMD_\w+ +-?\d+\s*$", text, re.M)) == 164 + 12
    assert (device.NV12_BT709, device.P016L_BT601_FULL, device.I420_BT709, device.I422L_BT601_FULL, device.I010_BT709, device.I416_BT601_FULL) == \
        (16, 243, 512, 551, 2112, 2251)


def test_packed_yuv_names_its_format_and_fills_a_descriptor():
    import torch
    from hydrium_amd import device

    for w, h in ((1, 5), (8, 8), (33, 9), (200, 120)):
        row = 4 * ((w + 1) // 2)
        for fmt in pkm.FAMILY:
            for order, (du, dv) in pkm.ORDERS.items():
                buf = torch.zeros(h * (row + 6), dtype=torch.uint8)
                surface = buf.as_strided((h, row), (row + 6, 1))
                pic = device.PackedYuv(surface, w, 16 + pkm.matrix_of(fmt), order, cm.FILTER_NAMES[pkm.filter_of(fmt)])
                assert isinstance(pic, device.Nv12) and device.sample_fmt_of(pic) == fmt == pic.sample_fmt and pic.shape == (h, w, 3)
                assert (pic.pitch, pic.pixel_stride) == (row + 6, 2)
                y = buf.data_ptr() + pkm.y_offset(order)
                assert pic.pointers() == [y, y + du, y + dv] and min(pic.pointers()) == buf.data_ptr()
                assert device.PackedYuv(surface, w, fmt, order).sample_fmt == fmt  # the number itself for the matrix
                descs, fmts = device.mixed_descriptors([pic])
                d = descs[0]
                assert fmts == [fmt] and (d.row_stride, d.pixel_stride, d.width, d.height) == (row + 6, 2, w, h)
                assert [d.src[0], d.src[1], d.src[2]] == pic.pointers()
    surface = torch.zeros((120, 400), dtype=torch.uint8)
    pic = device.PackedYuv(surface, 200)
    assert device.sample_fmt_of(pic) == device.YUY2_BT709 == 8192 and pic.order == "yuyv"  # the defaults
    assert device.PackedYuv(surface, 199).width == 199 and device.PackedYuv(surface, 57).pitch == 400  # a wider surface
    assert device.PackedYuv(surface, 200, order="YUY2").pointers() == pic.pointers()
    rgb8 = torch.zeros((120, 200, 3), dtype=torch.uint8)
    assert device.mixed_descriptors([pic, rgb8], sample_fmts="each")[1] == [8192, 0]


def test_packed_yuv_refuses_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    surface = torch.zeros((10, 36), dtype=torch.uint8)
    assert device.PackedYuv(surface, 18).pixel_stride == 2 and device.PackedYuv(surface, 17).width == 17
    with pytest.raises(ValueError, match="4 \\* ceil"):  # a row too short for the width
        device.PackedYuv(surface, 19)
    with pytest.raises(ValueError, match="4 \\* ceil"):
        device.PackedYuv(surface, 0)
    with pytest.raises(ValueError, match="unit element stride"):
        device.PackedYuv(torch.zeros((10, 72), dtype=torch.uint8)[:, ::2], 18)
    with pytest.raises(ValueError, match="8-bit"):
        device.PackedYuv(surface.to(torch.int16), 18)
    with pytest.raises(ValueError, match="8-bit"):
        device.PackedYuv(torch.zeros((10, 18, 2), dtype=torch.uint8), 18)
    with pytest.raises(ValueError, match="order"):
        device.PackedYuv(surface, 18, order="yyuv")
    with pytest.raises(ValueError):
        device.PackedYuv(surface, 18, chroma="bilinear")
    with pytest.raises(ValueError, match="another chroma filter"):
        device.PackedYuv(surface, 18, device.YUY2C_BT709, chroma="left")
    for bad in (0, 32, 80, 512, 2112, 8196, 8240):  # the matrix is one of the four, or one of the twelve numbers
        with pytest.raises(ValueError):
            device.PackedYuv(surface, 18, bad)
    with pytest.raises(TypeError):
        device.PackedYuv.from_surface(surface, 18, 10, 36, 0)


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((24, 16), np.uint8)
    for fmt in pkm.FAMILY:
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 1, p + 3], 0, 0, 16, 2, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_six_new_instances_have_symbols_of_their_own_and_keep_the_transform_kernels_contract():
    """k_transform_tokenize_yuy2<mode, HYDK_STORE_YUY2 | _YUY2I>: none under an older symbol name, no scratch, and the co-residency
    line the planar instances are held to (26 granules of 1280 bytes of static LDS, 128 registers)"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_yuy2" in k}
    assert sorted(re.match(r"_Z25k_transform_tokenize_yuy2ILi(\d)ELi(\d+)EE", k).groups() for k in new) == \
        [(mode, store) for mode in "012" for store in ("11", "12")], sorted(res)
    older = ("k_transform_tokenize_planar", "k_transform_tokenize_p016", "k_transform_tokenize_yuvp16", "_Z20k_transform_tokenizeI")
    assert not any(o in k for k in new for o in older)
    count = lambda stem: sum(stem in k for k in res)
    assert (count("k_transform_tokenize_planar"), count("k_transform_tokenize_p016"), count("k_transform_tokenize_yuvp16")) == (6, 6, 6)
    for name, d in sorted(new.items()):
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 26 * 1280 and d["next_free_vgpr"] <= 128, (name, d)
