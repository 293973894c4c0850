"""CPU-only: the planar YCbCr formats (HYDAMD_I420_*, HYDAMD_I422_*, HYDAMD_I444_* and their C / L forms) where no device is
needed — the numpy model's 4:2:2 taps against the 4:2:0 taps on doubled rows (far row = near row); the per-pixel definition
as the host compiler built it (csrc/hip/hydk_chroma.h, through the probe library, and as plain C++ under address and UB
sanitizers) against the model; the predicates, origins and the pitch helper of csrc/hyd_sample_fmt.h; device.PlanarYuv's
reading of its planes; the drop-in API's refusal; the header's constants; and what the six new instances of the transform
kernel ask of a compute unit."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import chroma_model as cm
import format_dump
import format_model as fm
import planar_model as plm
import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK_SIZES = [(1, 1), (2, 1), (3, 2), (33, 9), (200, 120)]


def random_plane(sub, w, h, seed=512):
    return np.random.default_rng(seed + 1000 * w + 10 * h + sub).integers(0, 256, plm.chroma_shape(sub, w, h), dtype=np.uint8)


def check_upsample(upsample):
    """upsample(sub, filter, plane, w, h) -> (h, w) uint8, held to the model on random planes and on all-255 (the top of the
    range: nothing may wrap).  Shared with the on-device test."""
    for w, h in HOOK_SIZES:
        for sub, filt in plm.FORMS:
            for plane in (random_plane(sub, w, h), np.full(plm.chroma_shape(sub, w, h), 255, np.uint8)):
                got, want = upsample(sub, filt, plane, w, h), plm.upsample(sub, filt, plane, w, h)
                assert got.dtype == np.uint8 and got.shape == want.shape == (h, w)
                wrong = np.argwhere(got != want)
                assert wrong.size == 0, (plm.SUB_NAMES[sub], cm.FILTER_NAMES[filt], w, h, [(tuple(p), int(got[tuple(p)]), int(want[tuple(p)])) for p in wrong[:8]])
                if plane.min() == 255:
                    assert (got == 255).all()


def hook(fn, *device):
    """a probe-flavour planar upsampling entry as upsample(sub, filter, plane, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def upsample(sub, filt, plane, w, h):
        plane = np.ascontiguousarray(plane)
        out = np.full((h, w), 0xA5, np.uint8)
        assert fn(*device, sub, filt, plane.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return upsample


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


# ---- the definition ----
def test_the_422_taps_are_the_420_taps_on_doubled_rows_and_i420_is_nv12s_upsampling():
    """the far = near identity: (12a + 4b + 8) >> 4 = (3a + b + 2) >> 2, (4a + 2) >> 2 = a, (4a + 4b + 4) >> 3 = (a + b + 1) >> 1.
    The only test of this module that holds on the parent: it checks the model alone."""
    for w in (1, 2, 3, 33):
        for h in (1, 2, 9):
            for kind in ("random", "255"):
                planes = [random_plane(plm.S422, w, h, seed) if kind == "random" else np.full(plm.chroma_shape(plm.S422, w, h), 255, np.uint8) for seed in (1, 2)]
                for filt in cm.FILTERS:
                    # 4:2:2 of a w x h picture = 4:2:0 of a w x 2h picture whose chroma rows are these: picture row 2r and 2r + 1
                    # of the tall one read chroma row r as near, and r - 1 or r + 1 as far — unless every row is doubled
                    doubled = np.stack([np.repeat(p, 2, 0) for p in planes], -1)  # (2h, cw, 2): rows r, r, r + 1, r + 1, ...
                    tall = cm.upsample(filt, doubled, w, 4 * h)  # 4h picture rows over 2h chroma rows
                    # picture rows 4r + 1 and 4r + 2 of the tall picture have near and far both copies of row r
                    for c in (0, 1):
                        got = plm.upsample(plm.S422, filt, planes[c], w, h)
                        assert np.array_equal(got, tall[1::4, :, c]) and np.array_equal(got, tall[2::4, :, c]), (w, h, kind, filt)
                # I420 of the model is chroma_model's upsampling of the interleaved pair
                u, v = (random_plane(plm.S420, w, h, seed) if kind == "random" else np.full(plm.chroma_shape(plm.S420, w, h), 255, np.uint8) for seed in (3, 4))
                for filt in cm.FILTERS:
                    both = cm.upsample(filt, np.stack([u, v], -1), w, h)
                    assert np.array_equal(plm.upsample(plm.S420, filt, u, w, h), both[..., 0])
                    assert np.array_equal(plm.upsample(plm.S420, filt, v, w, h), both[..., 1])
                # 4:4:4 is the plane
                p = random_plane(plm.S444, w, h)
                assert np.array_equal(plm.upsample(plm.S444, cm.NEAREST, p, w, h), p)


def test_the_host_build_of_the_definition_equals_the_model(probe):
    check_upsample(hook(probe.hydt_planar_upsample_host))
    one = np.zeros((1, 1), np.uint8)
    fn = probe.hydt_planar_upsample_host
    for sub, filt in ((-1, 0), (3, 0), (0, 3), (0, -1), (2, 1), (2, 2)):  # no subsampling, no filter, and 4:4:4 has none
        assert fn(sub, filt, one.ctypes.data, one.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_planar_upsample_host", b"hydt_planar_upsample_device"):
        assert name in probe and name not in shipped


# ---- the headers as plain C++ under address and UB sanitizers ----
@pytest.fixture(scope="module")
def planar_program():
    """tests/c/planar_formats.cc: hyd_sample_fmt.h and hydk_chroma.h with g++, no HIP header, no warning"""
    return format_dump.sanitized_program("planar_formats")


def test_the_predicates_origins_and_the_pitch_helper(planar_program):
    lo, hi = -8, 1101
    got = planar_program("geometry")
    origins = got[:3 * 2 * 3 * 8].view(np.int64).reshape(3, 2, 3)
    pitches = got[3 * 2 * 3 * 8:].view(np.int32).reshape(2, 3, 3, 2)
    # (a) every predicate for -8 ... 1100, read off the descriptor the C side gives each number (format_dump: held to
    # format_model.describe on all of -8 ... 4100 by tests/test_host_sanitizers.py)
    family = []
    for fmt in range(lo, hi):
        d = format_dump.described(fmt)
        assert d == fm.describe(fmt), (fmt, d)
        planar = d.layout == fm.PLANES and d.depth == 0
        want = plm.predicate_row(fmt)
        row = (int(planar), d.sub if planar else 0, d.filter if planar else 0, d.matrix if planar else 0, int(planar and d.filter != 0),
               d.bytes, d.device, d.host)
        assert row == want, (fmt, row, want)
        if want[0]:
            family.append(fmt)
            assert (d.sx, d.sy) == plm.shifts(d.sub) and (d.is_float, d.bits) == (0, 8), (fmt, d)  # not the float class, no (U, V) pairs
        assert d.is_float == int(2 <= fmt <= 4)
    assert tuple(family) == tuple(sorted(plm.FAMILY)) == tuple(sorted(fm.PLANAR_FAMILY)) and len(family) == 28
    assert family == list(range(512, 524)) + list(range(528, 536)) + list(range(544, 552))
    for fmt in (524, 527, 536, 543, 552, 559, 560, 575, 576, 640, 1024, 1100, 511, 264):
        assert format_dump.described(fmt) == fm.NOTHING, fmt
    # the numbers earlier families pin stay what they were
    for fmt in (5, 7, 15, 20, 31, 36, 47, 52, 64, 79, 84, 128, 244):
        d = format_dump.described(fmt)
        assert (d.bytes, d.device, d.host) == (0, 0, 0), fmt
    assert [format_dump.described(f).device for f in (0, 1, 2, 3, 4, 16, 35, 51, 80, 243)] == [1] * 10
    # (b) origins at (256, 512), Y pitch 1024, chroma pitch 520 and -520: I420C, I422L, I444
    for k, (sx, sy) in enumerate(((1, 1), (1, 0), (0, 0))):
        for j, cp in enumerate((520, -520)):
            chroma = (512 >> sy) * cp + (256 >> sx)
            assert origins[k, j].tolist() == [512 * 1024 + 256, chroma, chroma], (k, j)
    # (c) the pitch rule at |pitch| = cw - 1, cw, cw + 1, both signs, W = 199 and 200
    assert pitches.tolist() == [[[[0, 0], [1, 1], [1, 1]]] * 3] * 2


def test_the_definition_stays_inside_planes_of_exactly_their_samples(planar_program):
    """(d) every plane a malloc of cw * ch bytes, top-down and bottom-up: the sanitizer is the bounds check"""
    cases, blob = [], []
    for w, h in HOOK_SIZES:
        for sub, filt in plm.FORMS:
            plane = random_plane(sub, w, h, 77)
            cases.append((sub, filt, w, h, plm.upsample(sub, filt, plane, w, h)))
            blob.append(struct.pack("<IIII", sub, filt, w, h) + plane.tobytes())
    got = planar_program("planes", data=struct.pack("<I", len(cases)) + b"".join(blob))
    at = 0
    for sub, filt, w, h, want in cases:
        assert np.array_equal(got[at:at + w * h].reshape(h, w), want), (plm.SUB_NAMES[sub], cm.FILTER_NAMES[filt], w, h)
        at += w * h
    assert at == got.size


# ---- names ----
def test_the_headers_constants_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define (HYDAMD_I4(?:20|22|44)[CL]?_\w+) (\d+)\s*$", text, re.M)}
    want = {}
    for sub, filt in plm.FORMS:
        for m, name in enumerate(("BT709", "BT709_FULL", "BT601", "BT601_FULL")):
            stem = f"I{('420', '422', '444')[sub]}{('', 'C', 'L')[filt]}_{name}"
            assert getattr(device, stem) == plm.sample_fmt(m, sub, filt)
            assert device.planar_fmt(16 + m, ("420", "422", "444")[sub], cm.FILTER_NAMES[filt]) == plm.sample_fmt(m, sub, filt)
            want["HYDAMD_" + stem] = plm.sample_fmt(m, sub, filt)
    assert found == want and len(want) == 28
    assert sorted(device.PLANAR_FAMILY) == sorted(plm.FAMILY) == sorted(want.values())
    assert not set(device.PLANAR_FAMILY) & (set(device.NV12_FAMILY) | set(device.P016_FAMILY) | set(range(264)))
    assert "I420" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    # the C side's reading of each number spells the public name: layout and depth the stem, the filter the infix, the matrix the suffix
    assert {"HYDAMD_" + fm.public_name(v, format_dump.described(v)): v for v in want.values()} == want
    assert all(format_dump.described(v) == fm.describe(v) and format_dump.described(v).device for v in want.values())
    fmt_h = open(os.path.join(hbuild.CSRC, "hyd_sample_fmt.h")).read()
    assert fmt_h.count('"planar YCbCr wants the chroma planes\' pitch in pixel_stride"') == 1
    assert "planar YCbCr wants the chroma planes' pitch in pixel_stride" in text


def test_planar_yuv_names_its_format_and_fills_a_descriptor():
    import torch
    from hydrium_amd import device

    for w, h in ((8, 8), (33, 9), (200, 120)):
        for fmt in plm.FAMILY:
            sub, filt, m = plm.sub_of(fmt), plm.filter_of(fmt), plm.matrix_of(fmt)
            ch, cw = plm.chroma_shape(sub, w, h)
            ybuf, ubuf, vbuf = torch.zeros(h * (w + 5), dtype=torch.uint8), torch.zeros(ch * (cw + 3), dtype=torch.uint8), torch.zeros(ch * (cw + 3), dtype=torch.uint8)
            y, u, v = ybuf.as_strided((h, w), (w + 5, 1)), ubuf.as_strided((ch, cw), (cw + 3, 1)), vbuf.as_strided((ch, cw), (cw + 3, 1))
            pic = device.PlanarYuv(y, u, v, 16 + m, ("420", "422", "444")[sub], cm.FILTER_NAMES[filt])
            assert isinstance(pic, device.Nv12) and device.sample_fmt_of(pic) == fmt == pic.sample_fmt and pic.shape == (h, w, 3)
            assert pic.pointers() == [ybuf.data_ptr(), ubuf.data_ptr(), vbuf.data_ptr()]
            descs, fmts = device.mixed_descriptors([pic])
            d = descs[0]
            assert fmts == [fmt] and (d.row_stride, d.pixel_stride, d.width, d.height) == (w + 5, cw + 3, w, h)  # pixel_stride: the chroma pitch
            assert [d.src[0], d.src[1], d.src[2]] == pic.pointers()
    ybuf, ubuf, vbuf = (torch.zeros(n, dtype=torch.uint8) for n in (120 * 200, 60 * 100, 60 * 100))
    y, u, v = ybuf.view(120, 200), ubuf.view(60, 100), vbuf.view(60, 100)
    pic = device.PlanarYuv(y, u, v)
    assert device.sample_fmt_of(pic) == device.I420_BT709 == 512  # the defaults
    yv12 = device.PlanarYuv(y, v, u)
    assert yv12.pointers() == [ybuf.data_ptr(), vbuf.data_ptr(), ubuf.data_ptr()]
    rgb8 = torch.zeros((120, 200, 3), dtype=torch.uint8)
    assert device.mixed_descriptors([pic, rgb8], sample_fmts="each")[1] == [pic.sample_fmt, 0]
    with pytest.raises(ValueError, match="share one sample format"):
        device.mixed_descriptors([pic, rgb8])
    with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
        device.mixed_descriptors([rgb8], sample_fmts=[512])
    assert device.mixed_descriptors([rgb8], sample_fmts=[524])[1] == [524]  # no format at all: left to the library to refuse


def test_planar_yuv_refuses_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    w, h = 34, 10
    y = torch.zeros((h, w), dtype=torch.uint8)
    u, v = torch.zeros((5, 17), dtype=torch.uint8), torch.zeros((5, 17), dtype=torch.uint8)
    assert device.PlanarYuv(y, u, v).pixel_stride == 17
    with pytest.raises(ValueError, match="chroma planes"):  # a wrong chroma shape
        device.PlanarYuv(y, u[:4], v[:4])
    with pytest.raises(ValueError, match="chroma planes"):
        device.PlanarYuv(y, u, v, subsampling="422")
    with pytest.raises(ValueError, match="chroma planes"):
        device.PlanarYuv(y, u, v[:, :16])
    wide = torch.zeros((5, 40), dtype=torch.uint8)
    with pytest.raises(ValueError, match="one pitch"):  # u and v strides that differ
        device.PlanarYuv(y, u, wide[:, :17])
    with pytest.raises(ValueError, match="unit column stride"):  # a non-unit inner stride
        device.PlanarYuv(y, wide[:, :34:2], wide[:, :34:2])
    with pytest.raises(ValueError, match="unit column stride"):
        device.PlanarYuv(torch.zeros((h, 2 * w), dtype=torch.uint8)[:, ::2], u, v)
    full = torch.zeros((h, w), dtype=torch.uint8)
    assert device.PlanarYuv(y, full, full, subsampling="444").sample_fmt == 520
    for chroma in ("centre", "left"):  # a filter with "444"
        with pytest.raises(ValueError, match="4:4:4"):
            device.PlanarYuv(y, full, full, subsampling="444", chroma=chroma)
    with pytest.raises(ValueError):
        device.PlanarYuv(y, u, v, chroma="bilinear")
    with pytest.raises(ValueError):
        device.PlanarYuv(y, u, v, subsampling="411")
    for bad in (0, 32, 80, 512, 20):  # the matrix is one of the four
        with pytest.raises(ValueError):
            device.PlanarYuv(y, u, v, bad)
    with pytest.raises(ValueError, match="8-bit"):
        device.PlanarYuv(y.to(torch.int16), u, v)
    with pytest.raises(ValueError, match="8-bit"):
        device.PlanarYuv(y, torch.zeros((5, 17, 1), dtype=torch.uint8), v)


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((24, 8), np.uint8)
    for fmt in (512, 523, 531, 551):
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 64, p + 128], 0, 0, 8, 8, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_six_new_instances_have_symbols_of_their_own_and_keep_the_transform_kernels_contract():
    """k_transform_tokenize_planar<mode, HYDK_STORE_YUVP | _YUVPI>: none under the RGB8 / NV12 or the P016 instances' names, no
    scratch, and the co-residency line the NV12 instances are held to (26 granules of 1280 bytes of static LDS, 128 registers)"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_planar" in k}
    assert sorted(re.match(r"_Z27k_transform_tokenize_planarILi(\d)ELi(\d)EE", k).groups() for k in new) == \
        [(mode, store) for mode in "012" for store in "78"], sorted(res)
    assert not any(k.startswith(("_Z20", "_Z25")) for k in new)
    for name, d in sorted(new.items()):
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 26 * 1280 and d["next_free_vgpr"] <= 128, (name, d)
