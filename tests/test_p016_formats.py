"""CPU-only: the P010 / P012 / P016 formats (HYDAMD_P010_*, HYDAMD_P012_*, HYDAMD_P016_*) where no device is needed — the
conversion and the 16-bit chroma taps as the host compiler built them (csrc/hip/hydk_yuv16.h, through the probe library)
against the numpy model of the definition; the model against the real-valued conversion and the bound the header states;
the coefficient table; device.P016's reading of planes, depth and filter; the drop-in API's refusal; the header's constants;
and what the six new instances of the transform kernel ask of a compute unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chroma_model as cm
import p016_model as pm
import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(d, m) for d in pm.DEPTHS for m in ym.MATRICES]
ROW_IDS = [f"{pm.DEPTH_NAMES[d]}-{ym.NAMES[m]}" for d, m in ROWS]
HOOK_SIZES = [(1, 1), (2, 2), (3, 5), (33, 9), (257, 255)]
_cache = {}


def triples():
    """(n, 3) uint16, read-only: every ten-bit Y code x U and V over every 16th ten-bit code and 1023, all << 6; 2^20 seeded
    random full 16-bit triples (low bits set: the words count as stored); the 27 corners of {0, 32768, 65535}^3"""
    if "triples" not in _cache:
        codes = np.array(list(range(0, 1024, 16)) + [1023], np.uint16) << 6
        y, u, v = np.meshgrid(np.arange(1024, dtype=np.uint16) << 6, codes, codes, indexing="ij")
        grid = np.stack([y, u, v], -1).reshape(-1, 3)
        rnd = np.random.default_rng(2016).integers(0, 65536, (1 << 20, 3), dtype=np.uint16)
        k = np.array([0, 32768, 65535], np.uint16)
        corners = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
        t = np.ascontiguousarray(np.concatenate([grid, rnd, corners]))
        assert t.shape == (1024 * 65 * 65 + (1 << 20) + 27, 3)
        t.setflags(write=False)
        _cache["triples"] = t
    return _cache["triples"]


def model_rgb(depth, matrix):
    """the model's RGB16 of triples(); made once per row and shared by the tests (and the on-device test)"""
    key = ("rgb", depth, matrix)
    if key not in _cache:
        t = triples()
        _cache[key] = pm.yuv_to_rgb(depth, matrix, t[:, 0], t[:, 1], t[:, 2])
        _cache[key].setflags(write=False)
    return _cache[key]


def check_conversion(depth, matrix, convert):
    """convert((n, 3) uint16) -> (n, 3) uint16, held to the model over triples().  Shared with the on-device test."""
    t = triples()
    got, want = convert(t), model_rgb(depth, matrix)
    assert got.dtype == np.uint16 and got.shape == want.shape
    wrong = np.flatnonzero((got != want).any(-1))
    assert wrong.size == 0, (depth, matrix, wrong.size, [(t[i].tolist(), got[i].tolist(), want[i].tolist()) for i in wrong[:8]])


def random_pairs(w, h, seed=16):
    return np.random.default_rng(seed + 1000 * w + h).integers(0, 65536, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint16)


def check_upsample(upsample):
    """upsample(filter, uv, w, h) -> (h, w, 2) uint16, held to the model on random words and on all-65535 (the top of the
    range: nothing may wrap).  Shared with the on-device test."""
    for w, h in HOOK_SIZES:
        for uv in (random_pairs(w, h), np.full(((h + 1) // 2, (w + 1) // 2, 2), 65535, np.uint16)):
            for filt in (cm.CENTRE, cm.LEFT):
                got, want = upsample(filt, uv, w, h), pm.upsample(filt, uv, w, h)
                assert got.dtype == np.uint16 and got.shape == want.shape == (h, w, 2)
                wrong = np.argwhere((got != want).any(-1))
                assert wrong.size == 0, (cm.FILTER_NAMES[filt], w, h, [(tuple(p), got[tuple(p)].tolist(), want[tuple(p)].tolist()) for p in wrong[:8]])
                if uv.min() == 65535:
                    assert (got == 65535).all()


def conversion_hook(fn, depth, matrix, *device):
    """a probe-flavour conversion entry as convert(triples)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]

    def convert(yuv):
        yuv = np.ascontiguousarray(yuv)
        rgb = np.full(yuv.shape, 0xA5A5, np.uint16)
        assert fn(*device, depth, matrix, yuv.ctypes.data, rgb.ctypes.data, len(yuv)) == 0
        return rgb

    return convert


def upsample_hook(fn, *device):
    """a probe-flavour 16-bit upsampling entry as upsample(filter, uv, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def upsample(filt, uv, w, h):
        uv = np.ascontiguousarray(uv)
        out = np.full((h, w, 2), 0xA5A5, np.uint16)
        assert fn(*device, filt, uv.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return upsample


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


# ---- the definition ----
@pytest.mark.parametrize("depth,matrix", ROWS, ids=ROW_IDS)
def test_the_host_build_of_the_conversion_equals_the_model(probe, depth, matrix):
    check_conversion(depth, matrix, conversion_hook(probe.hydt_yuv16_to_rgb_host, depth, matrix))


def test_the_conversion_hook_refuses_what_is_no_row(probe):
    one = np.zeros((1, 3), np.uint16)
    fn = probe.hydt_yuv16_to_rgb_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    for depth, matrix in ((0, 0), (4, 0), (-1, 0), (1, 4), (1, -1)):
        assert fn(depth, matrix, one.ctypes.data, one.ctypes.data, 1) == api.HYD_API_ERROR


@pytest.mark.parametrize("depth,matrix", ROWS, ids=ROW_IDS)
def test_the_model_is_within_the_stated_bound_of_the_real_conversion(depth, matrix):
    t = triples()
    err = np.abs(model_rgb(depth, matrix).astype(np.float64) - pm.yuv_to_rgb_real(depth, matrix, t[:, 0], t[:, 1], t[:, 2]))
    worst = np.unravel_index(np.argmax(err), err.shape)
    print(f"{pm.DEPTH_NAMES[depth]} {ym.NAMES[matrix]}: worst |fixed - real| = {err[worst]:.6f} at (Y, U, V) = {t[worst[0]].tolist()}, channel {worst[1]}")
    assert err[worst] <= pm.BOUND


def test_the_table_is_the_rounded_real_coefficients_and_the_headers_rows_are_the_models():
    for (depth, matrix), row in pm.TABLE.items():
        co = pm.exact_coefficients(depth, matrix)
        assert row[0] == co[0] == (4096 if ym.LIMITED[matrix] else 0)
        for fixed, real in zip(row[1:], co[1:]):
            assert fixed == int(np.floor(float(real) * 2.0 ** 20 + 0.5)) and abs(fixed - real * (1 << 20)) <= 0.5 and 0 < fixed < 1 << 23
    text = open(os.path.join(hbuild.CSRC, "hip", "hydk_yuv16.h")).read()
    body = text[text.index("hydk_yuv16_matrix(int depth, int matrix)"):]
    rows = [tuple(int(x) for x in r.split(",")) for r in re.findall(r"^\s*\{((?:\d+, ){5}\d+)\},", body, re.M)]
    assert rows == [pm.TABLE[d, m] for d in pm.DEPTHS for m in ym.MATRICES]
    for d, m in ROWS:  # limited range needs no depth
        if ym.LIMITED[m]:
            assert pm.TABLE[d, m] == pm.TABLE[1, m]


def test_anchors():
    for m in (0, 2):  # depth 10, limited: code 64 is black, 940 white
        assert pm.yuv_to_rgb(1, m, 64 << 6, 32768, 32768).tolist() == [0, 0, 0]
        assert pm.yuv_to_rgb(1, m, 940 << 6, 32768, 32768).tolist() == [65535, 65535, 65535]
        assert pm.yuv_to_rgb(1, m, 939 << 6, 32768, 32768).max() < 65535 and pm.yuv_to_rgb(1, m, 65 << 6, 32768, 32768).min() > 0
    for depth in (1, 2):  # full range: the top code of the depth is white, the one below is not
        n = pm.BITS[depth]
        for m in (1, 3):
            assert pm.yuv_to_rgb(depth, m, ((1 << n) - 1) << (16 - n), 32768, 32768).tolist() == [65535, 65535, 65535]
            assert pm.yuv_to_rgb(depth, m, ((1 << n) - 2) << (16 - n), 32768, 32768).max() < 65535
    for m in (1, 3):
        assert pm.TABLE[3, m][1] == 1 << 20
        y = np.arange(65536)
        assert (pm.yuv_to_rgb(3, m, y, 32768, 32768) == y[:, None]).all()  # depth 16, full range, neutral chroma: the identity


def test_the_host_build_of_the_taps_equals_the_model(probe):
    check_upsample(upsample_hook(probe.hydt_chroma16_upsample_host))
    one = np.zeros((1, 1, 2), np.uint16)
    for bad in (-1, 0, 3):  # (0: nearest neighbour is not an interpolation)
        assert probe.hydt_chroma16_upsample_host(bad, one.ctypes.data, one.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_16_bit_taps_are_the_8_bit_taps():
    """the same integers before the shift: 8-bit samples through the 16-bit model give the 8-bit model's picture"""
    for w, h in HOOK_SIZES:
        uv8 = np.random.default_rng(w * 7 + h).integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8)
        for filt in cm.FILTERS:
            assert np.array_equal(pm.upsample(filt, uv8.astype(np.uint16), w, h), cm.upsample(filt, uv8, w, h))


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_yuv16_to_rgb_host", b"hydt_yuv16_to_rgb_device", b"hydt_chroma16_upsample_host", b"hydt_chroma16_upsample_device"):
        assert name in probe and name not in shipped


# ---- names ----
def test_the_headers_constants_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define (HYDAMD_P01[026][CL]?_\w+) (\d+)\s*$", text, re.M)}
    want = {}
    for depth in pm.DEPTHS:
        for filt, infix in ((cm.NEAREST, ""), (cm.CENTRE, "C"), (cm.LEFT, "L")):
            for m, name in enumerate(("BT709", "BT709_FULL", "BT601", "BT601_FULL")):
                py = getattr(device, f"P0{pm.BITS[depth]}{infix}_{name}")
                assert py == pm.sample_fmt(depth, m, filt)
                want[f"HYDAMD_P0{pm.BITS[depth]}{infix}_{name}"] = py
    assert found == want and len(want) == 36
    assert sorted(want.values()) == sorted(device.P016_FAMILY) == sorted(pm.FAMILY)
    assert [min(f for f in pm.FAMILY if pm.depth_of(f) == d and pm.filter_of(f) == k) for d in pm.DEPTHS for k in cm.FILTERS] == \
        [80, 96, 112, 144, 160, 176, 208, 224, 240]
    assert not any(n.startswith("HYDAMD_NV12") for n in want)
    assert not set(device.P016_FAMILY) & (set(range(64, 80)) | set(device.NV12_FAMILY) | {0, 1, 2, 3, 4})
    assert "P01" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    # the C side's reading of each number (hyd_fmt_describe under sanitizers) spells the public name: layout and depth the
    # stem, the filter the infix, the matrix the suffix
    import format_dump
    import format_model as fm

    assert {"HYDAMD_" + fm.public_name(v, format_dump.described(v)): v for v in want.values()} == want
    assert all(format_dump.described(v) == fm.describe(v) and format_dump.described(v).device for v in want.values())


def _surface16(w, h, pitch=None, extra=0):
    """(buffer of int16 words, pitch in words, chroma offset in words) of a decoder-style allocation"""
    import torch

    pitch = pitch or (w + 1) // 2 * 2
    return torch.zeros(pitch * (h + (h + 1) // 2) + extra, dtype=torch.int16), pitch, pitch * h


@pytest.mark.parametrize("w,h", [(8, 8), (33, 9), (257, 255), (520, 264)])
def test_p016_names_its_format_and_fills_a_descriptor(w, h):
    from hydrium_amd import device

    buf, pitch, coff = _surface16(w, h, pitch=528 if w == 520 else None)
    for fmt in pm.FAMILY:
        depth, filt, m = pm.BITS[pm.depth_of(fmt)], cm.FILTER_NAMES[pm.filter_of(fmt)], 16 + pm.matrix_of(fmt)
        pic = device.P016.from_surface(buf, w, h, 2 * pitch, 2 * coff, m, chroma=filt, depth=depth)
        assert isinstance(pic, device.Nv12) and device.sample_fmt_of(pic) == fmt and pic.shape == (h, w, 3) and pic.pitch == pitch
        assert device.sample_fmt_of(device.P016(pic.y, pic.uv, fmt)) == fmt  # or by number
        assert tuple(pic.uv.shape) == ((h + 1) // 2, (w + 1) // 2, 2)
        descs, fmts = device.mixed_descriptors([pic])
        d = descs[0]
        assert fmts == [fmt]
        assert (d.row_stride, d.pixel_stride, d.width, d.height) == (pitch, 1, w, h)  # the pitch in samples
        assert d.src[0] == buf.data_ptr() and d.src[1] == buf.data_ptr() + 2 * coff and d.src[2] == d.src[1] + 2
    assert device.sample_fmt_of(device.P016(pic.y, pic.uv)) == device.P010_BT709 == 80  # the defaults: HD video, 10 bits, nearest
    # a byte buffer holding the same surface
    as_bytes = device.P016.from_surface(buf.view(__import__("torch").uint8), w, h, 2 * pitch, 2 * coff, 17, depth=12)
    assert as_bytes.pointers() == pic.pointers() and as_bytes.sample_fmt == 145 and as_bytes.pitch == pitch
    # a crop at even coordinates is planes sliced: its origins are the helper's, in words
    if w > 20 and h > 8:
        x0, y0 = 18, 6
        crop = device.P016(pic.y[y0:, x0:], pic.uv[y0 // 2:, x0 // 2:], device.NV12_BT601, depth=16)
        d = device.mixed_descriptors([crop])[0][0]
        assert crop.sample_fmt == 210 and crop.shape == (h - y0, w - x0, 3)
        assert d.src[0] == buf.data_ptr() + 2 * (y0 * pitch + x0) and d.src[1] == buf.data_ptr() + 2 * (coff + (y0 // 2) * pitch + x0)
        assert d.src[2] == d.src[1] + 2 and d.row_stride == pitch


def test_p016_refuses_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    buf, pitch, coff = _surface16(34, 10, extra=64)
    good = device.P016.from_surface(buf, 34, 10, 2 * pitch, 2 * coff)
    b8 =torch.zeros(2 * len(buf), dtype=torch.uint8)
    with pytest.raises(ValueError, match="16-bit"):  # 1-byte planes
        device.P016(b8.as_strided((10, 34), (34, 1)), b8.as_strided((5, 17, 2), (34, 2, 1), 340))
    with pytest.raises(ValueError, match="16-bit"):  # two bytes, but no integers
        device.P016(good.y.view(torch.float16), good.uv.view(torch.float16))
    for pitch_bytes, off_bytes in ((2 * pitch + 1, 2 * coff), (2 * pitch, 2 * coff + 1)):  # odd pitches and offsets in bytes
        with pytest.raises(ValueError, match="even"):
            device.P016.from_surface(buf, 34, 10, pitch_bytes, off_bytes)
    with pytest.raises(ValueError, match="one pitch"):  # planes of two pitches
        device.P016(good.y, buf.as_strided((5, 17, 2), (pitch + 2, 2, 1), coff))
    with pytest.raises(ValueError, match="unit column stride"):  # a column stride other than 1
        device.P016(buf.as_strided((10, 17), (pitch, 2)), buf.as_strided((5, 9, 2), (pitch, 2, 1), coff))
    with pytest.raises(ValueError, match="unit column stride"):
        device.P016(good.y, buf.as_strided((5, 17, 2), (pitch, 4, 1), coff))
    for depth in (8, 9, 11, 14, 0, 32):
        with pytest.raises(ValueError, match="depth"):
            device.P016(good.y, good.uv, depth=depth)
    with pytest.raises(ValueError, match="chroma plane"):
        device.P016(good.y, good.uv[:4])
    with pytest.raises(ValueError):
        device.P016(good.y, good.uv, chroma="bilinear")
    with pytest.raises(ValueError):
        device.P016(good.y, good.uv, device.P010C_BT709, chroma="left")  # two filters named
    for bad in (2, 20, 32, 48, 64, 79, 84, 128, 244):  # no matrix, and no number of the family
        with pytest.raises(ValueError):
            device.P016(good.y, good.uv, bad)
    # and device.Nv12 keeps to its own: 16-bit planes and the new numbers are not NV12
    with pytest.raises(ValueError):
        device.Nv12(good.y, good.uv)
    nv = torch.zeros(34 * 15, dtype=torch.uint8)
    with pytest.raises(ValueError):
        device.Nv12.from_surface(nv, 34, 10, 34, 340, 80)


def test_descriptors_and_each():
    import torch
    from hydrium_amd import device

    buf, pitch, coff = _surface16(34, 10)
    p010, p010l, p016 = (device.P016.from_surface(buf, 34, 10, 2 * pitch, 2 * coff, 16, chroma=c, depth=d) for c, d in (("nearest", 10), ("left", 10), ("nearest", 16)))
    nvbuf = torch.zeros(34 * 15, dtype=torch.uint8)
    nv12 = device.Nv12.from_surface(nvbuf, 34, 10, 34, 340)
    rgb8, rgb16, f16 = (torch.zeros((10, 34, 3), dtype=t) for t in (torch.uint8, torch.int16, torch.float16))
    for pair in ([p010, p010l], [p010, p016], [p010, nv12], [p010, rgb16], [rgb8, p016]):
        with pytest.raises(ValueError, match="share one sample format"):
            device.mixed_descriptors(pair)
    descs, fmts = device.mixed_descriptors([p010, nv12, rgb8, rgb16, f16, p010l, p016], sample_fmts="each")
    assert fmts == [80, 16, 0, 1, 3, 112, 208]
    assert (descs[0].row_stride, descs[0].src[2] - descs[0].src[1]) == (pitch, 2) and (descs[1].row_stride, descs[1].src[2] - descs[1].src[1]) == (34, 1)
    assert device.mixed_descriptors([p016, p016])[1] == [208, 208]
    assert device.mixed_descriptors([p010l, rgb8], sample_fmts=[112, 0])[1] == [112, 0]
    for given in ([96, 0], [176, 0], [48, 0], [112, 1], [112, 80]):  # another filter, depth, family or tensor format than the objects'
        with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
            device.mixed_descriptors([p010l, rgb8], sample_fmts=given)
    assert device.mixed_descriptors([p010l], sample_fmts=[84])[1] == [84]  # no format at all: left to the library to refuse


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((12, 8), np.uint16)
    for fmt in (80, 99, 115, 144, 243):
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 128, p + 130], 0, 0, 8, 1, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_six_new_instances_have_symbols_of_their_own_and_keep_the_transform_kernels_contract():
    """k_transform_tokenize_p016<mode, HYDK_STORE_P016 | _P016I>: none under the RGB16 instances' name, no scratch, and the
    co-residency line the NV12 instances are held to (26 granules of 1280 bytes of static LDS, 128 registers)"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_p016" in k}
    assert sorted(re.match(r"_Z25k_transform_tokenize_p016ILi(\d)ELi(\d)EE", k).groups() for k in new) == \
        [(mode, store) for mode in "012" for store in "56"], sorted(res)
    assert not any(k.startswith("_Z20k_transform_tokenizeILi1E") for k in new)
    assert len([k for k in res if k.startswith("_Z20k_transform_tokenizeILi1E")]) == 5  # the RGB16 instances keep their five
    for name, d in sorted(new.items()):
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 26 * 1280 and d["next_free_vgpr"] <= 128, (name, d)
