"""CPU-only: the NV12 sample formats (HYDAMD_NV12_*) where no device is needed — the conversion header as the host compiler
built it, over all 2^24 (Y, U, V) triples, against the numpy model; the model against real arithmetic and the coefficient
table against Kr, Kb and the ranges; device.Nv12's reading of a decoder surface; the drop-in API's refusal of the four
formats (they name device pixels); and what the three NV12 instances of the transform kernel ask of a compute unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y_CHUNK = 32  # the 2^24 triples are walked 32 luma values (2^21 triples) at a time


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    d = C.CDLL(hbuild.PROBE_PATH)
    d.hydt_yuv_to_rgb_host.restype = C.c_int
    d.hydt_yuv_to_rgb_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    return d


def check_conversion(matrix, convert):
    """convert(yuv (n, 3) uint8) -> rgb (n, 3) uint8, held to the model over every triple.  Shared with the on-device test."""
    for lo in range(0, 256, Y_CHUNK):
        yuv = ym.all_triples(lo, lo + Y_CHUNK)
        got = convert(yuv)
        want = ym.yuv_to_rgb(matrix, yuv[:, 0], yuv[:, 1], yuv[:, 2])
        assert got.dtype == np.uint8 and got.shape == want.shape
        wrong = np.nonzero((got != want).any(1))[0]
        assert wrong.size == 0, [(yuv[i].tolist(), got[i].tolist(), want[i].tolist()) for i in wrong[:8]]


@pytest.mark.parametrize("matrix", ym.MATRICES, ids=ym.NAMES)
def test_conversion_of_every_triple_on_the_host(probe, matrix):
    def convert(yuv):
        rgb = np.full(yuv.shape, 0xA5, np.uint8)
        assert probe.hydt_yuv_to_rgb_host(matrix, yuv.ctypes.data, rgb.ctypes.data, len(yuv)) == 0
        return rgb

    check_conversion(matrix, convert)
    one = np.zeros((1, 3), np.uint8)
    for bad in (-1, 4):
        assert probe.hydt_yuv_to_rgb_host(bad, one.ctypes.data, one.ctypes.data, 1) == api.HYD_API_ERROR


def _header_table():
    """the coefficient rows of csrc/hip/hydk_yuv.h, in its order"""
    text = open(os.path.join(ROOT, "hydrium_amd", "csrc", "hip", "hydk_yuv.h")).read()
    return [tuple(map(int, r)) for r in re.findall(r"^\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},", text, re.M)]


@pytest.mark.parametrize("matrix", ym.MATRICES, ids=ym.NAMES)
def test_the_model_is_within_0_51_of_the_real_valued_conversion(matrix):
    """half a code of rounding + less than 0.01 from the coefficients' own rounding to 14 fractional bits; and the operands
    and accumulators the device's 24-bit multiplier is trusted with.  (The model's coefficients are the library's.)"""
    assert _header_table()[matrix] == ym.TABLE[matrix]
    worst = 0.0
    for lo in range(0, 256, Y_CHUNK):
        yuv = ym.all_triples(lo, lo + Y_CHUNK)
        y, u, v = yuv[:, 0], yuv[:, 1], yuv[:, 2]
        err = np.abs(ym.yuv_to_rgb(matrix, y, u, v).astype(np.float64) - ym.yuv_to_rgb_real(matrix, y, u, v))
        worst = max(worst, float(err.max()))
    print(f"{ym.NAMES[matrix]}: the model is within {worst:.4f} of the real-valued conversion")
    assert worst <= 0.51
    yo, cy, crv, cgu, cgv, cbu = ym.TABLE[matrix]
    assert max(cy, crv, cgu, cgv, cbu) < 2 ** 23  # operands of a signed 24-bit multiply
    hi = cy * (255 - yo) + max(crv, cbu, cgu + cgv) * 128 + 8192
    lo_ = cy * (0 - yo) - max(crv, cbu, cgu + cgv) * 128
    assert hi < 2 ** 24 and lo_ > -(2 ** 24)


@pytest.mark.parametrize("matrix", ym.MATRICES, ids=ym.NAMES)
def test_the_table_is_the_real_coefficients_rounded_to_14_bits(matrix):
    yo, *real = ym.real_coefficients(matrix)
    assert ym.TABLE[matrix] == (yo,) + tuple(int(np.floor(c * 2 ** 14 + 0.5)) for c in real)
    assert _header_table() == list(ym.TABLE)  # and the header says the same numbers


def test_the_conversion_hooks_are_in_the_probe_library_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_yuv_to_rgb_host", b"hydt_yuv_to_rgb_device"):
        assert name in probe and name not in shipped


def test_the_headers_constants_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define (HYDAMD_NV12_\w+) (\d+)\s*$", text, re.M)}
    assert found == {"HYDAMD_NV12_BT709": device.NV12_BT709, "HYDAMD_NV12_BT709_FULL": device.NV12_BT709_FULL,
                     "HYDAMD_NV12_BT601": device.NV12_BT601, "HYDAMD_NV12_BT601_FULL": device.NV12_BT601_FULL}
    assert device.NV12_FORMATS == (16, 17, 18, 19) == tuple(ym.FIRST_FORMAT + m for m in ym.MATRICES)
    assert "NV12" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()  # the drop-in header stays the reference's


# ---- device.Nv12 ----
def _surface(w, h, pitch=None, extra=0):
    """(buffer, pitch, chroma offset) of a decoder-style allocation: Y rows, then chroma rows, one pitch"""
    import torch

    pitch = pitch or (w + 1) // 2 * 2
    return torch.zeros(pitch * (h + (h + 1) // 2) + extra, dtype=torch.uint8), pitch, pitch * h


@pytest.mark.parametrize("w,h", [(8, 8), (33, 9), (257, 255), (520, 264)])
def test_nv12_names_its_format_and_fills_a_descriptor(w, h):
    from hydrium_amd import device

    buf, pitch, coff = _surface(w, h, pitch=528 if w == 520 else None)
    for fmt in device.NV12_FORMATS:
        pic = device.Nv12.from_surface(buf, w, h, pitch, coff, fmt)
        assert device.sample_fmt_of(pic) == fmt and pic.shape == (h, w, 3)
        assert tuple(pic.uv.shape) == ((h + 1) // 2, (w + 1) // 2, 2)
        descs, fmts = device.mixed_descriptors([pic])
        d = descs[0]
        assert fmts == [fmt]
        assert (d.row_stride, d.pixel_stride, d.width, d.height) == (pitch, 1, w, h)
        assert d.src[0] == buf.data_ptr() and d.src[1] == buf.data_ptr() + coff and d.src[2] == d.src[1] + 1
    assert device.sample_fmt_of(device.Nv12(pic.y, pic.uv)) == device.NV12_BT709  # the default: HD video
    # a crop at even coordinates is planes sliced: its origins are the helper's (y0 * pitch + x0, y0 / 2 * pitch + x0)
    if w > 20 and h > 8:
        x0, y0 = 18, 6
        crop = device.Nv12(pic.y[y0:, x0:], pic.uv[y0 // 2:, x0 // 2:], device.NV12_BT601)
        d = device.mixed_descriptors([crop])[0][0]
        assert d.src[0] == buf.data_ptr() + y0 * pitch + x0 and d.src[1] == buf.data_ptr() + coff + (y0 // 2) * pitch + x0
        assert (d.src[2], d.row_stride, d.width, d.height) == (d.src[1] + 1, pitch, w - x0, h - y0)


def test_nv12_refuses_what_is_no_nv12_picture():
    import torch
    from hydrium_amd import device

    y = torch.zeros((9, 33), dtype=torch.uint8)
    with pytest.raises(ValueError, match="share one pitch"):  # contiguous planes of an odd width: pitches 33 and 34
        device.Nv12(y, torch.zeros((5, 17, 2), dtype=torch.uint8))
    buf, pitch, coff = _surface(34, 10)
    good = device.Nv12.from_surface(buf, 34, 10, pitch, coff)
    with pytest.raises(ValueError, match="share one pitch"):
        device.Nv12(good.y, torch.zeros((5, 40, 2), dtype=torch.uint8)[:, :17])
    with pytest.raises(ValueError):
        device.Nv12(good.y, good.uv[:4])  # a chroma row short
    with pytest.raises(ValueError):
        device.Nv12(good.y, good.uv, 2)  # float32 is no matrix
    with pytest.raises(ValueError):
        device.Nv12(good.y.to(torch.int16), good.uv)
    with pytest.raises(ValueError):
        device.Nv12(good.y.t(), torch.zeros((17, 5, 2), dtype=torch.uint8))  # a column stride that is not 1


def test_nv12_beside_rgb_tensors_needs_each():
    import torch
    from hydrium_amd import device

    buf, pitch, coff = _surface(34, 10)
    pic = device.Nv12.from_surface(buf, 34, 10, pitch, coff, device.NV12_BT601_FULL)
    other = device.Nv12.from_surface(buf, 34, 10, pitch, coff, device.NV12_BT709)
    rgb, f16 = torch.zeros((10, 34, 3), dtype=torch.uint8), torch.zeros((10, 34, 3), dtype=torch.float16)
    for pair in ([pic, rgb], [rgb, pic], [pic, other]):
        with pytest.raises(ValueError, match="share one sample format"):
            device.mixed_descriptors(pair)
    descs, fmts = device.mixed_descriptors([pic, rgb, f16, other], sample_fmts="each")
    assert fmts == [19, 0, 3, 16]
    assert (descs[0].pixel_stride, descs[1].pixel_stride) == (1, 3)
    assert device.mixed_descriptors([pic, rgb], sample_fmts=[19, 0])[1] == [19, 0]
    with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
        device.mixed_descriptors([pic, rgb], sample_fmts=[19, 16])
    with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
        device.mixed_descriptors([pic, rgb], sample_fmts=[16, 0])  # another matrix than the object's


def test_the_drop_in_api_refuses_the_nv12_formats():
    """HYDAMD_NV12_* name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    from hydrium_amd import device

    hbuild.build()
    lib = api.Library()
    img = np.zeros((12, 8), np.uint8)
    for fmt in device.NV12_FORMATS:
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 64, p + 65], 0, 0, 8, 1, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def _transform_instances():
    """{mangled name: descriptor fields} of every k_transform_tokenize instance hipcc cross-compiles from kernels.hip"""
    return {k: v for k, v in kernel_descriptors().items() if k.startswith("_Z20k_transform_tokenize")}


def test_the_three_nv12_instances_keep_the_transform_kernels_contract():
    res = _transform_instances()
    nv12 = {k: v for k, v in res.items() if re.match(r"_Z20k_transform_tokenizeILi0ELi\dELi3EE", k)}  # <HYDK_FMT_U8, mode, HYDK_STORE_NV12>
    assert sorted(re.match(r".*ILi0ELi(\d)E", k).group(1) for k in nv12) == ["0", "1", "2"], sorted(res)
    for name, d in nv12.items():
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 26 * 1280 and d["next_free_vgpr"] <= 128, (name, d)
