"""CPU-only: the NV12 formats with interpolated chroma (HYDAMD_NV12C_*, HYDAMD_NV12L_*) where no device is needed — the
interpolation header as the host compiler built it against the numpy model of the definition; what the model promises the
GPU tests (constant chroma is the nearest-neighbour picture, results stay in 0 ... 255, the three filters differ); the
header's constants; device.Nv12's reading of the filter; the drop-in API's refusal; and what the three new instances of the
transform kernel ask of a compute unit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chroma_model as cm
import yuv_model as ym
from hydrium_amd import api, build as hbuild
from test_yuv_formats import _surface, _transform_instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK_SIZES = [(1, 1), (2, 2), (3, 3), (5, 4), (33, 9), (257, 255)]
INTERPOLATED = tuple(cm.sample_fmt(m, f) for f in (cm.CENTRE, cm.LEFT) for m in ym.MATRICES)


def random_planes(w, h, seed=7):
    rng = np.random.default_rng(seed + 1000 * w + h)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8)


def check_upsample(upsample):
    """upsample(filter, uv, w, h) -> (h, w, 2) uint8, held to the model on random planes.  Shared with the on-device test."""
    for w, h in HOOK_SIZES:
        uv = random_planes(w, h)[1]
        for filt in (cm.CENTRE, cm.LEFT):
            got, want = upsample(filt, uv, w, h), cm.upsample(filt, uv, w, h)
            assert got.dtype == np.uint8 and got.shape == want.shape == (h, w, 2)
            wrong = np.argwhere((got != want).any(-1))
            assert wrong.size == 0, (cm.FILTER_NAMES[filt], w, h, [(tuple(p), got[tuple(p)].tolist(), want[tuple(p)].tolist()) for p in wrong[:8]])


def hook(fn, *device):
    """a probe-flavour upsampling entry as upsample(filter, uv, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def upsample(filt, uv, w, h):
        uv = np.ascontiguousarray(uv)
        out = np.full((h, w, 2), 0xA5, np.uint8)
        assert fn(*device, filt, uv.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return upsample


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


# ---- the definition ----
def test_the_host_build_of_the_header_equals_the_model(probe):
    check_upsample(hook(probe.hydt_chroma_upsample_host))
    one = np.zeros((1, 1, 2), np.uint8)
    for bad in (-1, 0, 3):  # (0: nearest neighbour is not an interpolation)
        assert probe.hydt_chroma_upsample_host(bad, one.ctypes.data, one.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_chroma_upsample_host", b"hydt_chroma_upsample_device"):
        assert name in probe and name not in shipped
    assert b"hydamd_encode_lf_group_at" in shipped


def test_filter_0_is_the_nearest_neighbour_model():
    for w, h in HOOK_SIZES:
        planes = random_planes(w, h)
        for m in ym.MATRICES:
            assert np.array_equal(cm.expected_rgb(planes, m, cm.NEAREST), ym.expected_rgb(planes, m))


@pytest.mark.parametrize("w,h", HOOK_SIZES)
def test_constant_chroma_gives_the_nearest_neighbour_picture(w, h):
    y = random_planes(w, h)[0]
    for value in ((0, 0), (255, 255), (90, 201)):
        uv = np.empty(((h + 1) // 2, (w + 1) // 2, 2), np.uint8)
        uv[...] = value
        for filt in (cm.CENTRE, cm.LEFT):
            up = cm.upsample(filt, uv, w, h)
            assert (up == np.array(value, np.uint8)).all()  # (so all 0 and all 255 stay in 0 ... 255)
            for m in ym.MATRICES:
                assert np.array_equal(cm.expected_rgb((y, uv), m, filt), ym.expected_rgb((y, uv), m))


@pytest.mark.parametrize("w,h", [(8, 8), (33, 9), (257, 255), (520, 264)])
def test_the_three_filters_give_three_pictures(w, h):
    planes = random_planes(w, h)
    for m in ym.MATRICES:
        pics = [cm.expected_rgb(planes, m, f) for f in cm.FILTERS]
        assert not any(np.array_equal(pics[a], pics[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def test_the_taps_at_a_pictures_corner_by_hand():
    """4 x 4, one component: the first row and column replicate"""
    uv = np.zeros((2, 2, 2), np.uint8)
    uv[..., 0] = [[0, 160], [64, 255]]
    c = cm.upsample(cm.CENTRE, uv, 4, 4)[..., 0]
    assert c[0, 0] == 0 and c[0, 1] == (9 * 0 + 3 * 160 + 3 * 0 + 160 + 8) >> 4 and c[1, 1] == (9 * 0 + 3 * 160 + 3 * 64 + 255 + 8) >> 4
    assert c[3, 3] == 255 and c[2, 2] == (9 * 255 + 3 * 64 + 3 * 160 + 0 + 8) >> 4
    l = cm.upsample(cm.LEFT, uv, 4, 4)[..., 0]
    assert l[0, 0] == 0 and l[1, 0] == (3 * 0 + 64 + 2) >> 2 and l[1, 1] == (3 * (0 + 160) + 64 + 255 + 4) >> 3
    assert l[3, 3] == 255 and l[0, 3] == 160  # x odd in the last column: hx clamps to cx


# ---- names ----
def test_the_headers_constants_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define (HYDAMD_NV12[CL]_\w+) (\d+)\s*$", text, re.M)}
    want = {f"HYDAMD_NV12{k}_{name}": getattr(device, f"NV12{k}_{name}") for k in "CL" for name in ("BT709", "BT709_FULL", "BT601", "BT601_FULL")}
    assert found == want
    assert device.NV12_CENTER_FORMATS == (32, 33, 34, 35) == tuple(cm.sample_fmt(m, cm.CENTRE) for m in ym.MATRICES)
    assert device.NV12_LEFT_FORMATS == (48, 49, 50, 51) == tuple(cm.sample_fmt(m, cm.LEFT) for m in ym.MATRICES)
    assert device.NV12_FORMATS == (16, 17, 18, 19)
    assert len(re.findall(r"^#define (HYDAMD_NV12_\w+) (\d+)\s*$", text, re.M)) == 4  # the nearest-neighbour family keeps its four
    assert "NV12" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()


def test_nv12_takes_a_filter_by_name_or_by_number():
    from hydrium_amd import device

    buf, pitch, coff = _surface(34, 10)
    base = device.Nv12.from_surface(buf, 34, 10, pitch, coff, device.NV12_BT601)
    assert device.sample_fmt_of(base) == 18 == device.sample_fmt_of(device.Nv12(base.y, base.uv, 18, chroma="nearest"))
    for name, filt in (("centre", 1), ("center", 1), ("left", 2)):
        for m in ym.MATRICES:
            pic = device.Nv12(base.y, base.uv, 16 + m, chroma=name)
            assert device.sample_fmt_of(pic) == 16 + m + 16 * filt and pic.shape == (10, 34, 3)
            assert device.sample_fmt_of(device.Nv12(base.y, base.uv, 16 + m + 16 * filt)) == 16 + m + 16 * filt
            assert device.sample_fmt_of(device.Nv12.from_surface(buf, 34, 10, pitch, coff, 16 + m, chroma=name)) == 16 + m + 16 * filt
    assert device.sample_fmt_of(device.Nv12(base.y, base.uv, device.NV12L_BT601_FULL, chroma="left")) == 51
    with pytest.raises(ValueError):
        device.Nv12(base.y, base.uv, device.NV12C_BT709, chroma="left")  # two filters named
    with pytest.raises(ValueError):
        device.Nv12(base.y, base.uv, 16, chroma="bilinear")
    for bad in (2, 20, 31, 36, 47, 52, 64):
        with pytest.raises(ValueError):
            device.Nv12(base.y, base.uv, bad)


def test_descriptors_and_each():
    import torch
    from hydrium_amd import device

    buf, pitch, coff = _surface(34, 10)
    near, centre, left = (device.Nv12.from_surface(buf, 34, 10, pitch, coff, device.NV12_BT709, chroma=c) for c in ("nearest", "centre", "left"))
    rgb, f16 = torch.zeros((10, 34, 3), dtype=torch.uint8), torch.zeros((10, 34, 3), dtype=torch.float16)
    for pair in ([near, centre], [centre, left], [left, rgb]):
        with pytest.raises(ValueError, match="share one sample format"):
            device.mixed_descriptors(pair)
    descs, fmts = device.mixed_descriptors([near, centre, left, rgb, f16], sample_fmts="each")
    assert fmts == [16, 32, 48, 0, 3]
    for d in descs[:3]:
        assert (d.row_stride, d.pixel_stride, d.width, d.height) == (pitch, 1, 34, 10)
        assert d.src[0] == buf.data_ptr() and d.src[1] == buf.data_ptr() + coff and d.src[2] == d.src[1] + 1
    assert device.mixed_descriptors([centre, centre])[1] == [32, 32]
    assert device.mixed_descriptors([left, rgb], sample_fmts=[48, 0])[1] == [48, 0]
    with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
        device.mixed_descriptors([left, rgb], sample_fmts=[32, 0])  # another filter than the object's
    with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
        device.mixed_descriptors([left, rgb], sample_fmts=[48, 32])


def test_the_drop_in_api_refuses_the_eight_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((12, 8), np.uint8)
    for fmt in INTERPOLATED:
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 64, p + 65], 0, 0, 8, 1, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_three_new_instances_keep_the_transform_kernels_contract():
    """<HYDK_FMT_U8, mode, HYDK_STORE_NV12I>: no scratch, and the co-residency line hydamd_debug_transform_footprint documents
    (26 granules of 1280 bytes of static LDS, 128 registers), which the NV12 instances are held to"""
    res = _transform_instances()
    new = {k: v for k, v in res.items() if re.match(r"_Z20k_transform_tokenizeILi0ELi\dELi4EE", k)}
    assert sorted(re.match(r".*ILi0ELi(\d)E", k).group(1) for k in new) == ["0", "1", "2"], sorted(res)
    assert len(res) == 19, sorted(res)  # the sixteen there were, and these three
    for name, d in new.items():
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 26 * 1280 and d["next_free_vgpr"] <= 128, (name, d)
