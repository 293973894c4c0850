"""CPU-only: the half-precision sample formats (HYDAMD_FLOAT16, HYDAMD_BFLOAT16) where no device is needed — the widening
header as the host compiler built it, over every 16-bit pattern; device.py's reading of a tensor's dtype; and the drop-in
API's refusal of both formats (they name device pixels)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE_F16, STORE_BF16 = 1, 2  # csrc/hip/hydk_half.h


def check_widening(storage, got):
    """got[i]: float32 bits for the 16-bit pattern i.  Finite: numpy's exact widening, bit for bit (subnormals, signed zero);
    non-finite: an all-ones exponent.  Shared with the on-device test."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    if storage == STORE_F16:
        finite = (bits & 0x7C00) != 0x7C00
        want = bits.view(np.float16).astype(np.float32).view(np.uint32)
    else:
        finite = (bits & 0x7F80) != 0x7F80
        want = bits.astype(np.uint32) << 16
    assert got.dtype == np.uint32 and got.shape == (65536,)
    assert finite.sum() == (65536 - 2 * 1024 if storage == STORE_F16 else 65536 - 2 * 128)
    wrong = np.nonzero(finite & (got != want))[0]
    assert wrong.size == 0, [(hex(int(bits[i])), hex(int(got[i])), hex(int(want[i]))) for i in wrong[:8]]
    assert ((got[~finite] & 0x7F800000) == 0x7F800000).all()
    assert ((got[~finite] >> 31) == (bits[~finite] >> 15)).all()  # (the sign goes along)


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    d = C.CDLL(hbuild.PROBE_PATH)
    d.hydt_widen_half_host.restype = C.c_int
    d.hydt_widen_half_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    return d


@pytest.mark.parametrize("storage", [STORE_F16, STORE_BF16], ids=["float16", "bfloat16"])
def test_widening_of_every_bit_pattern_on_the_host(probe, storage):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = np.full(65536, 0xDEADBEEF, np.uint32)
    assert probe.hydt_widen_half_host(storage, bits.ctypes.data, got.ctypes.data, bits.size) == 0
    check_widening(storage, got)
    assert probe.hydt_widen_half_host(0, bits.ctypes.data, got.ctypes.data, bits.size) == api.HYD_API_ERROR  # float32 is no half form


def test_the_widening_hooks_are_not_in_the_shipped_library():
    hbuild.build()
    assert b"hydt_widen_half" in open(hbuild.PROBE_PATH, "rb").read()
    assert b"hydt_widen_half" not in open(hbuild.LIB_PATH, "rb").read()


def _tensors():
    import torch

    dtypes = [torch.uint8, torch.int16, torch.float32, torch.float16, torch.bfloat16]
    return [torch.zeros((8 + k, 16, 3), dtype=dt) for k, dt in enumerate(dtypes)]


def test_a_tensor_names_its_sample_format_by_dtype():
    import torch
    from hydrium_amd import device

    assert (device.FLOAT16, device.BFLOAT16) == (3, 4)
    u8, i16, f32, f16, bf16 = _tensors()
    for t, want in ((u8, 0), (i16, 1), (f32, 2), (f16, 3), (bf16, 4), (torch.zeros((8, 8, 3), dtype=torch.int8), 0)):
        _, fmts = device.mixed_descriptors([t, t])
        assert fmts == [want, want], (t.dtype, fmts)
        planes = [t[..., c] for c in range(3)]
        _, fmts = device.mixed_descriptors([planes])
        assert fmts == [want], (t.dtype, fmts)
    with pytest.raises(ValueError):
        device.mixed_descriptors([torch.zeros((8, 8, 3), dtype=torch.float64)])
    # 2-byte tensors of three kinds do not share a format
    for a, b in ((i16, f16), (f16, bf16), (bf16, i16)):
        with pytest.raises(ValueError, match="share one sample format"):
            device.mixed_descriptors([a, b])


def test_each_over_all_five_dtypes_and_what_a_descriptor_holds():
    from hydrium_amd import device

    imgs = _tensors()
    descs, fmts = device.mixed_descriptors(imgs, sample_fmts="each")
    assert fmts == [0, 1, 2, 3, 4]
    for k, t in enumerate(imgs):  # strides in samples, channel pointers a sample apart: 2 bytes for both half formats
        d = descs[k]
        assert (d.row_stride, d.pixel_stride, d.width, d.height) == (48, 3, 16, 8 + k)
        assert [d.src[c] - d.src[0] for c in range(3)] == [0, t.element_size(), 2 * t.element_size()]
    assert device.mixed_descriptors(imgs, sample_fmts=[0, 1, 2, 3, 4])[1] == [0, 1, 2, 3, 4]
    assert device.mixed_descriptors(imgs[::-1], sample_fmts="each")[1] == [4, 3, 2, 1, 0]


def test_an_explicit_format_that_contradicts_a_dtype_raises():
    from hydrium_amd import device

    imgs = _tensors()
    for k, wrong in ((3, 1), (3, 4), (3, 2), (4, 3), (4, 1), (1, 3), (1, 4), (2, 3), (0, 4)):
        fmts = [0, 1, 2, 3, 4]
        fmts[k] = wrong
        with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
            device.mixed_descriptors(imgs, sample_fmts=fmts)
    with pytest.raises(ValueError, match="share one sample format"):
        device.mixed_descriptors([imgs[3]], sample_fmt=1)
    # a value that is no format still goes through to the library, which refuses the batch
    assert device.mixed_descriptors(imgs, sample_fmts=[0, 1, 2, 7, 4])[1] == [0, 1, 2, 7, 4]
    # bare addresses take the caller's word
    t = imgs[3]
    tup = ([t.data_ptr() + 2 * c for c in range(3)], t.stride(0), t.stride(1), t.shape[1], t.shape[0])
    assert device.mixed_descriptors([tup, tup], sample_fmts=[3, 4])[1] == [3, 4]


def test_the_drop_in_api_refuses_the_half_formats():
    """HYDAMD_FLOAT16 / HYDAMD_BFLOAT16 name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    from hydrium_amd import device

    hbuild.build()
    lib = api.Library()
    img = np.zeros((8, 8, 3), np.uint16)
    for fmt in (device.FLOAT16, device.BFLOAT16):
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 2, p + 4], 0, 0, 24, 3, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


def test_the_headers_constants_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define (HYDAMD_FLOAT16|HYDAMD_BFLOAT16) (\d+)\s*$", text, re.M)}
    assert found == {"HYDAMD_FLOAT16": device.FLOAT16, "HYDAMD_BFLOAT16": device.BFLOAT16}
    ref = open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    assert "FLOAT16" not in ref  # the drop-in header stays the reference's
