"""GPU: float16 and bfloat16 pixels from device memory (HYDAMD_FLOAT16, HYDAMD_BFLOAT16) on every entry point that reads
device pixels.  A half sample is a float32 sample stored in two bytes: every file is compared whole with what the compiled
reference writes for the picture's exact float32 widening, computed on the host."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from hydrium_amd import build as hbuild
from test_gpu_image_status import _check_outcomes
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_half_formats import STORE_BF16, STORE_F16, check_widening

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FORMATS = ["float16", "bfloat16"]
_cache = {}


def _dtype(fmt):
    import torch

    return {"float16": torch.float16, "bfloat16": torch.bfloat16}[fmt]


def _widened(t):
    """the exact float32 widening of a half tensor, on the host"""
    import torch

    if t.dtype == torch.bfloat16:
        return (t.cpu().view(torch.int16).numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    return t.float().cpu().numpy()


def _source(kind, w, h, seed):
    from hydrium_amd import synth

    if kind == "gamut":  # what the float tests hold to the reference outside [0, 1]
        img = synth.make_image_f32("photo", w, h, seed).copy()
        img[:64, :64] *= 300
        return img
    if kind == "noise2":
        return synth.make_image_f32("noise", w, h, seed) * np.float32(2) - np.float32(0.5)
    return synth.make_image_f32(kind, w, h, seed)


def _half(kind, w, h, fmt, seed=1234, linear_light=0):
    """(half device tensor (H, W, 3), the reference's file for its float32 widening); made once"""
    import torch

    key = (kind, w, h, fmt, seed)
    if key not in _cache:
        t = torch.from_numpy(_source(kind, w, h, seed)).to(_dtype(fmt)).cuda()
        torch.cuda.synchronize()
        _cache[key] = (t, _widened(t))
    t, wide = _cache[key]
    return t, _reference_of(("half",) + key, wide, linear_light)


# ---- the widening itself ----
@pytest.mark.parametrize("storage", [STORE_F16, STORE_BF16], ids=FORMATS)
def test_widening_of_every_bit_pattern_on_the_device(storage):
    d = C.CDLL(hbuild.PROBE_PATH)
    d.hydt_widen_half_device.restype = C.c_int
    d.hydt_widen_half_device.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = np.full(65536, 0xDEADBEEF, np.uint32)
    assert d.hydt_widen_half_device(0, storage, bits.ctypes.data, got.ctypes.data) == 0
    check_widening(storage, got)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_pattern_below_two_codes_as_its_float32_widening_does(fmt):
    """the new loader against the existing float path on the same card: R, G and B each carry every pattern with |v| < 2
    (subnormals, both zeros, both signs: 32 768 of them in either format) in a permutation of its own, the rest 0.5"""
    import torch
    from hydrium_amd import device

    patterns = np.array([b for b in range(65536) if (b & 0x7FFF) < 0x4000], np.uint16)  # 2.0 is 0x4000 in both formats
    assert patterns.size == 32768
    half_of_one = {"float16": 0x3800, "bfloat16": 0x3F00}[fmt]
    rng = np.random.default_rng(7)
    planes = []
    for _ in range(3):
        cells = np.full(65536, half_of_one, np.uint16)
        cells[:32768] = patterns
        planes.append(rng.permutation(cells))
    bits = np.stack(planes, -1).reshape(256, 256, 3)
    half = torch.from_numpy(bits.view(np.int16)).cuda().view(_dtype(fmt))
    wide = torch.from_numpy(_widened(half)).cuda()
    assert wide.dtype == torch.float32 and float(wide.abs().max()) < 2 and float(wide.min()) < 0
    with device.MixedBatch(2) as mb:
        mb.encode([half, wide], sample_fmts="each")
        mb.result()
        a, b = (bytes(f) for f in mb.read())
    assert len(a) > 1000 and a == b


# ---- reference parity ----
SIZES = [(8, 8), (33, 9), (200, 120), (256, 256), (257, 256), (520, 264)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_photographs_of_six_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    pairs = [_half("photo", w, h, fmt, 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    wants = [p[1] for p in pairs]
    assert len(set(wants)) == len(SIZES)
    with device.MixedBatch(len(SIZES)) as mb:
        mb.encode([p[0] for p in pairs])
        _check_on_device(mb, wants)


@pytest.mark.parametrize("fmt", FORMATS)
def test_linear_light_and_out_of_gamut_pictures_equal_the_reference(fmt):
    from hydrium_amd import device

    t, want = _half("photo", 200, 120, fmt, 4321, linear_light=1)
    with device.MixedBatch(1, linear_light=1) as mb:
        mb.encode([t])
        _check(mb, [want])
    pairs = [_half("gamut", 232, 188, fmt), _half("noise2", 232, 188, fmt, 99)]
    assert float(pairs[0][0].float().max()) > 10 and float(pairs[1][0].float().min()) < 0
    with device.MixedBatch(2) as mb:
        mb.encode([p[0] for p in pairs])
        _check_on_device(mb, [p[1] for p in pairs])


def _layouts(t):
    """the picture `t` (H, W, 3, contiguous) in every layout the loader tells apart, as MixedBatch takes them"""
    import torch

    h, w, _ = t.shape
    planar = t.permute(2, 0, 1).contiguous()  # NCHW: three planes, rows of w samples
    rgba = torch.zeros((h, w, 4), dtype=t.dtype, device=t.device)
    rgba[..., :3] = t
    off = torch.zeros(h * w * 3 + 1, dtype=t.dtype, device=t.device)  # one sample into a buffer: a base that is no dword's
    off[1:] = t.reshape(-1)
    odd_rows = torch.zeros((h, w * 3 + 1), dtype=t.dtype, device=t.device)  # rows an odd number of samples apart
    odd_rows[:, : w * 3] = t.reshape(h, w * 3)
    odd_planes = torch.zeros((3, h, w + 1 - w % 2), dtype=t.dtype, device=t.device)
    odd_planes[:, :, :w] = planar
    out = {
        "interleaved": t,
        "planes": [planar[c] for c in range(3)],
        "rgba": rgba,
        "odd base": off[1:].view(h, w, 3),
        "odd row stride": odd_rows[:, : w * 3].unflatten(1, (w, 3)),
        "planes, odd row stride": [odd_planes[c, :, :w] for c in range(3)],
    }
    assert out["odd base"].data_ptr() % 4 == 2 and out["odd row stride"].stride(0) % 2 == 1
    assert out["planes, odd row stride"][0].stride(0) % 2 == 1 and out["rgba"].stride(1) == 4
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", [(200, 120), (264, 136)])
def test_every_layout_gives_the_one_reference_file(fmt, w, h):
    from hydrium_amd import device

    t, want = _half("photo", w, h, fmt, 77)
    lay = _layouts(t)
    with device.MixedBatch(len(lay)) as mb:
        mb.encode(list(lay.values()))
        _check(mb, [want] * len(lay))


# ---- every entry point ----
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_context_entry_points(fmt):
    """DeviceContext leaves sections, not a file: the half picture's sections are those of its float32 widening (which the
    existing tests hold to the reference)"""
    import torch
    from hydrium_amd import device

    halves = [_half("photo", 520, 264, fmt, s)[0] for s in (5, 6)]
    wides = [torch.from_numpy(_widened(t)).cuda() for t in halves]
    with device.DeviceContext(0, 2, 0) as ctx:
        got = []
        for t in (halves[0], wides[0]):
            ctx.encode_image_tensor(t)
            ctx.sync()
            got.append(bytes(ctx.read_payload()))
        assert len(got[0]) > 1000 and got[0] == got[1]
        got = []
        for pair in (halves, wides):
            ctx.encode_image_batch(pair)
            ctx.sync()
            got.append(bytes(ctx.read_payload()))
        assert len(got[0]) > 2000 and got[0] == got[1]


@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_batch_tiled_image_and_multi_frame(fmt):
    from hydrium_amd import api, device
    from oracle import refprobe

    pairs = [_half("photo", 200, 120, fmt, s) for s in (11, 12, 13)]
    with device.FrameBatch(200, 120, 3) as fb:
        fb.encode([p[0] for p in pairs])
        _check(fb, [p[1] for p in pairs])
        planar = [p[0].permute(2, 0, 1).contiguous() for p in pairs]
        fb.encode([[q[c] for c in range(3)] for q in planar])
        _check(fb, [p[1] for p in pairs])

    t, _ = _half("photo", 520, 264, fmt, 5)
    ref = refprobe.reference_library(optimised=True)
    want = api.encode_image(ref, _widened(t), shift_x=0, shift_y=0)
    with device.TiledImage(520, 264, 0, 0) as ti:  # six tiles of 256 x 256, every one a frame
        ti.encode(t)
        assert bytes(ti.read()) == want
        planar = t.permute(2, 0, 1).contiguous()
        ti.encode([planar[c] for c in range(3)])
        assert bytes(ti.read()) == want

    t, want = _half("photo", 2049, 16, fmt, 3)  # two LF groups, one per shard: the second starts 2048 samples in
    with device.MultiFrame((0, 0), 2049, 16) as m:
        m.encode([t, t])
        assert bytes(m.read()) == want


@pytest.mark.parametrize("fmt", FORMATS)
def test_mixed_batches_of_one_format_five_formats_and_two_lf_groups(fmt):
    from hydrium_amd import device

    a, b = _half("photo", 232, 188, fmt, 21), _half("photo", 33, 9, fmt, 22)
    with device.MixedBatch(2) as mb:
        mb.encode([a[0], b[0]], sample_fmt={"float16": device.FLOAT16, "bfloat16": device.BFLOAT16}[fmt])
        _check(mb, [a[1], b[1]])
    wide = _half("photo", 2049, 16, fmt, 3)
    with device.MixedBatch(2, max_lf_groups=3) as mb:
        mb.encode([wide[0], b[0]])
        _check(mb, [wide[1], b[1]])
        mb.encode([b[0], wide[0]])
        _check(mb, [b[1], wide[1]])


def test_five_sample_formats_in_one_batch():
    import torch
    from hydrium_amd import device

    f16, bf16 = _half("photo", 200, 120, "float16", 31), _half("photo", 232, 188, "bfloat16", 32)
    imgs = [_image("photo", 200, 120, 8, 33)[0], _image("photo", 232, 188, 16, 34)[0], _image("photo", 200, 120, 32, 35)[0], f16[0], bf16[0]]
    if imgs[1].dtype != torch.int16:
        imgs[1] = imgs[1].view(torch.int16)
    wants = [_reference("photo", 200, 120, 8, 33), _reference("photo", 232, 188, 16, 34), _reference("photo", 200, 120, 32, 35), f16[1], bf16[1]]
    with device.MixedBatch(5) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])


# ---- non-finite samples ----
BAD = [("float16", 0x7C00), ("float16", 0x7E01), ("bfloat16", 0x7FC1)]  # +inf, a NaN, a NaN


@pytest.mark.parametrize("fmt,bits", BAD, ids=["f16-inf", "f16-nan", "bf16-nan"])
def test_a_non_finite_half_sample_is_what_a_non_finite_float_is(fmt, bits):
    import torch
    from hydrium_amd import device

    t, want = _half("photo", 200, 120, fmt, 41)
    other, other_want = _half("photo", 232, 188, fmt, 42)
    bad = t.clone()
    bad.view(torch.int16)[60, 100, 1] = bits
    rgba = torch.zeros((120, 200, 4), dtype=t.dtype, device="cuda")  # pixel stride 4: the per-sample loader
    rgba[..., :3] = bad
    planar = bad.permute(2, 0, 1).contiguous()
    torch.cuda.synchronize()
    layouts = {"interleaved": bad, "planes": [planar[c] for c in range(3)], "rgba": rgba}
    with device.MixedBatch(3) as mb, device.MixedBatch(3, image_errors=True) as flagged:
        for name, given in layouts.items():
            mb.encode([other, given, t])
            with pytest.raises(device.DeviceError, match="NaN"):
                mb.result()
            mb.encode([other, t])  # the object stays usable
            _check(mb, [other_want, want])
            flagged.encode([other, given, t])
            _check_outcomes(flagged, [other_want, want, want], {1})
        flagged.encode([other, t, t])
        _check_outcomes(flagged, [other_want, want, want], set())


# ---- the kernel instances ----
def test_the_half_instances_ask_for_no_more_lds_than_the_float32_instance():
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        lds32, regs32 = ctx.transform_footprint(2)
        for fmt in (device.FLOAT16, device.BFLOAT16):
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers (float32: {lds32} B, {regs32})")
            assert 0 < lds <= lds32 and 0 < regs <= 128  # four wavefronts per SIMD, as the kernel is compiled for
        for bad in (5, 7, -1):
            with pytest.raises(device.DeviceError):
                ctx.transform_footprint(bad)
