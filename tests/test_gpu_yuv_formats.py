"""GPU: NV12 pictures from device memory (HYDAMD_NV12_*) on every entry point that reads device pixels.  An NV12 pixel is an
8-bit RGB pixel from the load on: every file is compared whole with what the compiled reference writes for the HYD_UINT8
picture the numpy model of the conversion (yuv_model.py) makes of the same planes."""
import ctypes as C

import numpy as np
import pytest

import yuv_model as ym
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_image_status import _check_outcomes
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_yuv_formats import check_conversion

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FORMATS = [16, 17, 18, 19]
_cache = {}


def _planes(kind, w, h, fmt, seed=1234):
    """host (y, uv) of one picture: a photograph made NV12, or crafted content"""
    from hydrium_amd import synth

    key = ("planes", kind, w, h, fmt, seed)
    if key not in _cache:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        rng = np.random.default_rng(seed)
        if kind == "photo":
            y, uv = ym.nv12_of_rgb(synth.make_image("photo", w, h, 8, seed), fmt - 16)
        elif kind == "random":  # most pixels clamp in at least one channel
            y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw, 2), dtype=np.uint8)
        elif kind in ("zeros", "ones"):
            y, uv = np.full((h, w), 0 if kind == "zeros" else 255, np.uint8), np.full((ch, cw, 2), 0 if kind == "zeros" else 255, np.uint8)
        elif kind == "out of range":  # luma below 16 and above 235, chroma beyond 16 ... 240, around a photograph's chroma
            y, uv = ym.nv12_of_rgb(synth.make_image("photo", w, h, 8, seed), fmt - 16)
            y = np.where(rng.integers(0, 2, (h, w)) == 0, rng.integers(0, 16, (h, w)), rng.integers(236, 256, (h, w))).astype(np.uint8)
            uv = uv.copy()
            uv[::3] = rng.choice(np.array([0, 5, 15, 241, 250, 255], np.uint8), uv[::3].shape)
        else:
            raise KeyError(kind)
        y.setflags(write=False)
        uv.setflags(write=False)
        _cache[key] = (y, uv)
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234, linear_light=0):
    """the reference's file for the model's RGB8 picture of those planes; made once"""
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = ym.expected_rgb(_planes(kind, w, h, fmt, seed), fmt - 16)
    return _reference_of(("nv12",) + key, _cache[key], linear_light)


def _model_tensor(kind, w, h, fmt, seed=1234):
    import torch

    _want(kind, w, h, fmt, seed)
    return torch.from_numpy(_cache[("model", kind, w, h, fmt, seed)]).cuda()


def _surface(planes, pitch=None, y_shift=0, c_shift=0, flip=False):
    """the planes in device memory as a decoder leaves them — Y rows, then chroma rows, one pitch — and where they start:
    (buffer to keep alive, [Y, U, V addresses], row stride).  y_shift / c_shift move a plane's base by bytes; flip stores
    the rows bottom-up (a negative row stride)."""
    import torch

    y, uv = planes
    (h, w), ch = y.shape, uv.shape[0]
    pitch = pitch or (w + 1) // 2 * 2
    assert pitch >= uv.shape[1] * 2
    host = np.full(16 + pitch * (h + ch + 2), 0x5A, np.uint8)
    y_at, c_at = 8 + y_shift, 8 + pitch * (h + 1) + c_shift  # (8: both planes start on a dword when nothing is shifted)
    yrows = host[y_at: y_at + pitch * h].reshape(h, pitch)
    crows = host[c_at: c_at + pitch * ch].reshape(ch, pitch)
    yrows[:, :w] = y[::-1] if flip else y
    crows[:, : uv.shape[1] * 2] = (uv[::-1] if flip else uv).reshape(ch, -1)
    buf = torch.from_numpy(host).cuda()
    base = buf.data_ptr()
    assert base % 256 == 0
    if flip:
        return buf, [base + y_at + (h - 1) * pitch, base + c_at + (ch - 1) * pitch, base + c_at + (ch - 1) * pitch + 1], -pitch
    return buf, [base + y_at, base + c_at, base + c_at + 1], pitch


def _nv12(kind, w, h, fmt, seed=1234, pitch=None):
    """device.Nv12 of the picture in a surface of its own (pitch: the width rounded up to even, or as given); made once"""
    import torch
    from hydrium_amd import device

    key = ("dev", kind, w, h, fmt, seed, pitch)
    if key not in _cache:
        y, uv = _planes(kind, w, h, fmt, seed)
        p = pitch or (w + 1) // 2 * 2
        host = np.full(p * (h + uv.shape[0]), 0x5A, np.uint8)
        host[: p * h].reshape(h, p)[:, :w] = y
        host[p * h:].reshape(uv.shape[0], p)[:, : uv.shape[1] * 2] = uv.reshape(uv.shape[0], -1)
        _cache[key] = device.Nv12.from_surface(torch.from_numpy(host).cuda(), w, h, p, p * h, fmt)
        torch.cuda.synchronize()
    return _cache[key]


# ---- the conversion itself ----
@pytest.mark.parametrize("matrix", ym.MATRICES, ids=ym.NAMES)
def test_conversion_of_every_triple_on_the_device(matrix):
    d = C.CDLL(hbuild.PROBE_PATH)
    d.hydt_yuv_to_rgb_device.restype = C.c_int
    d.hydt_yuv_to_rgb_device.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]

    def convert(yuv):
        rgb = np.full(yuv.shape, 0xA5, np.uint8)
        assert d.hydt_yuv_to_rgb_device(0, matrix, yuv.ctypes.data, rgb.ctypes.data, len(yuv)) == 0
        return rgb

    check_conversion(matrix, convert)


# ---- reference parity ----
SIZES = [(8, 8), (33, 9), (200, 120), (256, 256), (257, 255), (520, 264)]


@pytest.mark.parametrize("fmt", FORMATS, ids=ym.NAMES)
def test_photographs_of_six_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    pics = [_nv12("photo", w, h, fmt, 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    wants = [_want("photo", w, h, fmt, 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    assert len(set(wants)) == len(SIZES)
    with device.MixedBatch(len(SIZES)) as mb:
        mb.encode(pics)
        _check_on_device(mb, wants)


@pytest.mark.parametrize("fmt", FORMATS, ids=ym.NAMES)
def test_extreme_content_equals_the_reference(fmt):
    from hydrium_amd import device

    kinds = ["random", "zeros", "ones"] + (["out of range"] if fmt in (16, 18) else [])
    rgb = ym.expected_rgb(_planes("random", 264, 200, fmt), fmt - 16)
    clamped = ((rgb == 0) | (rgb == 255)).any(-1).mean()
    print(f"{ym.NAMES[fmt - 16]}: {clamped:.0%} of the random picture's pixels clamp")
    assert clamped > 0.5
    if fmt in (16, 18):
        y = _planes("out of range", 264, 200, fmt)[0]
        assert ((y < 16) | (y > 235)).all()
    with device.MixedBatch(len(kinds)) as mb:
        mb.encode([_nv12(k, 264, 200, fmt) for k in kinds])
        _check(mb, [_want(k, 264, 200, fmt) for k in kinds])


def test_the_dword_loader_and_the_byte_loader_give_one_file():
    """520 x 264 — three groups wide, ragged: whole block rows (the dword runs, where the layout allows them) and an edge —
    placed so that the runs apply and so that they do not"""
    from hydrium_amd import device

    fmt = 16
    planes, want = _planes("photo", 520, 264, fmt, 77), _want("photo", 520, 264, fmt, 77)
    placed = {
        "aligned, pitch 528": _surface(planes, 528),
        "pitch 531": _surface(planes, 531),
        "Y base + 1": _surface(planes, 528, y_shift=1),
        "chroma base + 2": _surface(planes, 528, c_shift=2),
        "negative pitch": _surface(planes, 528, flip=True),
    }
    assert all(p % 4 == 0 for p in placed["aligned, pitch 528"][1][:2]) and placed["Y base + 1"][1][0] % 4 == 1
    assert placed["chroma base + 2"][1][1] % 4 == 2 and placed["chroma base + 2"][1][0] % 4 == 0 and placed["negative pitch"][2] == -528
    with device.MixedBatch(len(placed)) as mb:
        mb.encode([(ptrs, rs, 1, 520, 264) for _, ptrs, rs in placed.values()], sample_fmt=fmt)
        _check(mb, [want] * len(placed))


def test_a_crop_at_even_coordinates_of_a_larger_surface():
    from hydrium_amd import device

    fmt, (x0, y0, w, h) = 18, (18, 6, 300, 270)
    big = _nv12("photo", 520, 300, fmt, 61, pitch=528)
    by, buv = _planes("photo", 520, 300, fmt, 61)
    crop = device.Nv12(big.y[y0:y0 + h, x0:x0 + w], big.uv[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], fmt)
    model = ym.expected_rgb((by[y0:y0 + h, x0:x0 + w], buv[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]), fmt - 16)
    whole = ym.expected_rgb((by, buv), fmt - 16)
    assert np.array_equal(model, whole[y0:y0 + h, x0:x0 + w])  # (even coordinates: the crop keeps its chroma pairs)
    want = _reference_of(("nv12 crop", x0, y0, w, h), model)
    with device.MixedBatch(2) as mb:
        mb.encode([crop, big])
        _check(mb, [want, _want("photo", 520, 300, fmt, 61)])


# ---- every entry point ----
def test_encode_image_on_four_ragged_lf_groups():
    import torch
    from hydrium_amd import device

    w, h, fmt = 2300, 2100, 16
    pic, want = _nv12("photo", w, h, fmt, 3), _want("photo", w, h, fmt, 3)
    md = api.HYDImageMetadata(w, h, 0, -1, -1)
    with device.DeviceContext(0, 4, 0) as ctx:
        assert ctx.encode_image_tensor(pic) == 4
        full = torch.zeros(ctx.blob_bound(4), dtype=torch.uint8, device="cuda")
        ctx.export_frame(4, full)
        ctx.sync()
        head = device.blob_header(full[:64].cpu().numpy().tobytes())
        blob = full[: int(head["total_bytes"])].cpu().numpy().tobytes()
    got = device.frame_from_blobs(md, [blob])
    assert len(got) == len(want) and got == want


def test_frame_batch_and_the_context_batch():
    import torch
    from hydrium_amd import device

    fmt = 17
    pics = [_nv12("photo", 520, 300, fmt, s, pitch=528) for s in (11, 12)]
    wants = [_want("photo", 520, 300, fmt, s) for s in (11, 12)]
    with device.FrameBatch(520, 300, 2) as fb:
        fb.encode(pics)
        _check(fb, wants)
    rgb = [_model_tensor("photo", 520, 300, fmt, s) for s in (11, 12)]  # DeviceContext leaves sections, not a file
    with device.DeviceContext(0, 2, 0) as ctx:
        got = []
        for pair in (pics, rgb):
            ctx.encode_image_batch(pair)
            ctx.sync()
            got.append(bytes(ctx.read_payload()))
        assert len(got[0]) > 2000 and got[0] == got[1]
    torch.cuda.synchronize()


def test_mixed_batch_with_two_lf_groups_tiled_image_and_multi_frame():
    from hydrium_amd import device
    from oracle import refprobe

    fmt = 19
    wide, small = _nv12("photo", 2049, 16, fmt, 3), _nv12("photo", 33, 9, fmt, 22)
    wants = [_want("photo", 2049, 16, fmt, 3), _want("photo", 33, 9, fmt, 22)]
    with device.MixedBatch(2, max_lf_groups=3) as mb:
        mb.encode([wide, small])
        _check(mb, wants)
        mb.encode([small, wide])
        _check(mb, wants[::-1])

    pic = _nv12("photo", 520, 300, fmt, 5, pitch=528)
    _want("photo", 520, 300, fmt, 5)
    model = _cache[("model", "photo", 520, 300, fmt, 5)]
    want = api.encode_image(refprobe.reference_library(optimised=True), model, shift_x=0, shift_y=0)
    with device.TiledImage(520, 300, 0, 0) as ti:  # six tiles of 256 x 256, every one a frame
        ti.encode(pic)
        assert bytes(ti.read()) == want

    with device.MultiFrame((0, 0), 2049, 16) as m:  # two LF groups, one per shard: the second starts 2048 bytes into both planes
        m.encode([wide, wide])
        assert bytes(m.read()) == wants[0]


# ---- formats side by side ----
def _side_by_side():
    import torch

    a, b = _nv12("photo", 200, 120, 16, 31), _nv12("photo", 232, 188, 19, 32)
    u16, f16 = _image("photo", 232, 188, 16, 34)[0], torch.from_numpy(_source_f16()).cuda()
    if u16.dtype != torch.int16:
        u16 = u16.view(torch.int16)
    imgs = [a, _model_tensor("photo", 200, 120, 16, 31), u16, f16, b]
    wants = [_want("photo", 200, 120, 16, 31)] * 2 + [_reference("photo", 232, 188, 16, 34), _reference_of("nv12 f16", _source_f16().astype(np.float32)),
                                                      _want("photo", 232, 188, 19, 32)]
    return imgs, wants


def _source_f16():
    from hydrium_amd import synth

    if "f16" not in _cache:
        _cache["f16"] = synth.make_image_f32("photo", 200, 120, 35).astype(np.float16)
    return _cache["f16"]


def test_nv12_beside_rgb8_uint16_and_float16_in_one_launch():
    from hydrium_amd import device

    imgs, wants = _side_by_side()
    with device.MixedBatch(5) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        files = [bytes(f) for f in mb.read()]
        assert files[0] == files[1]  # the NV12 picture and its own RGB8 picture
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])


def test_a_nan_in_the_float16_neighbour_leaves_both_nv12_files():
    import torch
    from hydrium_amd import device

    imgs, wants = _side_by_side()
    bad = imgs[3].clone()
    bad.view(torch.int16)[60, 100, 1] = 0x7E01
    torch.cuda.synchronize()
    with device.MixedBatch(5, image_errors=True) as mb:
        mb.encode(imgs[:3] + [bad, imgs[4]], sample_fmts="each")
        _check_outcomes(mb, wants, {3})
        mb.encode(imgs, sample_fmts="each")
        _check_outcomes(mb, wants, set())


# ---- the stages behind the transform ----
def test_both_entropy_stage_forms_give_the_same_bytes():
    from hydrium_amd import device

    fmt = 16
    pic, rgb = _nv12("photo", 520, 264, fmt, 77, pitch=528), _model_tensor("photo", 520, 264, fmt, 77)
    with device.DeviceContext(0, 1, 0) as ctx:
        got = {}
        for form in (4, 5):
            ctx.set_rans_waves(form)
            for name, t in (("nv12", pic), ("rgb8", rgb)):
                ctx.encode_image_tensor(t)
                ctx.sync()
                got[form, name] = bytes(ctx.read_payload())
    assert len(got[4, "nv12"]) > 1000 and len(set(got.values())) == 1


def test_linear_light():
    from hydrium_amd import device

    with device.MixedBatch(1, linear_light=1) as mb:
        mb.encode([_nv12("photo", 200, 120, 18, 4321)])
        _check(mb, [_want("photo", 200, 120, 18, 4321, linear_light=1)])


# ---- refusals ----
def test_what_is_no_nv12_layout_or_no_format_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device
    from oracle import refprobe

    fmt = 16
    planes, want = _planes("photo", 200, 120, fmt, 31), _want("photo", 200, 120, fmt, 31)
    buf, ptrs, rs = _surface(planes, 200)
    apart = [ptrs[0], ptrs[1], ptrs[1] + 2]
    layout = "NV12 wants pixel_stride 1 and V one byte behind U"
    attempts = [(ptrs, 3, fmt, layout), (apart, 1, fmt, layout)] + [(ptrs, 1, bad, "Invalid Sample Format") for bad in (5, 15, 20)]
    with device.MixedBatch(2) as mb, device.FrameBatch(200, 120, 2) as fb, device.TiledImage(200, 120, 0, 0) as ti, \
            device.DeviceContext(0, 1, 0) as ctx:
        for p, ps, f, message in attempts:
            with pytest.raises(device.DeviceError, match=message) as e:
                mb.encode([(p, rs, ps, 200, 120)], sample_fmts=[f])
            assert e.value.code == api.HYD_API_ERROR
            with pytest.raises(device.DeviceError, match=message):
                mb.encode([(p, rs, ps, 200, 120)], sample_fmt=f)
            with pytest.raises(device.DeviceError, match=message):
                fb.encode([p], rs, ps, f)
            with pytest.raises(device.DeviceError, match=message):
                ti.encode(p, rs, ps, f)
            ctx.begin_frame(1)
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group(0, p, rs, ps, f, 200, 120, 0)
        # nothing was enqueued: every object takes the good picture next
        mb.encode([(ptrs, rs, 1, 200, 120)], sample_fmt=fmt)
        _check(mb, [want])
        fb.encode([ptrs], rs, 1, fmt)
        _check(fb, [want])
        ti.encode(ptrs, rs, 1, fmt)
        tiled = bytes(ti.read())
        tiled_want = api.encode_image(refprobe.reference_library(optimised=True), _cache[("model", "photo", 200, 120, fmt, 31)], shift_x=0,
                                      shift_y=0)
        ctx.begin_frame(1)
        ctx.encode_lf_group(0, ptrs, rs, 1, fmt, 200, 120, 0)
        ctx.finish_frame(1)
        ctx.sync()
        sections = bytes(ctx.read_payload())
        ctx.encode_image_tensor(_model_tensor("photo", 200, 120, fmt, 31))
        ctx.sync()
        assert len(sections) > 1000 and sections == bytes(ctx.read_payload())
    assert tiled == tiled_want
    del buf


# ---- the kernel instances ----
def test_the_nv12_instances_fit_beside_an_entropy_stage_workgroup():
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        for fmt in FORMATS:
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert 0 < lds <= 26 * 1280 and 0 < regs <= 128
        for bad in (5, 15, 20):
            with pytest.raises(device.DeviceError):
                ctx.transform_footprint(bad)
