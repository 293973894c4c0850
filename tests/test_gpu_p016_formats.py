"""GPU: P010 / P012 / P016 pictures from device memory (HYDAMD_P010_*, HYDAMD_P012_*, HYDAMD_P016_*) on every entry point
that reads device pixels.  A pixel is a 16-bit RGB pixel right after the load: every file is compared whole with what the
compiled reference writes for the HYD_UINT16 picture the numpy model of the definition (p016_model.py) makes of the same
planes.  Planes sit between 0x5A5A words."""
import ctypes as C

import numpy as np
import pytest

import chroma_model as cm
import p016_model as pm
import yuv_model as ym
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_chroma_filters import _frame_of
from test_gpu_image_status import _check_outcomes
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_yuv_formats import _nv12, _source_f16, _want as _nv12_want
from test_p016_formats import ROW_IDS, ROWS, check_conversion, check_upsample, conversion_hook, upsample_hook

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

P010, P010C, P010L = 80, 97, 114  # BT.709 nearest; BT.709 full range centre-sited; BT.601 left-sited: what the wide tests use
LAYOUT = "P010/P016 wants pixel_stride 1 and V one sample behind U"
_cache = {}


def _planes(kind, w, h, fmt, seed=1234):
    """host (y, uv) uint16 of one picture: a photograph made P0xx at the format's depth, or crafted content"""
    from hydrium_amd import synth

    key = ("planes", kind, w, h, pm.depth_of(fmt), pm.matrix_of(fmt), seed)
    if key not in _cache:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        rng = np.random.default_rng(seed)
        photo = lambda: pm.p016_of_rgb(synth.make_image("photo", w, h, 16, seed), pm.depth_of(fmt), pm.matrix_of(fmt))
        if kind == "photo":
            y, uv = photo()
        elif kind == "random":  # full 16-bit words whatever the depth: the low bits count as stored; most pixels clamp
            y, uv = rng.integers(0, 65536, (h, w), dtype=np.uint16), rng.integers(0, 65536, (ch, cw, 2), dtype=np.uint16)
        elif kind in ("zeros", "ones"):
            y, uv = np.full((h, w), 0 if kind == "zeros" else 65535, np.uint16), np.full((ch, cw, 2), 0 if kind == "zeros" else 65535, np.uint16)
        elif kind == "out of range":  # luma below 4096 and above 60160, chroma beyond 4096 ... 61440, around a photograph's chroma
            y, uv = photo()
            y = np.where(rng.integers(0, 2, (h, w)) == 0, rng.integers(0, 4096, (h, w)), rng.integers(60161, 65536, (h, w))).astype(np.uint16)
            uv = uv.copy()
            uv[::3] = rng.choice(np.array([0, 1280, 4095, 61441, 64000, 65535], np.uint16), uv[::3].shape)
        elif kind == "random chroma":  # smooth luma under random chroma: tells the filters, and every neighbour they read, apart
            y = ((np.add.outer(np.arange(h) * 2, np.arange(w) * 3) // 7 + rng.integers(0, 4, (h, w))) % 256 * 257).astype(np.uint16)
            uv = rng.integers(16384, 49152, (ch, cw, 2), dtype=np.uint16)
        else:
            raise KeyError(kind)
        y.setflags(write=False)
        uv.setflags(write=False)
        _cache[key] = (y, uv)
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = pm.expected_rgb(_planes(kind, w, h, fmt, seed), fmt)
        _cache[key].setflags(write=False)
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234, linear_light=0):
    """the reference's file for the model's RGB16 picture of those planes; made once"""
    return _reference_of(("p016", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed), linear_light)


def _tiled_want(kind, w, h, fmt, seed=1234):
    from oracle import refprobe

    key = ("tiled", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), _model(kind, w, h, fmt, seed), shift_x=0, shift_y=0)
    return _cache[key]


def _model_tensor(kind, w, h, fmt, seed=1234):
    import torch

    return torch.from_numpy(_model(kind, w, h, fmt, seed).view(np.int16).copy()).cuda()  # (the cached model stays read-only)


def _surface(planes, pitch=None, y_shift=0, c_shift=0, flip=False):
    """the planes in device memory as a decoder leaves them — Y rows, then chroma rows, one pitch IN WORDS — and where they
    start: (buffer to keep alive, [Y, U, V addresses], row stride in words).  y_shift / c_shift move a plane's base by BYTES
    (even: samples are 2-byte aligned); flip stores the rows bottom-up (a negative row stride)."""
    import torch

    y, uv = planes
    (h, w), ch = y.shape, uv.shape[0]
    pitch = pitch or (w + 1) // 2 * 2
    assert pitch >= uv.shape[1] * 2 and y_shift % 2 == 0 and c_shift % 2 == 0
    host = np.full(16 + pitch * (h + ch + 2), 0x5A5A, np.uint16)
    y_at, c_at = 8 + y_shift // 2, 8 + pitch * (h + 1) + c_shift // 2  # in words (8: both planes start on a dword when nothing is shifted)
    yrows = host[y_at: y_at + pitch * h].reshape(h, pitch)
    crows = host[c_at: c_at + pitch * ch].reshape(ch, pitch)
    yrows[:, :w] = y[::-1] if flip else y
    crows[:, : uv.shape[1] * 2] = (uv[::-1] if flip else uv).reshape(ch, -1)
    buf = torch.from_numpy(host.view(np.int16)).cuda()
    base = buf.data_ptr()
    assert base % 256 == 0
    if flip:
        u = base + 2 * (c_at + (ch - 1) * pitch)
        return buf, [base + 2 * (y_at + (h - 1) * pitch), u, u + 2], -pitch
    return buf, [base + 2 * y_at, base + 2 * c_at, base + 2 * c_at + 2], pitch


def _p016(kind, w, h, fmt, seed=1234, pitch=None):
    """device.P016 of the picture in a surface of its own — 0x5A5A in the pitch's slack, and the allocation ENDS with the last
    chroma word; made once"""
    import torch
    from hydrium_amd import device

    key = ("dev", kind, w, h, fmt, seed, pitch)
    if key not in _cache:
        y, uv = _planes(kind, w, h, fmt, seed)
        p = pitch or (w + 1) // 2 * 2
        ch, cwords = uv.shape[0], uv.shape[1] * 2
        host = np.full(p * (h + ch - 1) + cwords, 0x5A5A, np.uint16)
        host[: p * h].reshape(h, p)[:, :w] = y
        for r in range(ch):
            host[p * (h + r): p * (h + r) + cwords] = uv[r].reshape(-1)
        _cache[key] = device.P016.from_surface(torch.from_numpy(host.view(np.int16)).cuda(), w, h, 2 * p, 2 * p * h, fmt)
        assert _cache[key].sample_fmt == fmt
        torch.cuda.synchronize()
    return _cache[key]


# ---- the conversion and the taps themselves ----
@pytest.mark.parametrize("depth,matrix", ROWS, ids=ROW_IDS)
def test_conversion_on_the_device(depth, matrix):
    check_conversion(depth, matrix, conversion_hook(C.CDLL(hbuild.PROBE_PATH).hydt_yuv16_to_rgb_device, depth, matrix, 0))


def test_the_device_build_of_the_taps_equals_the_model():
    check_upsample(upsample_hook(C.CDLL(hbuild.PROBE_PATH).hydt_chroma16_upsample_device, 0))


# ---- reference parity ----
SIZES = [(8, 8), (33, 9), (200, 120), (256, 256), (257, 255), (520, 264)]
# once per depth with nearest chroma, cycling the matrices over the six sizes; once per filter at depth 10
SIX = [("p010-nearest", 1, cm.NEAREST), ("p012-nearest", 2, cm.NEAREST), ("p016-nearest", 3, cm.NEAREST), ("p010-centre", 1, cm.CENTRE),
       ("p010-left", 1, cm.LEFT)]


@pytest.mark.parametrize("name,depth,filt", SIX, ids=[s[0] for s in SIX])
def test_photographs_of_six_sizes_equal_the_reference(name, depth, filt):
    from hydrium_amd import device

    cases = [(w, h, pm.sample_fmt(depth, (k + depth) % 4, filt), 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    pics = [_p016("photo", w, h, fmt, s) for w, h, fmt, s in cases]
    wants = [_want("photo", w, h, fmt, s) for w, h, fmt, s in cases]
    assert len(set(wants)) == len(SIZES)
    with device.MixedBatch(len(SIZES)) as mb:
        mb.encode(pics, sample_fmts="each")
        _check_on_device(mb, wants)


@pytest.mark.parametrize("fmt", [80, 82, 113], ids=[pm.name_of(f) for f in (80, 82, 113)])
def test_extreme_content_equals_the_reference(fmt):
    """random words under a depth-10 format: the low bits are used as stored (masking them would give another picture)"""
    from hydrium_amd import device

    kinds = ["random", "zeros", "ones"] + (["out of range"] if ym.LIMITED[pm.matrix_of(fmt)] else [])
    planes = _planes("random", 264, 200, fmt)
    rgb = _model("random", 264, 200, fmt)
    clamped = ((rgb == 0) | (rgb == 65535)).any(-1).mean()
    print(f"{pm.name_of(fmt)}: {clamped:.0%} of the random picture's pixels clamp")
    if pm.filter_of(fmt) == cm.NEAREST:  # (interpolation averages the random chroma towards neutral: fewer clamp)
        assert clamped > 0.5
    masked = pm.expected_rgb((planes[0] & 0xFFC0, planes[1] & 0xFFC0), fmt)
    assert not np.array_equal(masked, rgb)
    if "out of range" in kinds:
        y = _planes("out of range", 264, 200, fmt)[0]
        assert ((y < 4096) | (y > 60160)).all()
    with device.MixedBatch(len(kinds)) as mb:
        mb.encode([_p016(k, 264, 200, fmt) for k in kinds])
        _check(mb, [_want(k, 264, 200, fmt) for k in kinds])


@pytest.mark.parametrize("fmt", [P010, P010C], ids=[pm.name_of(P010), pm.name_of(P010C)])
def test_the_dword_loader_and_the_word_loader_give_one_file(fmt):
    """520 x 264 — three groups wide, ragged — placed so that the dword runs apply and so that they do not"""
    from hydrium_amd import device

    planes, want = _planes("random chroma", 520, 264, fmt, 77), _want("random chroma", 520, 264, fmt, 77)
    placed = {
        "aligned, pitch 528": _surface(planes, 528),
        "pitch 531": _surface(planes, 531),
        "Y base + 2": _surface(planes, 528, y_shift=2),
        "chroma base + 4": _surface(planes, 528, c_shift=4),
        "negative pitch": _surface(planes, 528, flip=True),
    }
    assert all(p % 4 == 0 for p in placed["aligned, pitch 528"][1][:2]) and placed["Y base + 2"][1][0] % 4 == 2
    assert placed["chroma base + 4"][1][1] % 8 == 4 and placed["negative pitch"][2] == -528
    with device.MixedBatch(len(placed) + 1) as mb:
        mb.encode([(ptrs, rs, 1, 520, 264) for _, ptrs, rs in placed.values()] + [_p016("random chroma", 520, 264, fmt, 77)], sample_fmt=fmt)
        _check(mb, [want] * (len(placed) + 1))


# ---- interpolation across LF groups and tiles: the picture is the image ----
@pytest.mark.parametrize("fmt", [P010C, P010L], ids=[pm.name_of(P010C), pm.name_of(P010L)])
def test_interpolation_is_continuous_across_lf_groups_and_tiles(fmt):
    from hydrium_amd import device

    wide = [(2049, 16), (16, 2049)]
    for w, h in wide:  # what this rests on: the first LF group alone clamps where the picture reads on
        planes, whole = _planes("random chroma", w, h, fmt, 9), _model("random chroma", w, h, fmt, 9)
        alone = pm.expected_rgb((planes[0][:2048, :2048], planes[1][:1024, :1024]), fmt)
        assert not np.array_equal(alone, whole[:2048, :2048]), (w, h)
    with device.MixedBatch(1, max_lf_groups=3) as mb:
        for w, h in wide:
            mb.encode([_p016("random chroma", w, h, fmt, 9, pitch=(w + 1) // 2 * 2)])
            _check(mb, [_want("random chroma", w, h, fmt, 9)])
    with device.TiledImage(520, 300, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_p016("random chroma", 520, 300, fmt, 5, pitch=528))
        assert bytes(ti.read()) == _tiled_want("random chroma", 520, 300, fmt, 5)


# ---- every entry point ----
def test_encode_image_on_four_ragged_lf_groups():
    from hydrium_amd import device

    w, h, fmt = 2300, 2100, P010L  # (smooth luma under random chroma: cheap to make at this size)
    with device.DeviceContext(0, 4, 0) as ctx:
        assert ctx.encode_image_tensor(_p016("random chroma", w, h, fmt, 3)) == 4
        got = _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), 4)
    want = _want("random chroma", w, h, fmt, 3)
    assert len(got) == len(want) and got == want


def test_frame_batch_and_the_context_batch():
    import torch
    from hydrium_amd import device

    fmt = 145  # P012, BT.709 full range
    pics = [_p016("photo", 520, 300, fmt, s, pitch=528) for s in (11, 12)]
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


def test_sharded_frames_take_nearest_and_refuse_interpolated_chroma():
    from hydrium_amd import device

    with device.MultiFrame((0, 0), 2049, 16) as m:  # two LF groups, one per shard
        for fmt in (P010C, P010L, 163, 240):
            wide = _p016("photo", 2049, 16, fmt, 3)
            with pytest.raises(device.DeviceError, match="interpolated chroma is not sharded") as e:
                m.encode([wide, wide])
            assert e.value.code == api.HYD_API_ERROR
        for fmt in (83, 208):
            near = _p016("photo", 2049, 16, fmt, 3)
            m.encode([near, near])
            assert bytes(m.read()) == _want("photo", 2049, 16, fmt, 3)


def test_both_entropy_stage_forms_and_the_three_xyb_modes_give_the_same_bytes():
    from hydrium_amd import device

    got = {}
    with device.DeviceContext(0, 1, 0) as ctx:
        default = ctx.xyb_mode()
        for fmt in (P010, P010L):
            pic, rgb = _p016("random chroma", 520, 264, fmt, 77, pitch=528), _model_tensor("random chroma", 520, 264, fmt, 77)
            for form in (4, 5):
                ctx.set_rans_waves(form)
                for name, t in (("p010", pic), ("rgb16", rgb)):
                    ctx.encode_image_tensor(t)
                    ctx.sync()
                    got[fmt, form, name] = bytes(ctx.read_payload())
            for mode in (0, 1, 2):
                ctx.set_xyb_mode(mode)
                ctx.encode_image_tensor(pic)
                ctx.sync()
                got[fmt, "mode", mode] = bytes(ctx.read_payload())
            ctx.set_xyb_mode(default)
    for fmt in (P010, P010L):
        mine = {v for k, v in got.items() if k[0] == fmt}
        assert len(got[fmt, 4, "p010"]) > 1000 and len(mine) == 1
    assert got[P010, 4, "p010"] != got[P010L, 4, "p010"]


def test_linear_light():
    from hydrium_amd import device

    with device.MixedBatch(2, linear_light=1) as mb:
        mb.encode([_p016("photo", 200, 120, 82, 4321), _p016("photo", 200, 120, 225, 4321)], sample_fmts="each")
        _check(mb, [_want("photo", 200, 120, 82, 4321, linear_light=1), _want("photo", 200, 120, 225, 4321, linear_light=1)])


# ---- formats side by side ----
def _side_by_side():
    import torch

    a, b = _p016("photo", 200, 120, P010, 31), _p016("random chroma", 232, 188, P010L, 32)
    u16, f16 = _image("photo", 232, 188, 16, 34)[0], torch.from_numpy(_source_f16()).cuda()
    if u16.dtype != torch.int16:
        u16 = u16.view(torch.int16)
    imgs = [a, _nv12("photo", 200, 120, 16, 31), _image("photo", 200, 120, 8, 36)[0], u16, f16, b]
    wants = [_want("photo", 200, 120, P010, 31), _nv12_want("photo", 200, 120, 16, 31), _reference("photo", 200, 120, 8, 36),
             _reference("photo", 232, 188, 16, 34), _reference_of("nv12 f16", _source_f16().astype(np.float32)),
             _want("random chroma", 232, 188, P010L, 32)]
    return imgs, wants


def test_p010_beside_nv12_rgb8_uint16_and_float16_in_one_launch():
    from hydrium_amd import device

    imgs, wants = _side_by_side()
    with device.MixedBatch(len(imgs)) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])


def test_a_nan_in_the_float16_neighbour_leaves_both_decoder_format_files():
    import torch
    from hydrium_amd import device

    imgs, wants = _side_by_side()
    bad = imgs[4].clone()
    bad.view(torch.int16)[60, 100, 1] = 0x7E01
    torch.cuda.synchronize()
    with device.MixedBatch(3, image_errors=True) as mb:
        mb.encode([imgs[0], bad, imgs[5]], sample_fmts="each")
        _check_outcomes(mb, [wants[0], wants[4], wants[5]], {1})
        mb.encode([imgs[0], imgs[4], imgs[5]], sample_fmts="each")
        _check_outcomes(mb, [wants[0], wants[4], wants[5]], set())


# ---- refusals ----
def test_what_is_no_layout_or_no_format_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    fmt = P010C
    planes, want = _planes("random chroma", 200, 120, fmt, 31), _want("random chroma", 200, 120, fmt, 31)
    buf, ptrs, rs = _surface(planes, 200)
    apart = [ptrs[0], ptrs[1], ptrs[1] + 4]  # V two samples behind U
    attempts = [(ptrs, 3, f, LAYOUT) for f in (P010, fmt, 243)] + [(apart, 1, f, LAYOUT) for f in (P010, fmt, 243)]
    attempts += [(ptrs, 1, bad, "Invalid Sample Format") for bad in (64, 79, 84, 128, 244)]
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
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group_at(0, p, rs, ps, f, 200, 120, 0, 0, 200, 120, 0)
        # nothing was enqueued: every object takes the good picture next
        mb.encode([(ptrs, rs, 1, 200, 120)], sample_fmt=fmt)
        _check(mb, [want])
        fb.encode([ptrs], rs, 1, fmt)
        _check(fb, [want])
        ti.encode(ptrs, rs, 1, fmt)
        tiled = bytes(ti.read())
        ctx.begin_frame(1)
        ctx.encode_lf_group(0, ptrs, rs, 1, fmt, 200, 120, 0)
        ctx.finish_frame(1)
        ctx.sync()
        sections = bytes(ctx.read_payload())
        ctx.encode_image_tensor(_model_tensor("random chroma", 200, 120, fmt, 31))
        ctx.sync()
        assert len(sections) > 1000 and sections == bytes(ctx.read_payload())
    assert tiled == _tiled_want("random chroma", 200, 120, fmt, 31)
    del buf


# ---- the kernel instances ----
def test_the_new_instances_fit_beside_an_entropy_stage_workgroup():
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        default = ctx.xyb_mode()
        for mode in (0, 1, 2):
            ctx.set_xyb_mode(mode)
            for fmt in (80, 147, 209, 99, 176, 243):  # HYDK_STORE_P016: nearest; HYDK_STORE_P016I: centre- and left-sited
                lds, regs = ctx.transform_footprint(fmt)
                print(f"transform footprint, XYB mode {mode}, format {fmt}: {lds} B of LDS, {regs} registers")
                assert 0 < lds <= 26 * 1280 and 0 < regs <= 128
        ctx.set_xyb_mode(default)
        for bad in (64, 79, 84, 128, 244):
            with pytest.raises(device.DeviceError):
                ctx.transform_footprint(bad)
