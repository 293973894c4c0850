"""GPU: NV12 pictures with interpolated chroma (HYDAMD_NV12C_*, HYDAMD_NV12L_*) on every entry point that reads device
pixels.  A pixel is an 8-bit RGB pixel right after the load: every file is compared whole with what the compiled reference
writes for the HYD_UINT8 picture the numpy model of the definition (chroma_model.py) makes of the same planes.  The filter
clamps at the edges of the PICTURE and reads across LF groups and tiles inside it; planes sit between 0x5A bytes."""
import ctypes as C

import numpy as np
import pytest

import chroma_model as cm
import yuv_model as ym
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_chroma_filters import INTERPOLATED, check_upsample, hook
from test_gpu_image_status import _check_outcomes
from test_gpu_mixed_batch import _check, _check_on_device, _reference_of
from test_gpu_yuv_formats import _planes as _nearest_planes, _surface

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = [16 + m + 16 * f for f in cm.FILTERS for m in ym.MATRICES]
IDS = {fmt: f"{cm.FILTER_NAMES[cm.filter_of(fmt)]}-{ym.NAMES[cm.matrix_of(fmt)]}" for fmt in FAMILY}
CENTRE, LEFT = 32, 51  # centre-sited BT.709; left-sited BT.601 full range: what the wide tests use
_cache = {}


def _planes(kind, w, h, fmt, seed=1234):
    """host (y, uv) of one picture, the same planes for every filter of a matrix: a photograph made NV12, random planes, or
    smooth luma under random chroma (what tells the filters, and every neighbour they read, apart; cheap to make at
    2050 x 2050, and chroma within 64 ... 191 keeps the reference's file and time small)"""
    if kind != "random chroma":
        return _nearest_planes(kind, w, h, 16 + cm.matrix_of(fmt), seed)
    key = ("planes", kind, w, h, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        y = ((np.add.outer(np.arange(h) * 2, np.arange(w) * 3) // 7 + rng.integers(0, 4, (h, w))) % 256).astype(np.uint8)
        uv = rng.integers(64, 192, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8)
        y.setflags(write=False)
        uv.setflags(write=False)
        _cache[key] = (y, uv)
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = cm.expected_rgb(_planes(kind, w, h, fmt, seed), cm.matrix_of(fmt), cm.filter_of(fmt))
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234):
    """the reference's file for the model's RGB8 picture of those planes; made once"""
    return _reference_of(("nv12i", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed))


def _tiled_want(kind, w, h, fmt, seed=1234):
    from oracle import refprobe

    key = ("tiled", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), _model(kind, w, h, fmt, seed), shift_x=0, shift_y=0)
    return _cache[key]


def _model_tensor(kind, w, h, fmt, seed=1234):
    import torch

    return torch.from_numpy(_model(kind, w, h, fmt, seed)).cuda()


def _nv12(kind, w, h, fmt, seed=1234, pitch=None):
    """device.Nv12 of the picture in a surface of its own — 0x5A in the pitch's slack, and the allocation ENDS with the last
    chroma byte; made once"""
    import torch
    from hydrium_amd import device

    key = ("dev", kind, w, h, fmt, seed, pitch)
    if key not in _cache:
        y, uv = _planes(kind, w, h, fmt, seed)
        p = pitch or (w + 1) // 2 * 2
        ch, cb = uv.shape[0], uv.shape[1] * 2
        host = np.full(p * (h + ch - 1) + cb, 0x5A, np.uint8)
        host[: p * h].reshape(h, p)[:, :w] = y
        for r in range(ch):
            host[p * (h + r): p * (h + r) + cb] = uv[r].reshape(-1)
        _cache[key] = device.Nv12.from_surface(torch.from_numpy(host).cuda(), w, h, p, p * h, fmt)
        torch.cuda.synchronize()
    return _cache[key]


def _frame_of(ctx, md, slots):
    """the file of the frame a DeviceContext has just been given"""
    import torch
    from hydrium_amd import device

    full = torch.zeros(ctx.blob_bound(slots), dtype=torch.uint8, device="cuda")
    ctx.export_frame(slots, full)
    ctx.sync()
    head = device.blob_header(full[:64].cpu().numpy().tobytes())
    return device.frame_from_blobs(md, [full[: int(head["total_bytes"])].cpu().numpy().tobytes()])


# ---- the interpolation itself ----
def test_the_device_build_of_the_header_equals_the_model():
    check_upsample(hook(C.CDLL(hbuild.PROBE_PATH).hydt_chroma_upsample_device, 0))


# ---- reference parity ----
SIZES = [(1, 1), (2, 2), (8, 8), (33, 9), (257, 255), (520, 264)]


@pytest.mark.parametrize("fmt", INTERPOLATED, ids=[IDS[f] for f in INTERPOLATED])
def test_photographs_and_random_planes_of_six_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    cases = [(kind, w, h, 1234 + 17 * k) for kind in ("photo", "random") for k, (w, h) in enumerate(SIZES)]
    wants = [_want(kind, w, h, fmt, s) for kind, w, h, s in cases]
    for kind, w, h, s in cases:
        if kind == "random" and min(w, h) >= 8:  # the three filters of this matrix: three files
            trio = {_want(kind, w, h, 16 + cm.matrix_of(fmt) + 16 * f, s) for f in cm.FILTERS}
            assert len(trio) == 3, (w, h)
    with device.MixedBatch(len(cases)) as mb:
        mb.encode([_nv12(kind, w, h, fmt, s) for kind, w, h, s in cases])
        _check_on_device(mb, wants)


# ---- across LF groups: the picture is the image ----
WIDE = [(2050, 10), (10, 2050), (2050, 2050)]
WIDE_CASES = [(w, h, fmt) for fmt in (CENTRE, LEFT) for w, h in WIDE]
WIDE_IDS = [f"{w}x{h}-{IDS[fmt]}" for w, h, fmt in WIDE_CASES]


def _wide(w, h, fmt):
    """the wide picture under a pitch of whole dwords, so that the dword runs meet the LF groups' edges"""
    return _nv12("random chroma", w, h, fmt, 9, pitch=(w + 3) // 4 * 4)


def test_the_wide_pictures_tell_the_filters_and_the_lf_group_edges_apart():
    """what the four tests below rest on: the picture as a whole is not the picture LF group by LF group"""
    for w, h, fmt in WIDE_CASES:
        planes, whole = _planes("random chroma", w, h, fmt, 9), _model("random chroma", w, h, fmt, 9)
        assert not np.array_equal(whole, ym.expected_rgb(planes, cm.matrix_of(fmt)))
        if w * h < 100000:  # the first LF group alone clamps where the picture reads on
            alone = cm.expected_rgb((planes[0][:2048, :2048], planes[1][:1024, :1024]), cm.matrix_of(fmt), cm.filter_of(fmt))
            assert not np.array_equal(alone, whole[:2048, :2048]), (w, h, fmt)


@pytest.mark.parametrize("w,h,fmt", WIDE_CASES, ids=WIDE_IDS)
def test_across_lf_groups_through_encode_image(w, h, fmt):
    from hydrium_amd import device

    n = -(-w // 2048) * -(-h // 2048)
    with device.DeviceContext(0, n, 0) as ctx:
        assert ctx.encode_image_tensor(_wide(w, h, fmt)) == n
        got = _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), n)
    want = _want("random chroma", w, h, fmt, 9)
    assert len(got) == len(want) and got == want


@pytest.mark.parametrize("w,h,fmt", WIDE_CASES, ids=WIDE_IDS)
def test_across_lf_groups_through_lf_group_at(w, h, fmt):
    """the caller's own loop over hydamd_encode_lf_group_at"""
    from hydrium_amd import device

    pic = _wide(w, h, fmt)
    lfx, lfy = -(-w // 2048), -(-h // 2048)
    with device.DeviceContext(0, lfx * lfy, 0) as ctx:
        ctx.begin_frame(lfx * lfy)
        for ty in range(lfy):
            for tx in range(lfx):
                ctx.encode_lf_group_at(ty * lfx + tx, pic.pointers(), pic.pitch, 1, fmt, w, h, tx * 2048, ty * 2048,
                                       min(2048, w - tx * 2048), min(2048, h - ty * 2048), ty * lfx + tx)
        ctx.finish_frame(lfx * lfy)
        got = _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), lfx * lfy)
    want = _want("random chroma", w, h, fmt, 9)
    assert len(got) == len(want) and got == want


@pytest.mark.parametrize("fmt", [CENTRE, LEFT], ids=[IDS[CENTRE], IDS[LEFT]])
def test_across_lf_groups_through_a_mixed_batch(fmt):
    from hydrium_amd import device

    with device.MixedBatch(3, max_lf_groups=8) as mb:
        mb.encode([_wide(w, h, fmt) for w, h in WIDE])
        _check(mb, [_want("random chroma", w, h, fmt, 9) for w, h in WIDE])


@pytest.mark.parametrize("w,h,fmt", WIDE_CASES, ids=WIDE_IDS)
def test_across_lf_groups_through_a_frame_batch(w, h, fmt):
    from hydrium_amd import device

    with device.FrameBatch(w, h, 1) as fb:
        fb.encode([_wide(w, h, fmt)])
        _check(fb, [_want("random chroma", w, h, fmt, 9)])


# ---- across tiles: the picture is the whole image ----
@pytest.mark.parametrize("w,h", [(300, 280), (520, 264)])
@pytest.mark.parametrize("fmt", [CENTRE, LEFT], ids=[IDS[CENTRE], IDS[LEFT]])
def test_across_the_tiles_of_a_tiled_image(fmt, w, h):
    from hydrium_amd import device

    with device.TiledImage(w, h, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_nv12("random chroma", w, h, fmt, 5))
        assert bytes(ti.read()) == _tiled_want("random chroma", w, h, fmt, 5)


# ---- layouts ----
@pytest.mark.parametrize("fmt", [CENTRE, LEFT], ids=[IDS[CENTRE], IDS[LEFT]])
def test_the_dword_loader_and_the_byte_loader_give_one_file(fmt):
    """520 x 264 — three groups wide, ragged — placed so that the dword runs apply and so that they do not; 0x5A around both
    planes and in the pitch's slack"""
    from hydrium_amd import device

    planes, want = _planes("random chroma", 520, 264, fmt, 77), _want("random chroma", 520, 264, fmt, 77)
    placed = {
        "aligned, pitch 528": _surface(planes, 528),
        "pitch 531": _surface(planes, 531),
        "pitch 1024": _surface(planes, 1024),
        "Y base + 1": _surface(planes, 528, y_shift=1),
        "Y base + 2": _surface(planes, 528, y_shift=2),
        "chroma base + 1": _surface(planes, 528, c_shift=1),
        "chroma base + 2": _surface(planes, 528, c_shift=2),
        "both + 3": _surface(planes, 528, y_shift=3, c_shift=3),
        "negative pitch": _surface(planes, 528, flip=True),
        "negative odd pitch": _surface(planes, 523, flip=True),
    }
    assert all(p % 4 == 0 for p in placed["aligned, pitch 528"][1][:2]) and placed["chroma base + 1"][1][1] % 4 == 1
    assert placed["both + 3"][1][0] % 4 == 3 == placed["both + 3"][1][1] % 4 and placed["negative pitch"][2] == -528
    with device.MixedBatch(len(placed)) as mb:
        mb.encode([(ptrs, rs, 1, 520, 264) for _, ptrs, rs in placed.values()], sample_fmt=fmt)
        _check(mb, [want] * len(placed))
        mb.encode([_nv12("random chroma", 520, 264, fmt, 77), _nv12("random chroma", 520, 264, fmt, 77, pitch=528)])  # ending with the chroma
        _check(mb, [want] * 2)


@pytest.mark.parametrize("fmt", [CENTRE, LEFT], ids=[IDS[CENTRE], IDS[LEFT]])
def test_a_crop_of_a_larger_surface_is_a_picture(fmt):
    """its edges replicate although real neighbours exist in memory"""
    from hydrium_amd import device

    x0, y0, w, h = 18, 6, 300, 270
    big = _nv12("random chroma", 520, 300, fmt, 61, pitch=528)
    by, buv = _planes("random chroma", 520, 300, fmt, 61)
    crop = device.Nv12(big.y[y0:y0 + h, x0:x0 + w], big.uv[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], fmt)
    model = cm.expected_rgb((by[y0:y0 + h, x0:x0 + w], buv[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]), cm.matrix_of(fmt), cm.filter_of(fmt))
    inside = _model("random chroma", 520, 300, fmt, 61)[y0:y0 + h, x0:x0 + w]
    assert not np.array_equal(model, inside) and np.array_equal(model[2:-2, 2:-2], inside[2:-2, 2:-2])
    with device.MixedBatch(2) as mb:
        mb.encode([crop, big])
        _check(mb, [_reference_of(("nv12i crop", fmt), model), _want("random chroma", 520, 300, fmt, 61)])


@pytest.mark.parametrize("fmt", [CENTRE, LEFT], ids=[IDS[CENTRE], IDS[LEFT]])
def test_plain_encode_lf_group_takes_the_lf_group_as_a_picture(fmt):
    from hydrium_amd import device

    big = _nv12("random chroma", 520, 300, fmt, 61, pitch=528)
    by, buv = _planes("random chroma", 520, 300, fmt, 61)
    import torch

    w, h = 256, 256  # the surface's first group, and as hydamd_encode_lf_group_at places it in the surface
    alone = torch.from_numpy(cm.expected_rgb((by[:h, :w], buv[:h // 2, :w // 2]), cm.matrix_of(fmt), cm.filter_of(fmt))).cuda()
    placed = torch.from_numpy(np.ascontiguousarray(_model("random chroma", 520, 300, fmt, 61)[:h, :w])).cuda()
    got = {}
    with device.DeviceContext(0, 1, 0) as ctx:
        for name in ("plain", "at", "alone", "placed"):
            if name in ("alone", "placed"):
                ctx.encode_image_tensor(alone if name == "alone" else placed)
            else:
                ctx.begin_frame(1)
                if name == "plain":
                    ctx.encode_lf_group(0, big.pointers(), big.pitch, 1, fmt, w, h, 0)
                else:
                    ctx.encode_lf_group_at(0, big.pointers(), big.pitch, 1, fmt, 520, 300, 0, 0, w, h, 0)
                ctx.finish_frame(1)
            ctx.sync()
            got[name] = bytes(ctx.read_payload())
    assert len(got["plain"]) > 1000 and got["plain"] == got["alone"] and got["at"] == got["placed"] and got["plain"] != got["at"]


def test_the_three_xyb_modes_give_the_same_bytes():
    from hydrium_amd import device

    got = {}
    with device.DeviceContext(0, 1, 0) as ctx:
        default = ctx.xyb_mode()
        for fmt in (CENTRE, LEFT):
            for mode in (0, 1, 2):
                ctx.set_xyb_mode(mode)
                ctx.encode_image_tensor(_nv12("random chroma", 520, 264, fmt, 77, pitch=528))
                ctx.sync()
                got[fmt, mode] = bytes(ctx.read_payload())
            ctx.set_xyb_mode(default)
            ctx.encode_image_tensor(_model_tensor("random chroma", 520, 264, fmt, 77))
            ctx.sync()
            got[fmt, "rgb8"] = bytes(ctx.read_payload())
    for fmt in (CENTRE, LEFT):
        assert len(got[fmt, 0]) > 1000 and len({got[fmt, k] for k in (0, 1, 2, "rgb8")}) == 1
    assert got[CENTRE, 0] != got[LEFT, 0]


# ---- formats side by side ----
def _side_by_side():
    import torch
    from hydrium_amd import synth

    if "f16" not in _cache:
        _cache["f16"] = synth.make_image_f32("photo", 200, 120, 35).astype(np.float16)
    fmts = [17, 33, 49]  # one matrix, the three filters, the same planes
    imgs = [_nv12("random chroma", 232, 188, f, 32) for f in fmts]
    wants = [_want("random chroma", 232, 188, f, 32) for f in fmts]
    assert len(set(wants)) == 3
    imgs += [_model_tensor("random chroma", 232, 188, 33, 32), torch.from_numpy(_cache["f16"]).cuda()]
    wants += [wants[1], _reference_of("nv12i f16", _cache["f16"].astype(np.float32))]
    return imgs, wants


def test_the_three_filters_beside_rgb8_and_float16_in_one_launch():
    from hydrium_amd import device

    imgs, wants = _side_by_side()
    with device.MixedBatch(5) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])


def test_a_nan_in_the_float16_picture_between_two_interpolated_ones():
    import torch
    from hydrium_amd import device

    imgs, wants = _side_by_side()
    bad = imgs[4].clone()
    bad.view(torch.int16)[60, 100, 1] = 0x7E01
    torch.cuda.synchronize()
    with device.MixedBatch(3, image_errors=True) as mb:
        mb.encode([imgs[1], bad, imgs[2]], sample_fmts="each")
        _check_outcomes(mb, [wants[1], wants[4], wants[2]], {1})
        mb.encode([imgs[1], imgs[4], imgs[2]], sample_fmts="each")
        _check_outcomes(mb, [wants[1], wants[4], wants[2]], set())


# ---- refusals ----
def test_sharded_frames_refuse_interpolated_chroma_and_stay_usable():
    from hydrium_amd import device

    sharded = "interpolated chroma is not sharded"
    with device.MultiFrame((0, 0), 2049, 16) as m:
        for fmt in INTERPOLATED:
            wide = _nv12("photo", 2049, 16, fmt, 3)
            with pytest.raises(device.DeviceError, match=sharded) as e:
                m.encode([wide, wide])
            assert e.value.code == api.HYD_API_ERROR
        near = _nv12("photo", 2049, 16, 19, 3)
        m.encode([near, near])
        assert bytes(m.read()) == _want("photo", 2049, 16, 19, 3)


def test_what_is_no_format_no_layout_or_no_place_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    fmt = CENTRE
    planes, want = _planes("random chroma", 200, 120, fmt, 31), _want("random chroma", 200, 120, fmt, 31)
    buf, ptrs, rs = _surface(planes, 200)
    apart = [ptrs[0], ptrs[1], ptrs[1] + 2]
    layout = "NV12 wants pixel_stride 1 and V one byte behind U"
    attempts = [(ptrs, 3, f, layout) for f in (CENTRE, LEFT)] + [(apart, 1, f, layout) for f in (CENTRE, LEFT)]
    attempts += [(ptrs, 1, bad, "Invalid Sample Format") for bad in (20, 31, 36, 47, 52, 64)]
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
        # hydamd_encode_lf_group_at: a place that is no LF group of the picture
        ctx.begin_frame(1)
        for x0, y0, w, h in ((128, 0, 72, 120), (0, 8, 200, 112), (1, 0, 199, 120)):
            with pytest.raises(device.DeviceError, match="multiples of 256") as e:
                ctx.encode_lf_group_at(0, ptrs, rs, 1, fmt, 200, 120, x0, y0, w, h, 0)
            assert e.value.code == api.HYD_API_ERROR
        for x0, y0, w, h in ((0, 0, 201, 120), (0, 0, 200, 121), (256, 0, 8, 8), (0, 256, 8, 8), (0, 0, 0, 120)):
            with pytest.raises(device.DeviceError, match="inside its picture"):
                ctx.encode_lf_group_at(0, ptrs, rs, 1, fmt, 200, 120, x0, y0, w, h, 0)
        with pytest.raises(device.DeviceError, match="inside its picture"):
            ctx.encode_lf_group_at(0, ptrs, rs, 3, 0, 200, 120, 0, 0, 201, 120, 0)  # every format, RGB8 too
        # nothing was enqueued: every object takes the good picture next
        mb.encode([(ptrs, rs, 1, 200, 120)], sample_fmt=fmt)
        _check(mb, [want])
        fb.encode([ptrs], rs, 1, fmt)
        _check(fb, [want])
        ti.encode(ptrs, rs, 1, fmt)
        tiled = bytes(ti.read())
        ctx.begin_frame(1)
        ctx.encode_lf_group_at(0, ptrs, rs, 1, fmt, 200, 120, 0, 0, 200, 120, 0)
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
        for fmt in INTERPOLATED:
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert 0 < lds <= 26 * 1280 and 0 < regs <= 128
        for bad in (20, 31, 36, 47, 52, 64):
            with pytest.raises(device.DeviceError):
                ctx.transform_footprint(bad)
