"""GPU: packed 4:2:2 YCbCr pictures from device memory (HYDAMD_YUY2_*, HYDAMD_YUY2C_*, HYDAMD_YUY2L_*; YUYV, UYVY, YVYU and VYUY by
the pointers) on every entry point that reads device pixels.  A pixel is an 8-bit RGB pixel right after the load: every file is
compared whole with what the compiled reference writes for the HYD_UINT8 picture the numpy model of the definition
(packed_model.py) makes of the same bytes.  Every surface sits in an allocation that ends with the last group of its last row,
or between 0x5A bytes."""
import ctypes as C

import numpy as np
import pytest

import chroma_model as cm
import packed_model as pkm
import planar_model as plm
import yuv_model as ym
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_chroma_filters import _frame_of, _nv12 as _nv12i, _want as _nv12i_want
from test_gpu_half_formats import _half
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_p016_formats import _p016, _want as _p016_want
from test_gpu_planar16_formats import _planar as _planar16, _want as _planar16_want
from test_gpu_planar_formats import _planar as _planar8, _planes as _planes8, _want as _planar8_want
from test_gpu_yuv_formats import _nv12, _want as _nv12_want
from test_packed_formats import check_definition, hook

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = sorted(pkm.FAMILY)
YUY2, YUY2C, YUY2L, YUY2C_JPEG = 8192, 8208, 8226, 8211  # what the layout and entry-point tests use
_cache = {}


def _planes(kind, w, h, fmt, seed=1234):
    """host (y, u, v) of one picture: the planar tests' 4:2:2 planes of the same matrix"""
    return _planes8(kind, w, h, plm.sample_fmt(pkm.matrix_of(fmt), plm.S422, cm.NEAREST), seed)


def _rows(kind, w, h, fmt, order="yuyv", seed=1234):
    key = ("rows", kind, w, h, pkm.matrix_of(fmt), order, seed)
    if key not in _cache:
        _cache[key] = pkm.interleave(_planes(kind, w, h, fmt, seed), order, w)
        _cache[key].setflags(write=False)
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    """the picture every byte order of those planes stands for"""
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = pkm.expected_rgb(_rows(kind, w, h, fmt, "yuyv", seed), "yuyv", w, pkm.matrix_of(fmt), pkm.filter_of(fmt))
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234):
    """the reference's file for the model's RGB8 picture of those bytes; made once"""
    return _reference_of(("packed", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed))


def _tiled_want(kind, w, h, fmt, seed=1234):
    from oracle import refprobe

    key = ("tiled", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), _model(kind, w, h, fmt, seed), shift_x=0, shift_y=0)
    return _cache[key]


def _surface(rows, pitch):
    """the rows in an allocation of its own that ENDS with the last group of the last row, 0x5A in the pitch's slack"""
    import torch

    h, row = rows.shape
    host = np.full(pitch * (h - 1) + row, 0x5A, np.uint8)
    for r in range(h):
        host[pitch * r: pitch * r + row] = rows[r]
    return torch.from_numpy(host).cuda().as_strided((h, row), (pitch, 1))


def _packed(kind, w, h, fmt, order="yuyv", seed=1234, pitch=None):
    """device.PackedYuv of the picture; pitch: the row itself (a multiple of 4), or as given; made once"""
    import torch
    from hydrium_amd import device

    key = ("dev", kind, w, h, fmt, order, seed, pitch)
    if key not in _cache:
        rows = _rows(kind, w, h, fmt, order, seed)
        _cache[key] = device.PackedYuv(_surface(rows, pitch or rows.shape[1]), w, 16 + pkm.matrix_of(fmt), order, cm.FILTER_NAMES[pkm.filter_of(fmt)])
        assert _cache[key].sample_fmt == fmt
        torch.cuda.synchronize()
    return _cache[key]


def _pointers(base, order):
    y = base + pkm.y_offset(order)
    du, dv = pkm.ORDERS[order]
    return [y, y + du, y + dv]


def _place(rows, order, pitch, shift=0, flip=False):
    """the surface at a bare address between 0x5A bytes: (buffer to keep alive, [Y, U, V addresses], row stride).  shift moves the
    first group off the dword; flip stores the rows bottom-up: a negative pitch"""
    import torch

    h, row = rows.shape
    host = np.full((16 + pitch * (h + 2) + 255) // 256 * 256, 0x5A, np.uint8)
    at = 8 + shift
    for r in range(h):
        o = at + pitch * (h - 1 - r if flip else r)
        host[o: o + row] = rows[r]
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0
    first = buf.data_ptr() + at + (pitch * (h - 1) if flip else 0)
    return buf, _pointers(first, order), -pitch if flip else pitch


# ---- the definition on the device ----
def test_the_device_build_of_the_definition_equals_the_model():
    check_definition(hook(C.CDLL(hbuild.PROBE_PATH).hydt_packed_to_rgb_device, 0), widths=(1, 7, 8, 33))


# ---- reference parity ----
SIZES = [(1, 5), (7, 3), (8, 8), (33, 9), (200, 120), (256, 256), (257, 255), (520, 264)]


@pytest.mark.parametrize("fmt", FAMILY, ids=[pkm.name_of(f) for f in FAMILY])
def test_photographs_of_eight_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    cases = [(w, h, 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    order = pkm.ORDER_NAMES[fmt % 4]  # a byte order per matrix: the orders themselves have a test of their own
    pics = [_packed("photo", w, h, fmt, order, s) for w, h, s in cases]
    wants = [_want("photo", w, h, fmt, s) for w, h, s in cases]
    assert len(set(wants)) == len(SIZES)
    with device.MixedBatch(len(SIZES)) as mb:
        mb.encode(pics)
        _check_on_device(mb, wants)


@pytest.mark.parametrize("fmt", FAMILY, ids=[pkm.name_of(f) for f in FAMILY])
def test_extreme_content_equals_the_reference(fmt):
    from hydrium_amd import device

    kinds = ["random", "zeros", "ones"] + (["out of range"] if ym.LIMITED[pkm.matrix_of(fmt)] else [])
    if "out of range" in kinds:
        y = _planes("out of range", 264, 200, fmt)[0]
        assert ((y < 16) | (y > 235)).all()
    if pkm.filter_of(fmt) == cm.NEAREST:
        rgb = _model("random", 264, 200, fmt)
        assert ((rgb == 0) | (rgb == 255)).any(-1).mean() > 0.5
    with device.MixedBatch(len(kinds)) as mb:
        mb.encode([_packed(k, 264, 200, fmt) for k in kinds])
        _check(mb, [_want(k, 264, 200, fmt) for k in kinds])


# ---- the loaders ----
@pytest.mark.parametrize("fmt,order", [(YUY2, "yuyv"), (YUY2C, "uyvy")], ids=["yuy2-yuyv", "yuy2c-uyvy"])
def test_the_dword_loader_and_the_byte_loader_give_one_file(fmt, order):
    """200 x 120 random bytes placed so that the dword path applies and so that it does not"""
    from hydrium_amd import device

    w, h = 200, 120
    rows, want = _rows("random", w, h, fmt, order, 77), _want("random", w, h, fmt, 77)
    placed = {
        "aligned": _place(rows, order, 400),
        "base + 1": _place(rows, order, 400, shift=1),
        "base + 2": _place(rows, order, 400, shift=2),
        "base + 3": _place(rows, order, 400, shift=3),
        "odd pitch": _place(rows, order, 403),
        "pitch a multiple of 4, larger than the row": _place(rows, order, 432),
        "negative pitch": _place(rows, order, 400, flip=True),
    }
    group = lambda p: (p[1][0] - pkm.y_offset(order)) % 4  # where the first group starts
    assert [group(placed[k]) for k in ("aligned", "base + 1", "base + 2", "base + 3", "negative pitch")] == [0, 1, 2, 3, 0]
    assert placed["odd pitch"][2] % 2 == 1 and placed["negative pitch"][2] == -400
    with device.MixedBatch(len(placed) + 1) as mb:
        mb.encode([(ptrs, rs, 2, w, h) for _, ptrs, rs in placed.values()] + [_packed("random", w, h, fmt, order, 77)], sample_fmt=fmt)
        _check(mb, [want] * (len(placed) + 1))
    del placed


# ---- byte orders ----
@pytest.mark.parametrize("fmt", [YUY2, YUY2C_JPEG, YUY2L], ids=[pkm.name_of(f) for f in (YUY2, YUY2C_JPEG, YUY2L)])
def test_the_four_byte_orders_of_the_same_planes_give_one_file(fmt):
    from hydrium_amd import device

    w, h = 232, 188
    want = _want("random chroma", w, h, fmt, 21)
    pics = [_packed("random chroma", w, h, fmt, order, 21) for order in pkm.ORDER_NAMES]
    assert len({bytes(_rows("random chroma", w, h, fmt, order, 21)) for order in pkm.ORDER_NAMES}) == 4
    # U and V swapped under the same order (YUYV bytes read as YVYU): the model with the planes swapped, and another file
    y, u, v = _planes("random chroma", w, h, fmt, 21)
    swapped = _reference_of(("packed swapped", fmt), plm.expected_rgb((y, v, u), pkm.matrix_of(fmt), plm.S422, pkm.filter_of(fmt)))
    assert swapped != want
    yuyv = pics[0]
    base = yuyv.surface.data_ptr()
    with device.MixedBatch(5) as mb:  # pictures of different byte orders in one launch group
        mb.encode(pics + [(_pointers(base, "yvyu"), yuyv.pitch, 2, w, h)], sample_fmt=fmt)
        _check(mb, [want] * 4 + [swapped])
        mb.encode(pics[::-1], sample_fmts="each")  # hydamd_encode_mixed_formats
        _check(mb, [want] * 4)


def test_the_file_is_the_one_the_library_writes_for_the_same_planes_as_i422():
    """per filter, in one batch"""
    from hydrium_amd import device

    w, h = 264, 200
    fmts = [8195, 8211, 8227]
    pics = [_packed("photo", w, h, f, "uyvy", 61) for f in fmts] + [_planar8("photo", w, h, pkm.as_i422(f), 61) for f in fmts]
    assert [p.sample_fmt for p in pics[3:]] == [519, 535, 551]
    with device.MixedBatch(6) as mb:
        mb.encode(pics, sample_fmts="each")
        files = [bytes(f) for f in mb.read()]
    assert files[:3] == files[3:] and len(set(files)) == 3
    assert files[:3] == [_want("photo", w, h, f, 61) for f in fmts]


# ---- entry points ----
def test_encode_image_and_a_frame_batch_of_three_frames():
    import torch
    from hydrium_amd import device

    w, h = 264, 200
    for fmt, order in ((YUY2, "yvyu"), (YUY2C_JPEG, "yuyv"), (YUY2L, "uyvy")):
        pics = [_packed("photo", w, h, fmt, order, s) for s in (11, 12, 13)]
        wants = [_want("photo", w, h, fmt, s) for s in (11, 12, 13)]
        with device.FrameBatch(w, h, 3) as fb:
            fb.encode(pics)
            _check(fb, wants)
        with device.DeviceContext(0, 1, 0) as ctx:
            assert ctx.encode_image_tensor(pics[0]) == 1
            got = _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), 1)
            assert got == wants[0]
            p = pics[1]
            ctx.encode_image(p.pointers(), p.pitch, p.pixel_stride, fmt, w, h)
            assert _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), 1) == wants[1]
    torch.cuda.synchronize()


def test_packed_beside_every_other_form_in_one_launch():
    """one picture of each of the fifteen forms the transform kernel has an instance for, 27 x 19 with pitches rounded up to a
    dword: an interpolated form's blocks 1 and 2 take the dword window, block 0 (the picture's first chroma column) and block 3
    (ragged, odd width) the edge fill; forward and reversed"""
    import torch
    from hydrium_amd import device

    w, h, pitch = 27, 19, 28
    f16, bf16 = _half("photo", w, h, "float16", 45), _half("photo", w, h, "bfloat16", 46)
    rgb16 = _image("photo", w, h, 16, 43)[0]
    imgs = [_packed("photo", w, h, YUY2, "vyuy", 51), _packed("photo", w, h, YUY2C_JPEG, "yuyv", 52), _packed("photo", 232, 188, YUY2L, "uyvy", 53),
            _planar8("photo", w, h, 512, 35), _planar8("photo", w, h, 528, 36), _nv12("photo", w, h, 17, 37, pitch),
            _nv12i("photo", w, h, 33, 38, pitch), _p016("photo", w, h, 80, 39, pitch), _p016("photo", w, h, 96, 40, pitch),
            _planar16("photo", w, h, 2112, 47), _planar16("photo", w, h, 2196, 48),
            _image("photo", w, h, 8, 42)[0], rgb16 if rgb16.dtype == torch.int16 else rgb16.view(torch.int16),
            _image("photo", w, h, 32, 44)[0], f16[0], bf16[0]]
    wants = [_want("photo", w, h, YUY2, 51), _want("photo", w, h, YUY2C_JPEG, 52), _want("photo", 232, 188, YUY2L, 53),
             _planar8_want("photo", w, h, 512, 35), _planar8_want("photo", w, h, 528, 36), _nv12_want("photo", w, h, 17, 37),
             _nv12i_want("photo", w, h, 33, 38), _p016_want("photo", w, h, 80, 39), _p016_want("photo", w, h, 96, 40),
             _planar16_want("photo", w, h, 2112, 47), _planar16_want("photo", w, h, 2196, 48),
             _reference("photo", w, h, 8, 42), _reference("photo", w, h, 16, 43), _reference("photo", w, h, 32, 44), f16[1], bf16[1]]
    with device.MixedBatch(len(imgs)) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])


# ---- continuity ----
@pytest.mark.parametrize("fmt", [YUY2C, YUY2L], ids=[pkm.name_of(YUY2C), pkm.name_of(YUY2L)])
def test_chroma_is_continuous_across_the_tiles_of_a_tiled_image(fmt):
    from hydrium_amd import device

    w, h = 520, 300
    rows, whole = _rows("random chroma", w, h, fmt, "yuyv", 5), _model("random chroma", w, h, fmt, 5)
    alone = pkm.expected_rgb(rows[:256, :512], "yuyv", 256, pkm.matrix_of(fmt), pkm.filter_of(fmt))
    assert not np.array_equal(alone, whole[:256, :256])  # the first tile alone clamps where the picture reads on
    with device.TiledImage(w, h, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_packed("random chroma", w, h, fmt, "yuyv", 5))
        assert bytes(ti.read()) == _tiled_want("random chroma", w, h, fmt, 5)


@pytest.mark.parametrize("fmt,order", [(YUY2C, "uyvy"), (YUY2L, "yuyv")], ids=["yuy2c-uyvy", "yuy2l-yuyv"])
def test_across_lf_groups_through_lf_group_at(fmt, order):
    """the caller's own loop over hydamd_encode_lf_group_at: two LF groups side by side (4:2:2 has no vertical taps, so a tall
    picture tells nothing)"""
    from hydrium_amd import device

    w, h = 2056, 264
    rows, whole = _rows("random chroma", w, h, fmt, order, 9), _model("random chroma", w, h, fmt, 9)
    first = pkm.expected_rgb(rows[:, :4096], order, 2048, pkm.matrix_of(fmt), pkm.filter_of(fmt))
    assert not np.array_equal(first, whole[:, :2048])
    pic = _packed("random chroma", w, h, fmt, order, 9)
    with device.DeviceContext(0, 2, 0) as ctx:
        ctx.begin_frame(2)
        for tx in range(2):
            ctx.encode_lf_group_at(tx, pic.pointers(), pic.pitch, pic.pixel_stride, fmt, w, h, tx * 2048, 0, min(2048, w - tx * 2048), h, tx)
        ctx.finish_frame(2)
        got = _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), 2)
    want = _want("random chroma", w, h, fmt, 9)
    assert len(got) == len(want) and got == want


def test_sharded_frames_take_nearest_and_refuse_interpolated_chroma():
    from hydrium_amd import device

    w, h = 2056, 264
    with device.MultiFrame((0, 0), w, h) as m:  # two LF groups, one per (aliased) shard
        for fmt, order in ((YUY2C, "uyvy"), (YUY2L, "yuyv")):
            wide = _packed("random chroma", w, h, fmt, order, 9)
            with pytest.raises(device.DeviceError, match="interpolated chroma is not sharded") as e:
                m.encode([wide, wide])
            assert e.value.code == api.HYD_API_ERROR
        for fmt, order in ((YUY2, "vyuy"), (8195, "yuyv")):
            near = _packed("random chroma", w, h, fmt, order, 9)
            m.encode([near, near])
            assert bytes(m.read()) == _want("random chroma", w, h, fmt, 9)


# ---- refusals ----
def test_what_is_no_format_or_no_layout_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    w, h, fmt = 200, 120, YUY2C
    rows, want = _rows("random chroma", w, h, fmt, "yuyv", 31), _want("random chroma", w, h, fmt, 31)
    buf, ptrs, rs = _place(rows, "yuyv", 400)
    y = ptrs[0]
    attempts = [(ptrs, 2, bad, "Invalid Sample Format") for bad in (8191, 8196, 8240, 8256, 12288)]
    attempts += [(ptrs, ps, f, pkm.LAYOUT_MSG) for ps in (1, 4) for f in (YUY2, YUY2C)]
    attempts += [(p, 2, f, pkm.LAYOUT_MSG) for f in (YUY2, YUY2L) for p in ([y, y - 1, y - 3], [y, y + 1, y + 1], [y, y + 40000, y + 80000])]
    with device.MixedBatch(2) as mb, device.FrameBatch(w, h, 2) as fb, device.TiledImage(w, h, 0, 0) as ti, \
            device.DeviceContext(0, 1, 0) as ctx:
        for p, ps, f, message in attempts:
            with pytest.raises(device.DeviceError, match=message) as e:
                mb.encode([(p, rs, ps, w, h)], sample_fmts=[f])
            assert e.value.code == api.HYD_API_ERROR
            with pytest.raises(device.DeviceError, match=message):
                mb.encode([(p, rs, ps, w, h)], sample_fmt=f)
            with pytest.raises(device.DeviceError, match=message):
                fb.encode([p], rs, ps, f)
            with pytest.raises(device.DeviceError, match=message):
                ti.encode(p, rs, ps, f)
            with pytest.raises(device.DeviceError, match=message) as e:
                ctx.encode_image(p, rs, ps, f, w, h)
            assert e.value.code == api.HYD_API_ERROR
            ctx.begin_frame(1)
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group(0, p, rs, ps, f, w, h, 0)
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group_at(0, p, rs, ps, f, w, h, 0, 0, w, h, 0)
            if message != pkm.LAYOUT_MSG:
                with pytest.raises(device.DeviceError):
                    ctx.transform_footprint(f)
        # nothing was enqueued: every object takes the good picture next
        mb.encode([(ptrs, rs, 2, w, h)], sample_fmt=fmt)
        _check(mb, [want])
        fb.encode([ptrs], rs, 2, fmt)
        _check(fb, [want])
        ti.encode(ptrs, rs, 2, fmt)
        tiled = bytes(ti.read())
        ctx.encode_image(ptrs, rs, 2, fmt, w, h)
        assert _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), 1) == want
    assert tiled == _tiled_want("random chroma", w, h, fmt, 31)
    del buf


# ---- the kernel instances ----
def test_the_new_instances_fit_beside_an_entropy_stage_workgroup():
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        for fmt in (YUY2, YUY2C):
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert 0 < lds <= 26 * 1280 and 0 < regs <= 128
