"""GPU: planar YCbCr pictures from device memory (HYDAMD_I420_*, HYDAMD_I422_*, HYDAMD_I444_* and their C / L forms) on every
entry point that reads device pixels.  A pixel is an 8-bit RGB pixel right after the load: every file is compared whole with
what the compiled reference writes for the HYD_UINT8 picture the numpy model of the definition (planar_model.py) makes of the
same planes.  Every plane sits in an allocation that ends with its last sample, or between 0x5A bytes."""
import ctypes as C

import numpy as np
import pytest

import chroma_model as cm
import planar_model as plm
import yuv_model as ym
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_chroma_filters import _frame_of, _nv12 as _nv12i, _want as _nv12i_want
from test_gpu_half_formats import _half
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_p016_formats import _p016, _want as _p016_want
from test_gpu_yuv_formats import _nv12, _want as _nv12_want
from test_planar_formats import check_upsample, hook

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = sorted(plm.FAMILY)
PITCH_MSG = "planar YCbCr wants the chroma planes' pitch in pixel_stride"
I420, I420C, I422C, I420L, I422L, I444 = 512, 528, 532, 547, 551, 523  # what the layout and entry-point tests use
_cache = {}


def _planes(kind, w, h, fmt, seed=1234):
    """host (y, u, v) of one picture, the same planes for every filter of a matrix and subsampling: a photograph made planar,
    or crafted content"""
    from hydrium_amd import synth

    m, sub = plm.matrix_of(fmt), plm.sub_of(fmt)
    key = ("planes", kind, w, h, m, sub, seed)
    if key not in _cache:
        cs = plm.chroma_shape(sub, w, h)
        rng = np.random.default_rng(seed)
        if kind == "photo":
            y, u, v = plm.planes_of_rgb(synth.make_image("photo", w, h, 8, seed), m, sub)
        elif kind == "random":  # most pixels clamp in at least one channel
            y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), cs, cs))
        elif kind == "random chroma":  # smooth luma under random chroma: tells the filters, and every neighbour they read, apart
            y = ((np.add.outer(np.arange(h) * 2, np.arange(w) * 3) // 7 + rng.integers(0, 4, (h, w))) % 256).astype(np.uint8)
            u, v = (rng.integers(64, 192, cs, dtype=np.uint8) for _ in range(2))
        elif kind in ("zeros", "ones"):
            y, u, v = (np.full(s, 0 if kind == "zeros" else 255, np.uint8) for s in ((h, w), cs, cs))
        elif kind == "out of range":  # luma below 16 and above 235, chroma beyond 16 ... 240, around a photograph's chroma
            y, u, v = plm.planes_of_rgb(synth.make_image("photo", w, h, 8, seed), m, sub)
            y = np.where(rng.integers(0, 2, (h, w)) == 0, rng.integers(0, 16, (h, w)), rng.integers(236, 256, (h, w))).astype(np.uint8)
            u, v = u.copy(), v.copy()
            for p in (u, v):
                p[::3] = rng.choice(np.array([0, 5, 15, 241, 250, 255], np.uint8), p[::3].shape)
        else:
            raise KeyError(kind)
        for p in (y, u, v):
            p.setflags(write=False)
        _cache[key] = (y, u, v)
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = plm.expected_rgb(_planes(kind, w, h, fmt, seed), plm.matrix_of(fmt), plm.sub_of(fmt), plm.filter_of(fmt))
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234):
    """the reference's file for the model's RGB8 picture of those planes; made once"""
    return _reference_of(("planar", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed))


def _tiled_want(kind, w, h, fmt, seed=1234):
    from oracle import refprobe

    key = ("tiled", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), _model(kind, w, h, fmt, seed), shift_x=0, shift_y=0)
    return _cache[key]


def _plane_tensor(plane, pitch):
    """one plane in an allocation of its own that ENDS with the plane's last sample, 0x5A in the pitch's slack"""
    import torch

    rows, cols = plane.shape
    host = np.full(pitch * (rows - 1) + cols, 0x5A, np.uint8)
    for r in range(rows):
        host[pitch * r: pitch * r + cols] = plane[r]
    return torch.from_numpy(host).cuda().as_strided((rows, cols), (pitch, 1))


def _planar(kind, w, h, fmt, seed=1234, pitch=None, cpitch=None):
    """device.PlanarYuv of the picture, three allocations; pitches: the plane's width rounded up to a dword, or as given; made once"""
    import torch
    from hydrium_amd import device

    key = ("dev", kind, w, h, fmt, seed, pitch, cpitch)
    if key not in _cache:
        y, u, v = _planes(kind, w, h, fmt, seed)
        yp, cp = pitch or (w + 3) // 4 * 4, cpitch or (u.shape[1] + 3) // 4 * 4
        sub, filt = ("420", "422", "444")[plm.sub_of(fmt)], cm.FILTER_NAMES[plm.filter_of(fmt)]
        _cache[key] = device.PlanarYuv(_plane_tensor(y, yp), _plane_tensor(u, cp), _plane_tensor(v, cp), 16 + plm.matrix_of(fmt), sub, filt)
        assert _cache[key].sample_fmt == fmt
        torch.cuda.synchronize()
    return _cache[key]


def _place(planes, ypitch, cpitch, y_shift=0, u_shift=0, v_shift=0, flip_y=False, flip_c=False, one_buffer=True):
    """the planes at bare addresses: (buffers to keep alive, [Y, U, V addresses], row stride, chroma pitch).  One buffer holds
    Y, then U, then V between 0x5A bytes (shifts move a plane's base by bytes; flips store its rows bottom-up: a negative pitch),
    or every plane has an allocation of its own."""
    import torch

    pitches, shifts, flips = (ypitch, cpitch, cpitch), (y_shift, u_shift, v_shift), (flip_y, flip_c, flip_c)
    spans = [16 + p * (pl.shape[0] + 2) for p, pl in zip(pitches, planes)]
    spans = [(s + 255) // 256 * 256 for s in spans]
    hosts, starts = [], []
    for pl, p, sh, fl, span in zip(planes, pitches, shifts, flips, spans):
        host = np.full(span, 0x5A, np.uint8)
        at = 8 + sh  # (8: a plane starts on a dword when nothing is shifted)
        rows = host[at: at + p * pl.shape[0]].reshape(pl.shape[0], p)
        rows[:, : pl.shape[1]] = pl[::-1] if fl else pl
        hosts.append(host)
        starts.append(at + (pl.shape[0] - 1) * p if fl else at)
    if one_buffer:
        bufs = [torch.from_numpy(np.concatenate(hosts)).cuda()]
        bases = [bufs[0].data_ptr() + sum(spans[:k]) for k in range(3)]
    else:
        bufs = [torch.from_numpy(hst).cuda() for hst in hosts]
        bases = [b.data_ptr() for b in bufs]
    assert all(b % 256 == 0 for b in bases)
    return bufs, [b + s for b, s in zip(bases, starts)], -ypitch if flip_y else ypitch, -cpitch if flip_c else cpitch


# ---- the definition on the device ----
def test_the_device_build_of_the_definition_equals_the_model():
    check_upsample(hook(C.CDLL(hbuild.PROBE_PATH).hydt_planar_upsample_device, 0))


# ---- reference parity ----
SIZES = [(8, 8), (33, 9), (200, 120), (256, 256), (257, 255), (520, 264)]


@pytest.mark.parametrize("fmt", FAMILY, ids=[plm.name_of(f) for f in FAMILY])
def test_photographs_of_six_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    cases = [(w, h, 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    pics = [_planar("photo", w, h, fmt, s) for w, h, s in cases]
    wants = [_want("photo", w, h, fmt, s) for w, h, s in cases]
    assert len(set(wants)) == len(SIZES)
    with device.MixedBatch(len(SIZES)) as mb:
        mb.encode(pics)
        _check_on_device(mb, wants)


@pytest.mark.parametrize("fmt", FAMILY, ids=[plm.name_of(f) for f in FAMILY])
def test_extreme_content_equals_the_reference(fmt):
    from hydrium_amd import device

    kinds = ["random", "zeros", "ones"] + (["out of range"] if ym.LIMITED[plm.matrix_of(fmt)] else [])
    if "out of range" in kinds:
        y = _planes("out of range", 264, 200, fmt)[0]
        assert ((y < 16) | (y > 235)).all()
    if plm.filter_of(fmt) == cm.NEAREST:
        rgb = _model("random", 264, 200, fmt)
        assert ((rgb == 0) | (rgb == 255)).any(-1).mean() > 0.5
    with device.MixedBatch(len(kinds)) as mb:
        mb.encode([_planar(k, 264, 200, fmt) for k in kinds])
        _check(mb, [_want(k, 264, 200, fmt) for k in kinds])


# ---- the loaders ----
@pytest.mark.parametrize("fmt", [I420, I420C, I422L, I444], ids=[plm.name_of(f) for f in (I420, I420C, I422L, I444)])
def test_the_dword_loader_and_the_byte_loader_give_one_file(fmt):
    """200 x 120 random planes placed so that the dword runs apply and so that they do not"""
    from hydrium_amd import device

    w, h = 200, 120
    planes, want = _planes("random", w, h, fmt, 77), _want("random", w, h, fmt, 77)
    cw = planes[1].shape[1]
    cp = (cw + 3) // 4 * 4
    placed = {
        "aligned": _place(planes, 200, cp),
        "Y base + 1": _place(planes, 200, cp, y_shift=1),
        "U base + 1, V base + 2": _place(planes, 200, cp, u_shift=1, v_shift=2),
        "chroma pitch odd": _place(planes, 200, cw + 3 if (cw + 3) % 2 else cw + 1),
        "chroma pitch not half the Y pitch": _place(planes, 208, cp + 24),
        "both pitches negative": _place(planes, 200, cp, flip_y=True, flip_c=True),
        "Y negative only": _place(planes, 200, cp, flip_y=True),
        "chroma negative only": _place(planes, 200, cp, flip_c=True),
        "separate allocations": _place(planes, 200, cp, one_buffer=False),
    }
    assert all(p % 4 == 0 for p in placed["aligned"][1]) and placed["Y base + 1"][1][0] % 4 == 1
    assert [p % 4 for p in placed["U base + 1, V base + 2"][1]] == [0, 1, 2] and placed["chroma pitch odd"][3] % 2 == 1
    assert placed["both pitches negative"][2:] == (-200, -cp) and placed["Y negative only"][2:] == (-200, cp)
    with device.MixedBatch(len(placed) + 1) as mb:
        mb.encode([(ptrs, rs, ps, w, h) for _, ptrs, rs, ps in placed.values()] + [_planar("random", w, h, fmt, 77)], sample_fmt=fmt)
        _check(mb, [want] * (len(placed) + 1))
        # U and V swapped (YV12): the model with its planes swapped, and another file
        swapped = _reference_of(("planar swapped", fmt), plm.expected_rgb((planes[0], planes[2], planes[1]), plm.matrix_of(fmt), plm.sub_of(fmt), plm.filter_of(fmt)))
        assert swapped != want
        _, ptrs, rs, ps = placed["separate allocations"]
        mb.encode([([ptrs[0], ptrs[2], ptrs[1]], rs, ps, w, h)], sample_fmt=fmt)
        _check(mb, [swapped])
    del placed


# ---- entry points ----
def test_encode_image_and_a_frame_batch_of_three_frames():
    import torch
    from hydrium_amd import device

    w, h = 264, 200
    for fmt in (I420C, I422L, I444):
        pics = [_planar("photo", w, h, fmt, s) for s in (11, 12, 13)]
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


def test_planar_beside_nv12_p010_and_rgb8_in_one_launch():
    """and, in the same round, one picture of each of the eleven forms the transform kernel has an instance for, 27 x 19 with
    pitches rounded up to a dword: an interpolated form's blocks 1 and 2 take the dword window, block 0 (the picture's first
    chroma column) and block 3 (ragged, odd width) the edge fill"""
    import torch
    from hydrium_amd import device

    imgs = [_planar("photo", 232, 188, I420C, 31), _planar("photo", 200, 120, I444, 32), _nv12("photo", 232, 188, 17, 33),
            _p016("photo", 200, 120, 80, 34), torch.from_numpy(_model("photo", 232, 188, I420C, 31)).cuda()]
    wants = [_want("photo", 232, 188, I420C, 31), _want("photo", 200, 120, I444, 32), _nv12_want("photo", 232, 188, 17, 33),
             _p016_want("photo", 200, 120, 80, 34), _want("photo", 232, 188, I420C, 31)]
    w, h, pitch = 27, 19, 28
    f16, bf16 = _half("photo", w, h, "float16", 45), _half("photo", w, h, "bfloat16", 46)
    rgb16 = _image("photo", w, h, 16, 43)[0]
    imgs += [_planar("photo", w, h, I420, 35), _planar("photo", w, h, I420C, 36), _nv12("photo", w, h, 17, 37, pitch),
             _nv12i("photo", w, h, 33, 38, pitch), _p016("photo", w, h, 80, 39, pitch), _p016("photo", w, h, 96, 40, pitch),
             _image("photo", w, h, 8, 42)[0], rgb16 if rgb16.dtype == torch.int16 else rgb16.view(torch.int16),
             _image("photo", w, h, 32, 44)[0], f16[0], bf16[0]]
    wants += [_want("photo", w, h, I420, 35), _want("photo", w, h, I420C, 36), _nv12_want("photo", w, h, 17, 37),
              _nv12i_want("photo", w, h, 33, 38), _p016_want("photo", w, h, 80, 39), _p016_want("photo", w, h, 96, 40),
              _reference("photo", w, h, 8, 42), _reference("photo", w, h, 16, 43), _reference("photo", w, h, 32, 44), f16[1], bf16[1]]
    with device.MixedBatch(len(imgs)) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])


@pytest.mark.parametrize("fmt", [I420C, I422C], ids=[plm.name_of(I420C), plm.name_of(I422C)])
def test_chroma_is_continuous_across_the_tiles_of_a_tiled_image(fmt):
    from hydrium_amd import device

    w, h = 520, 300
    planes, whole = _planes("random chroma", w, h, fmt, 5), _model("random chroma", w, h, fmt, 5)
    sub = plm.sub_of(fmt)
    sx, sy = plm.shifts(sub)
    alone = plm.expected_rgb((planes[0][:256, :256], planes[1][:256 >> sy, :256 >> sx], planes[2][:256 >> sy, :256 >> sx]), plm.matrix_of(fmt), sub, plm.filter_of(fmt))
    assert not np.array_equal(alone, whole[:256, :256])  # the first tile alone clamps where the picture reads on
    with device.TiledImage(w, h, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_planar("random chroma", w, h, fmt, 5))
        assert bytes(ti.read()) == _tiled_want("random chroma", w, h, fmt, 5)


WIDE = [(2056, 264), (264, 2056)]
WIDE_CASES = [(w, h, fmt) for fmt in (I420C, I420L, I422C, I422L) for w, h in WIDE]


@pytest.mark.parametrize("w,h,fmt", WIDE_CASES, ids=[f"{w}x{h}-{plm.name_of(f)}" for w, h, f in WIDE_CASES])
def test_across_lf_groups_through_lf_group_at(w, h, fmt):
    """the caller's own loop over hydamd_encode_lf_group_at: two LF groups side by side, or one above the other"""
    from hydrium_amd import device

    planes, whole = _planes("random chroma", w, h, fmt, 9), _model("random chroma", w, h, fmt, 9)
    if w > 2048:  # (4:2:2 has no vertical taps: only the side-by-side picture tells its LF groups apart)
        sx, sy = plm.shifts(plm.sub_of(fmt))
        first = (planes[0][:2048, :2048], planes[1][:2048 >> sy, :2048 >> sx], planes[2][:2048 >> sy, :2048 >> sx])
        assert not np.array_equal(plm.expected_rgb(first, plm.matrix_of(fmt), plm.sub_of(fmt), plm.filter_of(fmt)), whole[:2048, :2048])
    pic = _planar("random chroma", w, h, fmt, 9)
    lfx, lfy = -(-w // 2048), -(-h // 2048)
    with device.DeviceContext(0, lfx * lfy, 0) as ctx:
        ctx.begin_frame(lfx * lfy)
        for ty in range(lfy):
            for tx in range(lfx):
                ctx.encode_lf_group_at(ty * lfx + tx, pic.pointers(), pic.pitch, pic.pixel_stride, fmt, w, h, tx * 2048, ty * 2048,
                                       min(2048, w - tx * 2048), min(2048, h - ty * 2048), ty * lfx + tx)
        ctx.finish_frame(lfx * lfy)
        got = _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), lfx * lfy)
    want = _want("random chroma", w, h, fmt, 9)
    assert len(got) == len(want) and got == want


def test_sharded_frames_take_nearest_and_refuse_interpolated_chroma():
    from hydrium_amd import device

    w, h = 2056, 264
    with device.MultiFrame((0, 0), w, h) as m:  # two LF groups, one per (aliased) shard
        for fmt in (I420C, I422L):
            wide = _planar("random chroma", w, h, fmt, 9)
            with pytest.raises(device.DeviceError, match="interpolated chroma is not sharded") as e:
                m.encode([wide, wide])
            assert e.value.code == api.HYD_API_ERROR
        for fmt in (I420, 517, I444):
            near = _planar("random chroma", w, h, fmt, 9)
            m.encode([near, near])
            assert bytes(m.read()) == _want("random chroma", w, h, fmt, 9)


# ---- refusals ----
def test_what_is_no_format_or_no_pitch_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    w, h, fmt = 200, 120, I420C
    planes, want = _planes("random chroma", w, h, fmt, 31), _want("random chroma", w, h, fmt, 31)
    bufs, ptrs, rs, cp = _place(planes, 200, 100)
    attempts = [(cp, bad, "Invalid Sample Format") for bad in (524, 527, 536, 552, 576, 1024)]
    attempts += [(1, f, PITCH_MSG) for f in (I420, I420C, I422L, I444)] + [(-99, I420C, PITCH_MSG), (199, I444, PITCH_MSG)]
    with device.MixedBatch(2) as mb, device.FrameBatch(w, h, 2) as fb, device.TiledImage(w, h, 0, 0) as ti, \
            device.DeviceContext(0, 1, 0) as ctx:
        for ps, f, message in attempts:
            with pytest.raises(device.DeviceError, match=message) as e:
                mb.encode([(ptrs, rs, ps, w, h)], sample_fmts=[f])
            assert e.value.code == api.HYD_API_ERROR
            with pytest.raises(device.DeviceError, match=message):
                mb.encode([(ptrs, rs, ps, w, h)], sample_fmt=f)
            with pytest.raises(device.DeviceError, match=message):
                fb.encode([ptrs], rs, ps, f)
            with pytest.raises(device.DeviceError, match=message):
                ti.encode(ptrs, rs, ps, f)
            with pytest.raises(device.DeviceError, match=message) as e:
                ctx.encode_image(ptrs, rs, ps, f, w, h)
            assert e.value.code == api.HYD_API_ERROR
            ctx.begin_frame(1)
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group(0, ptrs, rs, ps, f, w, h, 0)
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group_at(0, ptrs, rs, ps, f, w, h, 0, 0, w, h, 0)
            if message != PITCH_MSG:
                with pytest.raises(device.DeviceError):
                    ctx.transform_footprint(f)
        # nothing was enqueued: every object takes the good picture next
        mb.encode([(ptrs, rs, cp, w, h)], sample_fmt=fmt)
        _check(mb, [want])
        fb.encode([ptrs], rs, cp, fmt)
        _check(fb, [want])
        ti.encode(ptrs, rs, cp, fmt)
        tiled = bytes(ti.read())
        ctx.encode_image(ptrs, rs, cp, fmt, w, h)
        assert _frame_of(ctx, api.HYDImageMetadata(w, h, 0, -1, -1), 1) == want
    assert tiled == _tiled_want("random chroma", w, h, fmt, 31)
    del bufs


# ---- the kernel instances ----
def test_the_new_instances_fit_beside_an_entropy_stage_workgroup():
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        for fmt in (I420, I420C, I422L, I444):
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert 0 < lds <= 26 * 1280 and 0 < regs <= 128
