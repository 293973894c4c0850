"""GPU: planar YCbCr pictures of 16-bit words from device memory (HYDAMD_I010_* ... HYDAMD_I416_* and their C / L forms) on every
entry point that reads device pixels.  A pixel is a 16-bit RGB pixel right after the load: every file is compared whole with
what the compiled reference writes for the HYD_UINT16 picture the numpy model of the definition (planar16_model.py) makes of the
same planes.  Every plane sits in an allocation that ends with its last sample, or between 0x5A5A words."""
import ctypes as C

import numpy as np
import pytest

import chroma_model as cm
import planar16_model as m16
import planar_model as plm
import yuv_model as ym
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_chroma_filters import _frame_of
from test_gpu_half_formats import _half
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_p016_formats import _p016, _want as _p016_want
from test_gpu_planar_formats import _planar as _planar8, _want as _planar8_want
from test_gpu_yuv_formats import _nv12, _want as _nv12_want
from test_planar16_formats import check_definition, hook

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = sorted(m16.FAMILY)
PITCH_MSG = "planar YCbCr wants the chroma planes' pitch in pixel_stride"
ALIGN_MSG = "planar YCbCr of 16-bit words wants its three planes on 2-byte boundaries"
SHARDED_MSG = "interpolated chroma is not sharded"
I010, I010C, I212L, I416 = 2112, 2129, 2215, 2251  # nearest 4:2:0, centre 4:2:0, left 4:2:2, 4:4:4: what the layout tests use
I210C, I016L = 2133, 2274
NO_FORMAT = (2048, 2111, 2124, 2152, 2280, 4096)
# the share of random 16-bit words that have a bit set above depth n: 1 - 2^-(16 - n), 63/64 and 15/16; asserted with 1 % to spare
UNMASKED_SHARE = {1: 63 / 64 - 0.01, 2: 15 / 16 - 0.01}
_cache = {}


def _planes(kind, w, h, fmt, seed=1234):
    """host (y, u, v) uint16 of one picture, the same planes for every filter of a depth, matrix and subsampling"""
    from hydrium_amd import synth

    d, m, sub = m16.depth_of(fmt), m16.matrix_of(fmt), m16.sub_of(fmt)
    key = ("planes", kind, w, h, d, m, sub, seed)
    if key not in _cache:
        n = m16.BITS[d]
        cs = plm.chroma_shape(sub, w, h)
        rng = np.random.default_rng(seed)
        photo = lambda: m16.planes_of_rgb(synth.make_image("photo", w, h, 16, seed), d, m, sub)
        if kind == "photo":  # valid n-bit codes
            y, u, v = photo()
        elif kind == "random":  # random n-bit codes: most pixels clamp in at least one channel
            y, u, v = (rng.integers(0, 1 << n, s, dtype=np.uint16) for s in ((h, w), cs, cs))
        elif kind == "random words":  # full 16-bit words whatever the depth: bits above the depth are set in most
            y, u, v = (rng.integers(0, 65536, s, dtype=np.uint16) for s in ((h, w), cs, cs))
        elif kind == "masked words":  # the same words with only their n bits
            y, u, v = (p & ((1 << n) - 1) for p in _planes("random words", w, h, fmt, seed))
        elif kind == "random chroma":  # smooth luma under random chroma: tells the filters, and every neighbour they read, apart
            y = (((np.add.outer(np.arange(h) * 2, np.arange(w) * 3) // 7 + rng.integers(0, 4, (h, w))) % 256) << (n - 8)).astype(np.uint16)
            u, v = (rng.integers(1 << (n - 2), 3 << (n - 2), cs, dtype=np.uint16) for _ in range(2))
        elif kind in ("zeros", "ones"):  # ones: all-ones in n bits
            y, u, v = (np.full(s, 0 if kind == "zeros" else (1 << n) - 1, np.uint16) for s in ((h, w), cs, cs))
        elif kind == "out of range":  # luma below 16 and above 235, chroma beyond 16 ... 240 (at 8 bits), around a photograph's chroma
            y, u, v = photo()
            unit = 1 << (n - 8)
            y = np.where(rng.integers(0, 2, (h, w)) == 0, rng.integers(0, 16 * unit, (h, w)), rng.integers(236 * unit, 256 * unit, (h, w))).astype(np.uint16)
            u, v = u.copy(), v.copy()
            for p in (u, v):
                p[::3] = rng.choice(np.array([0, 5 * unit, 16 * unit - 1, 240 * unit + 1, 250 * unit, 256 * unit - 1], np.uint16), p[::3].shape)
        else:
            raise KeyError(kind)
        y, u, v = (np.ascontiguousarray(p, np.uint16) for p in (y, u, v))
        for p in (y, u, v):
            p.setflags(write=False)
        _cache[key] = (y, u, v)
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = m16.expected_rgb(_planes(kind, w, h, fmt, seed), fmt)
        _cache[key].setflags(write=False)
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234):
    """the reference's file for the model's RGB16 picture of those planes; made once"""
    return _reference_of(("planar16", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed))


def _tiled_want(kind, w, h, fmt, seed=1234):
    from oracle import refprobe

    key = ("tiled", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), _model(kind, w, h, fmt, seed), shift_x=0, shift_y=0)
    return _cache[key]


def _plane_tensor(plane, pitch):
    """one plane in an allocation of its own that ENDS with the plane's last word, 0x5A5A in the pitch's slack"""
    import torch

    rows, cols = plane.shape
    host = np.full(pitch * (rows - 1) + cols, 0x5A5A, np.uint16)
    for r in range(rows):
        host[pitch * r: pitch * r + cols] = plane[r]
    return torch.from_numpy(host.view(np.int16)).cuda().as_strided((rows, cols), (pitch, 1))


def _device_picture(planes, fmt, pitch=None, cpitch=None):
    from hydrium_amd import device

    y, u, v = planes
    yp, cp = pitch or (y.shape[1] + 1) // 2 * 2, cpitch or (u.shape[1] + 1) // 2 * 2  # rounded up to a dword
    sub, filt = ("420", "422", "444")[m16.sub_of(fmt)], cm.FILTER_NAMES[m16.filter_of(fmt)]
    pic = device.PlanarYuv16(_plane_tensor(y, yp), _plane_tensor(u, cp), _plane_tensor(v, cp), 16 + m16.matrix_of(fmt), sub, filt, m16.bits_of(fmt))
    assert pic.sample_fmt == fmt
    return pic


def _planar(kind, w, h, fmt, seed=1234, pitch=None, cpitch=None):
    """device.PlanarYuv16 of the picture, three allocations; made once"""
    import torch

    key = ("dev", kind, w, h, fmt, seed, pitch, cpitch)
    if key not in _cache:
        _cache[key] = _device_picture(_planes(kind, w, h, fmt, seed), fmt, pitch, cpitch)
        torch.cuda.synchronize()
    return _cache[key]


def _place(planes, ypitch, cpitch, y_shift=0, u_shift=0, v_shift=0, flip_y=False, flip_c=False, one_buffer=True):
    """the planes at bare addresses: (buffers to keep alive, [Y, U, V addresses], row stride, chroma pitch), pitches in WORDS.  One
    buffer holds Y, then U, then V between 0x5A5A words (shifts move a plane's base by BYTES, even; flips store its rows bottom-up:
    a negative pitch), or every plane has an allocation of its own."""
    import torch

    pitches, shifts, flips = (ypitch, cpitch, cpitch), (y_shift, u_shift, v_shift), (flip_y, flip_c, flip_c)
    assert all(s % 2 == 0 for s in shifts)
    spans = [(16 + p * (pl.shape[0] + 2) + 127) // 128 * 128 for p, pl in zip(pitches, planes)]  # in words: 256-byte multiples
    hosts, starts = [], []
    for pl, p, sh, fl, span in zip(planes, pitches, shifts, flips, spans):
        host = np.full(span, 0x5A5A, np.uint16)
        at = 8 + sh // 2  # (8 words: a plane starts on a dword when nothing is shifted)
        rows = host[at: at + p * pl.shape[0]].reshape(pl.shape[0], p)
        rows[:, : pl.shape[1]] = pl[::-1] if fl else pl
        hosts.append(host)
        starts.append(at + (pl.shape[0] - 1) * p if fl else at)
    if one_buffer:
        bufs = [torch.from_numpy(np.concatenate(hosts).view(np.int16)).cuda()]
        bases = [bufs[0].data_ptr() + 2 * sum(spans[:k]) for k in range(3)]
    else:
        bufs = [torch.from_numpy(hst.view(np.int16)).cuda() for hst in hosts]
        bases = [b.data_ptr() for b in bufs]
    assert all(b % 256 == 0 for b in bases)
    return bufs, [b + 2 * s for b, s in zip(bases, starts)], -ypitch if flip_y else ypitch, -cpitch if flip_c else cpitch


# ---- the definition on the device ----
def test_the_device_build_of_the_definition_equals_the_model():
    check_definition(hook(C.CDLL(hbuild.PROBE_PATH).hydt_planar16_to_rgb_device, 0))


# ---- reference parity ----
SIZES = [(8, 8), (33, 9), (200, 120), (256, 256), (257, 255), (520, 264)]


@pytest.mark.parametrize("fmt", FAMILY, ids=[m16.name_of(f) for f in FAMILY])
def test_photographs_of_six_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    cases = [(w, h, 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    n = m16.bits_of(fmt)
    assert all(max(int(p.max()) for p in _planes("photo", w, h, fmt, s)) < 1 << n for w, h, s in cases)  # valid n-bit codes
    pics = [_planar("photo", w, h, fmt, s) for w, h, s in cases]
    wants = [_want("photo", w, h, fmt, s) for w, h, s in cases]
    assert len(set(wants)) == len(SIZES)
    with device.MixedBatch(len(SIZES)) as mb:
        mb.encode(pics)
        _check_on_device(mb, wants)


@pytest.mark.parametrize("fmt", FAMILY, ids=[m16.name_of(f) for f in FAMILY])
def test_extreme_content_equals_the_reference(fmt):
    from hydrium_amd import device

    w, h, d = 264, 200, m16.depth_of(fmt)
    kinds = ["zeros", "ones", "random"] + (["out of range"] if ym.LIMITED[m16.matrix_of(fmt)] else [])
    if "out of range" in kinds:
        y, unit = _planes("out of range", w, h, fmt)[0], 1 << (m16.bits_of(fmt) - 8)
        assert ((y < 16 * unit) | (y > 235 * unit)).all()
    pics, wants = [_planar(k, w, h, fmt) for k in kinds], [_want(k, w, h, fmt) for k in kinds]
    if d in UNMASKED_SHARE:
        # random full 16-bit words: the file of the same words masked to n bits, although most words differ
        raw, masked = _planes("random words", w, h, fmt), _planes("masked words", w, h, fmt)
        share = sum(int((a != b).sum()) for a, b in zip(raw, masked)) / sum(a.size for a in raw)
        assert share > UNMASKED_SHARE[d], share
        pics += [_planar("random words", w, h, fmt), _planar("masked words", w, h, fmt)]
        wants += [_want("masked words", w, h, fmt)] * 2
    with device.MixedBatch(len(pics)) as mb:
        mb.encode(pics)
        _check(mb, wants)


# ---- the loaders ----
@pytest.mark.parametrize("fmt", [I010, I010C, I212L, I416], ids=[m16.name_of(f) for f in (I010, I010C, I212L, I416)])
def test_the_dword_loader_and_the_sample_loader_give_one_file(fmt):
    """200 x 120 random planes placed so that the dword windows apply and so that they do not"""
    from hydrium_amd import device

    w, h = 200, 120
    kind = "random words" if m16.depth_of(fmt) < 3 else "random"
    planes, want = _planes(kind, w, h, fmt, 77), _want(kind, w, h, fmt, 77)
    cw = planes[1].shape[1]
    cp = (cw + 1) // 2 * 2
    placed = {
        "aligned": _place(planes, 200, cp),
        "Y base + 2 bytes": _place(planes, 200, cp, y_shift=2),
        "U base + 2, V base + 6": _place(planes, 200, cp, u_shift=2, v_shift=6),
        "chroma pitch odd": _place(planes, 200, cp + 1),
        "Y pitch odd": _place(planes, 201, cp),
        "chroma pitch not half the Y pitch": _place(planes, 208, cp + 24),
        "both pitches negative": _place(planes, 200, cp, flip_y=True, flip_c=True),
        "Y negative only": _place(planes, 200, cp, flip_y=True),
        "chroma negative only": _place(planes, 200, cp, flip_c=True),
        "separate allocations": _place(planes, 200, cp, one_buffer=False),
    }
    assert all(p % 4 == 0 for p in placed["aligned"][1]) and placed["Y base + 2 bytes"][1][0] % 4 == 2
    assert [p % 4 for p in placed["U base + 2, V base + 6"][1]] == [0, 2, 2] and placed["chroma pitch odd"][3] % 2 == 1
    assert placed["both pitches negative"][2:] == (-200, -cp) and placed["Y negative only"][2:] == (-200, cp)
    with device.MixedBatch(len(placed) + 1) as mb:
        mb.encode([(ptrs, rs, ps, w, h) for _, ptrs, rs, ps in placed.values()] + [_planar(kind, w, h, fmt, 77)], sample_fmt=fmt)
        _check(mb, [want] * (len(placed) + 1))
    del placed


# ---- picture semantics ----
@pytest.mark.parametrize("w,h,fmt", [(520, 264, I010C), (520, 264, I212L), (2056, 264, I016L)],
                         ids=["520x264-i010c", "520x264-i212l", "2056x264-i016l"])
def test_the_lf_groups_of_a_picture_through_lf_group_at_give_the_whole_pictures_file(w, h, fmt):
    from hydrium_amd import device

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


def test_a_crop_clamps_at_its_own_edges():
    """a 200 x 120 crop at (64, 32) of a 520 x 264 surface is a picture: its edges replicate although real neighbours exist"""
    from hydrium_amd import device

    w, h, x0, y0, cw_, ch_ = 520, 264, 64, 32, 200, 120
    for fmt in (I010C, I212L):
        y, u, v = _planes("random chroma", w, h, fmt, 5)
        sx, sy = plm.shifts(m16.sub_of(fmt))
        crop = (y[y0:y0 + ch_, x0:x0 + cw_], u[y0 >> sy:(y0 + ch_) >> sy, x0 >> sx:(x0 + cw_) >> sx], v[y0 >> sy:(y0 + ch_) >> sy, x0 >> sx:(x0 + cw_) >> sx])
        alone = m16.expected_rgb(crop, fmt)
        assert not np.array_equal(alone, _model("random chroma", w, h, fmt, 5)[y0:y0 + ch_, x0:x0 + cw_])
        whole = _planar("random chroma", w, h, fmt, 5)
        sub, filt = ("420", "422", "444")[m16.sub_of(fmt)], cm.FILTER_NAMES[m16.filter_of(fmt)]
        view = device.PlanarYuv16(whole.y[y0:y0 + ch_, x0:x0 + cw_], whole.u[y0 >> sy:(y0 + ch_) >> sy, x0 >> sx:(x0 + cw_) >> sx],
                                  whole.v[y0 >> sy:(y0 + ch_) >> sy, x0 >> sx:(x0 + cw_) >> sx], 16 + m16.matrix_of(fmt), sub, filt, m16.bits_of(fmt))
        with device.MixedBatch(1) as mb:
            mb.encode([view])
            _check(mb, [_reference_of(("planar16 crop", fmt), alone)])


@pytest.mark.parametrize("fmt", [I010C, I210C], ids=[m16.name_of(I010C), m16.name_of(I210C)])
def test_chroma_is_continuous_across_the_tiles_of_a_tiled_image(fmt):
    from hydrium_amd import device

    w, h = 520, 264
    planes, whole = _planes("random chroma", w, h, fmt, 5), _model("random chroma", w, h, fmt, 5)
    sx, sy = plm.shifts(m16.sub_of(fmt))
    alone = m16.expected_rgb((planes[0][:256, :256], planes[1][:256 >> sy, :256 >> sx], planes[2][:256 >> sy, :256 >> sx]), fmt)
    assert not np.array_equal(alone, whole[:256, :256])  # the first tile alone clamps where the picture reads on
    with device.TiledImage(w, h, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_planar("random chroma", w, h, fmt, 5))
        assert bytes(ti.read()) == _tiled_want("random chroma", w, h, fmt, 5)


# ---- beside the other families ----
def test_one_launch_group_holds_every_family():
    import torch
    from hydrium_amd import device

    rgb16 = _image("photo", 200, 120, 16, 43)[0]
    f16 = _half("photo", 27, 19, "float16", 45)
    imgs = [_planar("photo", 232, 188, I010C, 31), _p016("photo", 200, 120, 80, 34), _planar8("photo", 200, 120, 512, 32),
            _nv12("photo", 232, 188, 17, 33), rgb16 if rgb16.dtype == torch.int16 else rgb16.view(torch.int16),
            _image("photo", 27, 19, 8, 42)[0], f16[0], _planar("photo", 27, 19, I416, 36), _planar("photo", 27, 19, I212L, 37)]
    wants = [_want("photo", 232, 188, I010C, 31), _p016_want("photo", 200, 120, 80, 34), _planar8_want("photo", 200, 120, 512, 32),
             _nv12_want("photo", 232, 188, 17, 33), _reference("photo", 200, 120, 16, 43), _reference("photo", 27, 19, 8, 42), f16[1],
             _want("photo", 27, 19, I416, 36), _want("photo", 27, 19, I212L, 37)]
    with device.MixedBatch(len(imgs)) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])


def test_i010_is_the_p010_picture_of_the_shifted_interleaved_planes_on_the_card():
    import torch
    from hydrium_amd import device

    w, h = 200, 120
    for fmt, p_fmt in ((2112, 80), (2129, 97), (2210, 178)):  # I010 / P010, I010C / P010C full range, I012L / P012L BT.601
        y, u, v = _planes("random", w, h, fmt, 21)
        d = m16.depth_of(fmt)
        host = np.full(w * (h + h // 2), 0x5A5A, np.uint16)
        host[: w * h] = m16.samples(d, y).reshape(-1)
        host[w * h:] = m16.interleave(m16.samples(d, u), m16.samples(d, v)).reshape(-1)
        p01x = device.P016.from_surface(torch.from_numpy(host.view(np.int16)).cuda(), w, h, 2 * w, 2 * w * h, p_fmt)
        with device.MixedBatch(2) as mb:
            mb.encode([_planar("random", w, h, fmt, 21), p01x], sample_fmts="each")
            files = [bytes(f) for f in mb.read()]
        assert files[0] == files[1] == _want("random", w, h, fmt, 21)


def test_sharded_frames_take_nearest_and_refuse_interpolated_chroma():
    from hydrium_amd import device

    w, h = 2056, 264
    with device.MultiFrame((0, 0), w, h) as m:  # two LF groups, one per (aliased) shard
        for fmt in (I010C, I212L):
            wide = _planar("random chroma", w, h, fmt, 9)
            with pytest.raises(device.DeviceError, match=SHARDED_MSG) as e:
                m.encode([wide, wide])
            assert e.value.code == api.HYD_API_ERROR
        near = _planar("random chroma", w, h, I010, 9)
        both = (C.c_void_p * 6)(*(near.pointers() * 2))
        for bad in NO_FORMAT:  # nothing is enqueued: the frames below are the next thing the object sees
            with pytest.raises(device.DeviceError, match="Invalid Sample Format") as e:
                m._ck(m.d.hydamd_encode_image_multi(m.h, both, near.pitch, near.pixel_stride, bad, 0))
            assert e.value.code == api.HYD_API_ERROR
        for fmt in (I010, I416):
            near = _planar("random chroma", w, h, fmt, 9)
            m.encode([near, near])
            assert bytes(m.read()) == _want("random chroma", w, h, fmt, 9)


# ---- refusals ----
def test_what_is_no_format_no_pitch_or_no_address_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    w, h, fmt = 200, 120, I010C
    planes, want = _planes("random chroma", w, h, fmt, 31), _want("random chroma", w, h, fmt, 31)
    bufs, ptrs, rs, cp = _place(planes, 200, 100)
    odd = lambda k: [p + (c == k) for c, p in enumerate(ptrs)]
    attempts = [(ptrs, cp, bad, "Invalid Sample Format") for bad in NO_FORMAT]
    attempts += [(ptrs, 1, f, PITCH_MSG) for f in (I010, I010C, I212L, I416)] + [(ptrs, -99, I010C, PITCH_MSG), (ptrs, 199, I416, PITCH_MSG)]
    attempts += [(odd(k), cp, f, ALIGN_MSG) for k, f in ((0, I010), (1, I010C), (2, I212L))]
    with device.MixedBatch(2) as mb, device.FrameBatch(w, h, 2) as fb, device.TiledImage(w, h, 0, 0) as ti, \
            device.DeviceContext(0, 1, 0) as ctx:
        for at, ps, f, message in attempts:
            with pytest.raises(device.DeviceError, match=message) as e:
                mb.encode([(at, rs, ps, w, h)], sample_fmts=[f])
            assert e.value.code == api.HYD_API_ERROR
            with pytest.raises(device.DeviceError, match=message):
                mb.encode([(at, rs, ps, w, h)], sample_fmt=f)
            with pytest.raises(device.DeviceError, match=message):
                fb.encode([at], rs, ps, f)
            with pytest.raises(device.DeviceError, match=message):
                ti.encode(at, rs, ps, f)
            with pytest.raises(device.DeviceError, match=message) as e:
                ctx.encode_image(at, rs, ps, f, w, h)
            assert e.value.code == api.HYD_API_ERROR
            ctx.begin_frame(1)
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group(0, at, rs, ps, f, w, h, 0)
            with pytest.raises(device.DeviceError, match=message):
                ctx.encode_lf_group_at(0, at, rs, ps, f, w, h, 0, 0, w, h, 0)
            if message == "Invalid Sample Format":
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
        for fmt in (I010, I010C, I212L, I416):
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert 0 < lds <= 26 * 1280 and 0 < regs <= 128
