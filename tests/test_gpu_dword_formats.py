"""GPU: pictures whose pixel is one dword of three 10-bit fields, from device memory (HYDAMD_RGB10A2, HYDAMD_BGR10A2, HYDAMD_Y410_*) on
every entry point that reads device pixels.  A pixel is a 16-bit RGB pixel right after the load: every file is compared whole with what
the compiled reference writes for the HYD_UINT16 picture the numpy model of the definition (dword_model.py) makes of the same dwords;
a Y410 file also with what the library itself writes for the three extracted planes as I410.  Every surface sits in an allocation that
ends with the last dword of its last row, 0x5A bytes in the pitch's slack, or between 0x5A bytes."""
import ctypes as C

import numpy as np
import pytest

import dword_model as dm
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_dword_formats import check_definition, hook
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_packed16_formats import _packed as _packed16, _want as _packed16_want
from test_gpu_planar16_formats import _device_picture as _planar16_picture
from test_gpu_yuv_formats import _nv12, _want as _nv12_want

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = list(dm.FAMILY)
IDS = [dm.public_name(f).lower() for f in FAMILY]
RGB10, BGR10, Y410, Y410_601F = 131072, 131073, 131144, 131147
_cache = {}


def _dwords(kind, w, h, fmt, seed=1234):
    """host (h, w) uint32 of one picture: a photograph in valid codes (the spare bits random), dwords of 32 random bits — the spare bits
    and YCbCr far out of range — all-zeros or all-ones"""
    from hydrium_amd import synth

    key = ("dwords", kind, w, h, fmt if kind == "photo" else 0, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        if kind == "photo":
            d = dm.surface_of_rgb(synth.make_image("photo", w, h, 16, seed), fmt, rng.integers(0, 4, (h, w)))
        elif kind == "random":
            d = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
        elif kind in ("zeros", "ones"):
            d = np.full((h, w), 0 if kind == "zeros" else 0xFFFFFFFF, np.uint32)
        else:
            raise KeyError(kind)
        d = np.ascontiguousarray(d, np.uint32)
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = dm.expected_rgb(_dwords(kind, w, h, fmt, seed), fmt)
        _cache[key].setflags(write=False)
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234):
    """the reference's file for the model's RGB16 picture of those dwords; made once"""
    return _reference_of(("dword", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed))


def _surface(dwords, pitch=None):
    """the rows in an allocation of its own that ENDS with the last dword of the last row, 0x5A bytes in the pitch's slack"""
    import torch

    h, w = dwords.shape
    pitch = pitch or w
    host = np.full(pitch * (h - 1) + w, 0x5A5A5A5A, np.uint32)
    for r in range(h):
        host[pitch * r: pitch * r + w] = dwords[r]
    return torch.from_numpy(host.view(np.int32)).cuda().as_strided((h, w), (pitch, 1))


def _picture(dwords, fmt, pitch=None):
    from hydrium_amd import device

    s = _surface(dwords, pitch)
    pic = device.Y410(s, dwords.shape[1], fmt) if dm.is_ycbcr(fmt) else device.Rgb10(s, dwords.shape[1], ("rgb", "bgr")[fmt - RGB10])
    assert pic.sample_fmt == fmt and (pic.pitch == (pitch or dwords.shape[1]) or dwords.shape[0] == 1)
    return pic


def _pic(kind, w, h, fmt, seed=1234, pitch=None):
    import torch

    key = ("dev", kind, w, h, fmt, seed, pitch)
    if key not in _cache:
        _cache[key] = _picture(_dwords(kind, w, h, fmt, seed), fmt, pitch)
        torch.cuda.synchronize()
    return _cache[key]


def _place(dwords, pitch, shift=0, flip=False):
    """the surface at a bare address between 0x5A bytes: (buffer to keep alive, the three addresses, row stride in dwords).  shift moves
    the first dword by that many BYTES from a 256-byte boundary; flip stores the rows bottom-up: a negative pitch"""
    import torch

    h, w = dwords.shape
    host = np.full((256 + 4 * pitch * (h + 2) + 255) // 256 * 256, 0x5A, np.uint8)
    at = 256 + shift
    for r in range(h):
        o = at + 4 * pitch * (h - 1 - r if flip else r)
        host[o: o + 4 * w] = dwords[r].view(np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0
    first = buf.data_ptr() + at + (4 * pitch * (h - 1) if flip else 0)
    return buf, [first] * 3, -pitch if flip else pitch


def _frame(ctx, w, h, slots=1):
    """the file of the frame a DeviceContext has just been given; the wait comes first, so that a frame of random dwords that outgrew
    the token arrays has been rerun before its blob is taken"""
    import torch
    from hydrium_amd import device

    ctx.sync()
    full = torch.zeros(ctx.blob_bound(slots), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the zeros are torch's stream's: they land before the context's stream writes the blob over them)
    ctx.export_frame(slots, full)
    ctx.sync()
    head = device.blob_header(full[:64].cpu().numpy().tobytes())
    return device.frame_from_blobs(api.HYDImageMetadata(w, h, 0, -1, -1), [full[: int(head["total_bytes"])].cpu().numpy().tobytes()])


def _file_of(ctx, pic, slots=1):
    assert ctx.encode_image_tensor(pic) == slots
    return _frame(ctx, pic.width, pic.height, slots)


# ---- the definition on the device ----
def test_the_device_build_of_the_definition_equals_the_model():
    check_definition(hook(C.CDLL(hbuild.PROBE_PATH).hydt_dword_to_rgb_device, 0))


# ---- reference parity: whole files through encode_image_tensor ----
SIZES = [(1, 1), (7, 3), (9, 8), (33, 9), (232, 188), (257, 255), (520, 264)]


@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_photographs_of_seven_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        files = set()
        for k, (w, h) in enumerate(SIZES):
            got, want = _file_of(ctx, _pic("photo", w, h, fmt, 1234 + 17 * k)), _want("photo", w, h, fmt, 1234 + 17 * k)
            assert len(got) == len(want) and got == want, (w, h)
            files.add(want)
        assert len(files) == len(SIZES)


@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_random_dwords_zeros_and_ones_equal_the_reference(fmt):
    """all 32 bits random — the spare bits set, YCbCr codes far outside their range, most Y410 pixels clamped — and the two ends"""
    from hydrium_amd import device

    if dm.is_ycbcr(fmt):
        rgb = _model("random", 257, 255, fmt)
        assert ((rgb == 0) | (rgb == 65535)).any(-1).mean() > 0.4
    assert (_dwords("random", 257, 255, fmt) >> 30 != 0).mean() > 0.7
    with device.DeviceContext(0, 1, 0) as ctx:
        for kind in ("random", "zeros", "ones"):
            for w, h in ((9, 8), (257, 255)):
                got, want = _file_of(ctx, _pic(kind, w, h, fmt)), _want(kind, w, h, fmt)
                assert len(got) == len(want) and got == want, (kind, w, h)


@pytest.mark.parametrize("fmt", [BGR10, Y410_601F], ids=["bgr10a2", "y410_bt601_full"])
def test_a_picture_of_two_lf_groups(fmt):
    from hydrium_amd import device

    w, h = 2056, 16
    with device.DeviceContext(0, 2, 0) as ctx:
        got = _file_of(ctx, _pic("random", w, h, fmt, 9), 2)
    want = _want("random", w, h, fmt, 9)
    assert len(got) == len(want) and got == want


# ---- layouts ----
@pytest.mark.parametrize("fmt", [RGB10, Y410 + 1], ids=["rgb10a2", "y410_bt709_full"])
def test_pitches_wider_than_the_row_and_negative_give_one_file(fmt):
    """232 x 188 and 33 x 9 random dwords: the pitch the width, wider with 0x5A slack (odd and even numbers of dwords, so rows start on
    every residue of the dword modulo 16 bytes), and negative"""
    from hydrium_amd import device

    for w, h in ((232, 188), (33, 9)):
        d, want = _dwords("random", w, h, fmt, 77), _want("random", w, h, fmt, 77)
        placed = {"the width": _place(d, w), "wider, odd": _place(d, w + 5), "wider, even": _place(d, w + 8), "shifted a dword": _place(d, w + 3, shift=4),
                  "negative": _place(d, w, flip=True), "negative and wider": _place(d, w + 7, shift=12, flip=True)}
        assert placed["negative"][2] == -w and placed["negative and wider"][2] == -(w + 7)
        with device.MixedBatch(len(placed) + 2) as mb:
            mb.encode([(ptrs, rs, 1, w, h) for _, ptrs, rs in placed.values()] + [_pic("random", w, h, fmt, 77), _pic("random", w, h, fmt, 77, w + 6)],
                      sample_fmt=fmt)
            _check(mb, [want] * (len(placed) + 2))
        del placed


@pytest.mark.parametrize("fmt", [BGR10, Y410 + 2], ids=["bgr10a2", "y410_bt601"])
def test_a_crop_at_odd_x0_and_y0_is_the_picture_cut_out_on_the_host(fmt):
    from hydrium_amd import device

    W, H, x0, y0, w, h = 300, 280, 37, 11, 257, 263
    big = _dwords("random", W, H, fmt, 5)
    cut = np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])
    want = _reference_of(("dword crop", fmt), dm.expected_rgb(cut, fmt))
    surface = _surface(big)
    view = surface[y0:y0 + h, x0:]
    pic = device.Y410(view, w, fmt) if dm.is_ycbcr(fmt) else device.Rgb10(view, w, "bgr")
    assert pic.pointers()[0] == surface.data_ptr() + 4 * (y0 * W + x0) and (pic.pitch, pic.height) == (W, h)
    with device.DeviceContext(0, 1, 0) as ctx:
        assert _file_of(ctx, pic) == want
    with device.MixedBatch(2) as mb:
        mb.encode([pic, _picture(cut, fmt)])
        _check(mb, [want, want])


def test_the_two_rgb_orders_of_one_picture_give_one_file():
    from hydrium_amd import device

    w, h = 232, 188
    rgb = _dwords("photo", w, h, RGB10, 21)
    r, g, b = dm.fields(rgb)
    bgr = dm.pack(b, g, r, 3)
    assert not np.array_equal(rgb, bgr) and np.array_equal(dm.expected_rgb(rgb, RGB10), dm.expected_rgb(bgr, BGR10))
    want = _want("photo", w, h, RGB10, 21)
    misread = _reference_of(("dword misread",), dm.expected_rgb(rgb, BGR10))  # the same dwords under the other number: another file
    assert misread != want
    a = _picture(rgb, RGB10)
    with device.MixedBatch(3) as mb:
        mb.encode([a, _picture(bgr, BGR10), device.Rgb10(a.surface, w, "bgr")], sample_fmts="each")
        _check(mb, [want, want, misread])


@pytest.mark.parametrize("fmt", dm.Y410, ids=IDS[2:])
def test_a_y410_file_is_the_i410_file_of_its_three_fields(fmt):
    from hydrium_amd import device

    w, h = 257, 255
    d = _dwords("random", w, h, fmt)
    planar = _planar16_picture(dm.y410_planes(d), dm.as_i410(fmt))
    assert planar.sample_fmt == 2120 + dm.matrix_of(fmt) and planar.pixel_stride >= w
    with device.MixedBatch(2) as mb:
        mb.encode([_pic("random", w, h, fmt), planar], sample_fmts="each")
        files = [bytes(f) for f in mb.read()]
    assert files[0] == files[1] == _want("random", w, h, fmt)


# ---- entry points ----
def test_a_frame_batch_of_two():
    from hydrium_amd import device

    w, h = 264, 200
    for fmt in (RGB10, Y410):
        pics = [_pic("photo", w, h, fmt, s) for s in (11, 12)]
        with device.FrameBatch(w, h, 2) as fb:
            fb.encode(pics)
            _check(fb, [_want("photo", w, h, fmt, s) for s in (11, 12)])


def test_beside_the_other_families_in_one_launch_group_with_an_outcome_per_image():
    import torch
    from hydrium_amd import device

    w, h = 27, 19
    rgb16 = _image("photo", w, h, 16, 43)[0]
    imgs = [_pic("photo", w, h, RGB10, 51), _pic("photo", w, h, BGR10, 52), _pic("photo", 232, 188, Y410_601F, 53),
            _packed16("photo", w, h, 32832, "vyuy", 51), _nv12("photo", w, h, 17, 37, 28),
            rgb16 if rgb16.dtype == torch.int16 else rgb16.view(torch.int16), _image("photo", w, h, 8, 42)[0]]
    wants = [_want("photo", w, h, RGB10, 51), _want("photo", w, h, BGR10, 52), _want("photo", 232, 188, Y410_601F, 53),
             _packed16_want("photo", w, h, 32832, 51), _nv12_want("photo", w, h, 17, 37), _reference("photo", w, h, 16, 43), _reference("photo", w, h, 8, 42)]
    with device.MixedBatch(len(imgs), image_errors=True) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        assert mb.status().tolist() == [0] * len(imgs)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])
        assert mb.status().tolist() == [0] * len(imgs)


@pytest.mark.parametrize("fmt", [RGB10, Y410 + 1], ids=["rgb10a2", "y410_bt709_full"])
def test_a_tiled_image_of_256_tiles_equals_the_references_tiled_file(fmt):
    from oracle import refprobe
    from hydrium_amd import device

    w, h = 520, 264
    want = api.encode_image(refprobe.reference_library(optimised=True), _model("photo", w, h, fmt, 1234 + 17 * 6), shift_x=0, shift_y=0)
    with device.TiledImage(w, h, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_pic("photo", w, h, fmt, 1234 + 17 * 6))
        assert bytes(ti.read()) == want


def test_the_callers_own_loop_over_lf_group_at():
    from hydrium_amd import device

    w, h = 2056, 16
    for fmt in (RGB10, Y410_601F):
        pic = _pic("random", w, h, fmt, 9)
        with device.DeviceContext(0, 2, 0) as ctx:
            ctx.begin_frame(2)
            for tx in range(2):
                ctx.encode_lf_group_at(tx, pic.pointers(), pic.pitch, pic.pixel_stride, fmt, w, h, tx * 2048, 0, min(2048, w - tx * 2048), h, tx)
            ctx.finish_frame(2)
            got = _frame(ctx, w, h, 2)
        want = _want("random", w, h, fmt, 9)
        assert len(got) == len(want) and got == want


def test_sharded_frames_take_all_six():
    """there is no chroma filter, so nothing is refused"""
    from hydrium_amd import device

    w, h = 2056, 16
    with device.MultiFrame((0, 0), w, h) as m:  # two LF groups, one per (aliased) shard
        for fmt in FAMILY:
            pic = _pic("random", w, h, fmt, 9)
            m.encode([pic, pic])
            assert bytes(m.read()) == _want("random", w, h, fmt, 9), fmt


# ---- refusals ----
def test_what_is_no_format_or_no_layout_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    w, h, fmt = 200, 120, Y410
    d, want = _dwords("random", w, h, fmt, 31), _want("random", w, h, fmt, 31)
    buf, ptrs, rs = _place(d, w + 4)
    p0 = ptrs[0]
    attempts = [(ptrs, 1, bad, "Invalid Sample Format") for bad in (131074, 131148)]
    attempts += [(ptrs, ps, f, dm.LAYOUT_MSG) for ps in (0, 2, 3, -1) for f in (RGB10, Y410)]  # the stride
    attempts += [(p, 1, f, dm.LAYOUT_MSG) for f in (BGR10, Y410_601F) for p in (
        [p0, p0 + 4, p0 + 8], [p0, p0, p0 + 4], [p0, p0 + 4, p0],           # unequal pointers
        [p0 + 1] * 3, [p0 + 2] * 3, [p0 + 3] * 3)]                          # an address off the dword
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
            if message != dm.LAYOUT_MSG:
                with pytest.raises(device.DeviceError):
                    ctx.transform_footprint(f)
        # nothing was enqueued: every object takes the good picture next
        mb.encode([(ptrs, rs, 1, w, h)], sample_fmt=fmt)
        _check(mb, [want])
        fb.encode([ptrs], rs, 1, fmt)
        _check(fb, [want])
        ti.encode(ptrs, rs, 1, fmt)
        ti.read()
        ctx.encode_image(ptrs, rs, 1, fmt, w, h)
        assert _frame(ctx, w, h) == want
    del buf


def test_the_host_pointer_entry_points_refuse_all_six():
    from hydrium_amd import device

    host = np.zeros((16, 16), np.uint32)
    p = host.ctypes.data
    lib = api.Library()
    with device.DeviceContext(0, 1, 0) as ctx:
        for fmt in FAMILY:
            ctx.begin_frame(1)
            with pytest.raises(device.DeviceError, match="Invalid Sample Format") as e:
                ctx.encode_lf_group(0, [p, p, p], 16, 1, fmt, 16, 16, 0, host=True)
            assert e.value.code == api.HYD_API_ERROR
            with api.Encoder(lib) as enc:
                assert enc.set_metadata(16, 16) == api.HYD_OK
                assert enc.send_tile_ptrs([p, p, p], 0, 0, 16, 1, -1, fmt) == api.HYD_API_ERROR
                assert enc.error_message() == "Invalid Sample Format"
        pic = _pic("photo", 33, 9, RGB10, 1234 + 17 * 3)  # and the context goes on
        assert _file_of(ctx, pic) == _want("photo", 33, 9, RGB10, 1234 + 17 * 3)


# ---- the kernel instances ----
def test_the_new_instances_footprint():
    """31 856 B of LDS as the other storage forms of the 16-bit class, and the register counts DESIGN.md writes down"""
    from hydrium_amd import device

    import os

    design = " ".join(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read().split())
    with device.DeviceContext(0, 1, 0) as ctx:
        got = {}
        for fmt in (RGB10, Y410):
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert lds == 31856 and 0 < regs <= 128
            got[fmt] = regs
    assert f"reports 31 856 B and {got[RGB10]} registers for 131072, 31 856 B and {got[Y410]} for 131144 on the card" in design
