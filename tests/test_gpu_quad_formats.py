"""GPU: pictures whose pixel is one group of four samples, from device memory (HYDAMD_AYUV_*, HYDAMD_Y412_*, HYDAMD_Y416_*) on every
entry point that reads device pixels.  A pixel is an RGB pixel of its class right after the load: every file is compared whole with
what the compiled reference writes for the HYD_UINT8 or HYD_UINT16 picture the numpy model of the definition (quad_model.py) makes of
the same pixels; an AYUV file also with what the library itself writes for the three extracted planes as I444, a Y416 file as I416 and
a Y412 file with zero low bits as I412.  Every surface sits in an allocation that ends with the last pixel of its last row, 0x5A bytes
in the pitch's slack, or between 0x5A bytes."""
import ctypes as C

import numpy as np
import pytest

import planar_model as plm
import quad_model as qm
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_dword_formats import _frame, _pic as _dword_pic, _want as _dword_want
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_packed_formats import _packed, _want as _packed_want
from test_gpu_planar16_formats import _device_picture as _planar16_picture
from test_gpu_planar_formats import _plane_tensor
from test_gpu_yuv_formats import _nv12, _want as _nv12_want
from test_quad_formats import check_definition, hook

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = list(qm.FAMILY)
IDS = [qm.public_name(f).lower() for f in FAMILY]
AYUV, AYUV_601F, Y412, Y412_709F, Y416, Y416_601 = 524296, 524299, 524424, 524425, 524488, 524490
_cache = {}


def _pixels(kind, w, h, fmt, seed=1234):
    """host (h, w) dwords or qwords of one picture: a photograph in valid codes (Y412's low four bits zero, the fourth sample random),
    pixels of random bits — the fourth sample and all three codes far out of range — all-zeros or all-ones"""
    from hydrium_amd import synth

    bits = 8 * qm.pixel_bytes(fmt)
    key = ("pixels", kind, w, h, fmt if kind == "photo" else bits, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        if kind == "photo":
            d = qm.surface_of_rgb(synth.make_image("photo", w, h, 16 if qm.depth_of(fmt) else 8, seed), fmt, rng.integers(0, 2 ** (bits // 4), (h, w)))
        elif kind == "random":
            d = rng.integers(0, 2 ** 64, (h, w), dtype=np.uint64) >> np.uint64(64 - bits)
        elif kind in ("zeros", "ones"):
            d = np.full((h, w), 0 if kind == "zeros" else 2 ** bits - 1, np.uint64)
        else:
            raise KeyError(kind)
        d = np.ascontiguousarray(d.astype(qm.dtype_of(fmt)))
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = qm.expected_rgb(_pixels(kind, w, h, fmt, seed), fmt)
        _cache[key].setflags(write=False)
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234):
    """the reference's file for the model's RGB picture of those pixels; made once"""
    return _reference_of(("quad", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed))


def _surface(pixels, pitch=None):
    """the rows in an allocation of its own that ENDS with the last pixel of the last row, 0x5A bytes in the pitch's slack"""
    import torch

    h, w = pixels.shape
    pitch = pitch or w
    host = np.full(pitch * (h - 1) + w, 0x5A5A5A5A5A5A5A5A >> (64 - 8 * pixels.itemsize), pixels.dtype)
    for r in range(h):
        host[pitch * r: pitch * r + w] = pixels[r]
    return torch.from_numpy(host.view(np.int64 if pixels.itemsize == 8 else np.int32)).cuda().as_strided((h, w), (pitch, 1))


def _of_surface(s, w, fmt):
    from hydrium_amd import device

    pic = device.Y416(s, w, fmt, depth=qm.BITS[qm.depth_of(fmt)]) if qm.depth_of(fmt) else device.Ayuv(s, w, fmt)
    assert pic.sample_fmt == fmt
    return pic


def _picture(pixels, fmt, pitch=None):
    pic = _of_surface(_surface(pixels, pitch), pixels.shape[1], fmt)
    assert pic.pitch == (pitch or pixels.shape[1]) or pixels.shape[0] == 1
    return pic


def _pic(kind, w, h, fmt, seed=1234, pitch=None):
    import torch

    key = ("dev", kind, w, h, fmt, seed, pitch)
    if key not in _cache:
        _cache[key] = _picture(_pixels(kind, w, h, fmt, seed), fmt, pitch)
        torch.cuda.synchronize()
    return _cache[key]


def _place(pixels, pitch, shift=0, flip=False):
    """the surface at a bare address between 0x5A bytes: (buffer to keep alive, the three addresses, row stride in pixels).  shift moves
    the first pixel by that many BYTES from a 256-byte boundary; flip stores the rows bottom-up: a negative pitch"""
    import torch

    h, w = pixels.shape
    b = pixels.itemsize
    host = np.full((256 + b * pitch * (h + 2) + 255) // 256 * 256, 0x5A, np.uint8)
    at = 256 + shift
    for r in range(h):
        o = at + b * pitch * (h - 1 - r if flip else r)
        host[o: o + b * w] = pixels[r].view(np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0
    first = buf.data_ptr() + at + (b * pitch * (h - 1) if flip else 0)
    return buf, [first] * 3, -pitch if flip else pitch


def _file_of(ctx, pic, slots=1):
    assert ctx.encode_image_tensor(pic) == slots
    return _frame(ctx, pic.width, pic.height, slots)


# ---- the definition on the device ----
def test_the_device_build_of_the_definition_equals_the_model():
    check_definition(hook(C.CDLL(hbuild.PROBE_PATH).hydt_quad_to_rgb_device, 0))


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
def test_random_bits_zeros_and_ones_equal_the_reference(fmt):
    """every bit random — the fourth sample set, all three codes far outside their range, most pixels clamped — and the two ends"""
    from hydrium_amd import device

    rgb = _model("random", 257, 255, fmt)
    assert ((rgb == 0) | (rgb == (65535 if qm.depth_of(fmt) else 255))).any(-1).mean() > 0.4
    y, u, v, a = qm.samples(_pixels("random", 257, 255, fmt), fmt)
    assert (a != 0).mean() > 0.9 and len(np.unique(a)) > 200
    if ((fmt - 524288) & 3) in (0, 2):  # limited range: codes outside 16 ... 235 / 240 of the top byte
        assert ((y >> (8 if qm.depth_of(fmt) else 0)) > 235).mean() > 0.05 and ((u >> (8 if qm.depth_of(fmt) else 0)) < 16).mean() > 0.03
    with device.DeviceContext(0, 1, 0) as ctx:
        for kind in ("random", "zeros", "ones"):
            for w, h in ((33, 9), (257, 255)):
                got, want = _file_of(ctx, _pic(kind, w, h, fmt)), _want(kind, w, h, fmt)
                assert len(got) == len(want) and got == want, (kind, w, h)


@pytest.mark.parametrize("fmt", [AYUV_601F, Y412], ids=["ayuv_bt601_full", "y412_bt709"])
def test_a_picture_of_two_lf_groups(fmt):
    from hydrium_amd import device

    w, h = 2057, 9
    with device.DeviceContext(0, 2, 0) as ctx:
        got = _file_of(ctx, _pic("random", w, h, fmt, 9), 2)
    want = _want("random", w, h, fmt, 9)
    assert len(got) == len(want) and got == want


# ---- layouts ----
@pytest.mark.parametrize("fmt", [AYUV, Y416_601], ids=["ayuv_bt709", "y416_bt601"])
def test_pitches_wider_than_the_row_and_negative_give_one_file(fmt):
    """232 x 188 and 33 x 9 random pixels: the pitch the width, wider with 0x5A slack (odd and even numbers of pixels, so rows start on
    every residue of the pixel modulo 16 bytes), and negative"""
    from hydrium_amd import device

    b = qm.pixel_bytes(fmt)
    for w, h in ((232, 188), (33, 9)):
        d, want = _pixels("random", w, h, fmt, 77), _want("random", w, h, fmt, 77)
        placed = {"the width": _place(d, w), "wider, odd": _place(d, w + 5), "wider, even": _place(d, w + 8), "shifted a pixel": _place(d, w + 3, shift=b),
                  "negative": _place(d, w, flip=True), "negative and wider": _place(d, w + 7, shift=3 * b, flip=True)}
        assert placed["negative"][2] == -w and placed["negative and wider"][2] == -(w + 7)
        with device.MixedBatch(len(placed) + 2) as mb:
            mb.encode([(ptrs, rs, 1, w, h) for _, ptrs, rs in placed.values()] + [_pic("random", w, h, fmt, 77), _pic("random", w, h, fmt, 77, w + 6)],
                      sample_fmt=fmt)
            _check(mb, [want] * (len(placed) + 2))
        del placed


@pytest.mark.parametrize("fmt", [AYUV + 2, Y412_709F], ids=["ayuv_bt601", "y412_bt709_full"])
def test_a_crop_at_odd_x0_and_y0_is_the_picture_cut_out_on_the_host(fmt):
    from hydrium_amd import device

    W, H, x0, y0, w, h = 300, 280, 37, 11, 257, 263
    big = _pixels("random", W, H, fmt, 5)
    cut = np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])
    want = _reference_of(("quad crop", fmt), qm.expected_rgb(cut, fmt))
    surface = _surface(big)
    pic = _of_surface(surface[y0:y0 + h, x0:], w, fmt)
    assert pic.pointers()[0] == surface.data_ptr() + qm.pixel_bytes(fmt) * (y0 * W + x0) and (pic.pitch, pic.height) == (W, h)
    with device.DeviceContext(0, 1, 0) as ctx:
        assert _file_of(ctx, pic) == want
    with device.MixedBatch(2) as mb:
        mb.encode([pic, _picture(cut, fmt)])
        _check(mb, [want, want])


def test_a_surface_of_samples_four_to_a_pixel_gives_the_same_file():
    """the (h, w, 4) view of bytes or words is the same memory"""
    import torch
    from hydrium_amd import device

    w, h = 33, 9
    for fmt, dtype in ((AYUV, torch.uint8), (Y416, torch.int16)):
        s = _pic("random", w, h, fmt).surface
        pic = _of_surface(s.view(dtype).view(h, w, 4), w, fmt)
        assert pic.pointers() == _pic("random", w, h, fmt).pointers()
        with device.DeviceContext(0, 1, 0) as ctx:
            assert _file_of(ctx, pic) == _want("random", w, h, fmt)


# ---- the planar picture of the same samples ----
@pytest.mark.parametrize("fmt", qm.AYUV, ids=IDS[:4])
def test_an_ayuv_file_is_the_i444_file_of_its_three_planes(fmt):
    from hydrium_amd import device

    w, h = 257, 255
    y, u, v, _ = qm.samples(_pixels("random", w, h, fmt), fmt)
    cp = (w + 3) // 4 * 4
    planar = device.PlanarYuv(_plane_tensor(y, cp), _plane_tensor(u, cp), _plane_tensor(v, cp), 16 + qm.matrix_of(fmt), "444", "nearest")
    assert planar.sample_fmt == qm.as_planar(fmt) == 520 + qm.matrix_of(fmt) and plm.sub_of(planar.sample_fmt) == plm.S444
    with device.MixedBatch(2) as mb:
        mb.encode([_pic("random", w, h, fmt), planar], sample_fmts="each")
        files = [bytes(f) for f in mb.read()]
    assert files[0] == files[1] == _want("random", w, h, fmt)


@pytest.mark.parametrize("fmt", qm.Y412 + qm.Y416, ids=IDS[4:])
def test_a_y416_file_is_the_i416_file_and_a_y412_file_with_zero_low_bits_the_i412_file(fmt):
    from hydrium_amd import device

    w, h = 257, 255
    d = _pixels("random", w, h, fmt)
    if qm.depth_of(fmt) == 2:
        d = d & np.uint64(0xFFF0FFF0FFF0FFF0)
    y, u, v, _ = qm.samples(d, fmt)
    shift = 16 - qm.BITS[qm.depth_of(fmt)]
    planar = _planar16_picture((y >> shift, u >> shift, v >> shift), qm.as_planar(fmt))
    assert planar.sample_fmt == {2: 2184, 3: 2248}[qm.depth_of(fmt)] + qm.matrix_of(fmt)
    want = _reference_of(("quad as planar", fmt), qm.expected_rgb(d, fmt))
    with device.MixedBatch(2) as mb:
        mb.encode([_picture(d, fmt), planar], sample_fmts="each")
        files = [bytes(f) for f in mb.read()]
    assert files[0] == files[1] == want


# ---- entry points ----
def test_a_frame_batch_of_two():
    from hydrium_amd import device

    w, h = 264, 200
    for fmt in (AYUV, Y412, Y416):
        pics = [_pic("photo", w, h, fmt, s) for s in (11, 12)]
        with device.FrameBatch(w, h, 2) as fb:
            fb.encode(pics)
            _check(fb, [_want("photo", w, h, fmt, s) for s in (11, 12)])


def test_beside_the_other_families_in_one_launch_group_with_an_outcome_per_image():
    import torch
    from hydrium_amd import device

    w, h = 27, 19
    rgb16 = _image("photo", w, h, 16, 43)[0]
    imgs = [_pic("photo", w, h, AYUV, 51), _pic("photo", 232, 188, Y416_601, 52), _pic("photo", w, h, Y412_709F, 54), _dword_pic("photo", w, h, 131147, 53),
            _packed("photo", w, h, 8192, "uyvy", 51), _nv12("photo", w, h, 17, 37, 28),
            rgb16 if rgb16.dtype == torch.int16 else rgb16.view(torch.int16)]
    wants = [_want("photo", w, h, AYUV, 51), _want("photo", 232, 188, Y416_601, 52), _want("photo", w, h, Y412_709F, 54), _dword_want("photo", w, h, 131147, 53),
             _packed_want("photo", w, h, 8192, 51), _nv12_want("photo", w, h, 17, 37), _reference("photo", w, h, 16, 43)]
    with device.MixedBatch(len(imgs), image_errors=True) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        assert mb.status().tolist() == [0] * len(imgs)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])
        assert mb.status().tolist() == [0] * len(imgs)


@pytest.mark.parametrize("fmt", [AYUV + 1, Y416], ids=["ayuv_bt709_full", "y416_bt709"])
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

    w, h = 2057, 9
    for fmt in (AYUV_601F, Y412):
        pic = _pic("random", w, h, fmt, 9)
        with device.DeviceContext(0, 2, 0) as ctx:
            ctx.begin_frame(2)
            for tx in range(2):
                ctx.encode_lf_group_at(tx, pic.pointers(), pic.pitch, pic.pixel_stride, fmt, w, h, tx * 2048, 0, min(2048, w - tx * 2048), h, tx)
            ctx.finish_frame(2)
            got = _frame(ctx, w, h, 2)
        want = _want("random", w, h, fmt, 9)
        assert len(got) == len(want) and got == want


def test_sharded_frames_take_the_family():
    """there is no chroma filter, so nothing is refused: one format of each depth, and the descriptor says the same of all twelve"""
    from hydrium_amd import device

    w, h = 2057, 9
    with device.MultiFrame((0, 0), w, h) as m:  # two LF groups, one per (aliased) shard
        for fmt in (AYUV_601F, Y412, Y416_601):
            pic = _pic("random", w, h, fmt, 9)
            m.encode([pic, pic])
            assert bytes(m.read()) == _want("random", w, h, fmt, 9), fmt


# ---- refusals ----
def test_what_is_no_format_or_no_layout_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    w, h, fmt = 200, 120, Y416
    d, want = _pixels("random", w, h, fmt, 31), _want("random", w, h, fmt, 31)
    buf, ptrs, rs = _place(d, w + 4)
    p0 = ptrs[0]
    assert p0 % 8 == 0
    attempts = [(ptrs, 1, bad, "Invalid Sample Format") for bad in (524288, 524360, 524300, 524492)]
    attempts += [(ptrs, ps, f, qm.LAYOUT_MSG) for ps in (0, 2, 4, -1) for f in (AYUV, Y416)]  # the stride
    attempts += [(p, 1, f, qm.LAYOUT_MSG) for f in (AYUV_601F, Y412) for p in ([p0, p0 + 8, p0 + 16], [p0, p0, p0 + 8], [p0, p0 + 8, p0])]  # unequal pointers
    attempts += [([p0 + off] * 3, 1, AYUV, qm.LAYOUT_MSG) for off in (1, 2, 3)]  # an address off the dword
    attempts += [([p0 + off] * 3, 1, f, qm.LAYOUT_MSG) for f in (Y412, Y416) for off in (2, 4, 6)]  # off the qword: + 4 too
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
            if message != qm.LAYOUT_MSG:
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


def test_the_host_pointer_entry_points_refuse_all_twelve():
    from hydrium_amd import device

    host = np.zeros((16, 16), np.uint64)
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
        pic = _pic("photo", 33, 9, AYUV, 1234 + 17 * 3)  # and the context goes on
        assert _file_of(ctx, pic) == _want("photo", 33, 9, AYUV, 1234 + 17 * 3)


# ---- the kernel instances ----
def test_the_new_instances_footprint():
    """no more than 31 856 B of LDS and 128 registers for either storage form, as the card reports it"""
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        for fmt in (AYUV, Y412, Y416):
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert 0 < lds <= 31856 and 0 < regs <= 128
