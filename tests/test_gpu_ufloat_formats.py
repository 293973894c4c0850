"""GPU: the float render targets whose pixel is one dword of three unsigned floats, from device memory (HYDAMD_R11G11B10F,
HYDAMD_RGB9E5) on every entry point that reads device pixels.  A sample is widened exactly on load and the pixel is a float32 pixel
from there on: every file is compared whole with what the compiled reference writes for the HYD_FLOAT32 picture the numpy model of the
definition (ufloat_model.py) makes of the same dwords, and with what the library itself writes for that float32 picture.  Every surface
sits in an allocation that ends with the last dword of its last row, 0x5A bytes in the pitch's slack, or between 0x5A bytes."""
import ctypes as C

import numpy as np
import pytest

import ufloat_model as um
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_image_status import _check_outcomes
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_packed16_formats import _packed as _packed16, _want as _packed16_want
from test_gpu_yuv_formats import _nv12, _want as _nv12_want
from test_ufloat_formats import check_definition, check_widening, every_pattern_through, surface_hook, widen_hook

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = list(um.FAMILY)
IDS = [um.public_name(f).lower() for f in FAMILY]
R11, E5 = um.R11G11B10F, um.RGB9E5
_cache = {}


def _source(kind, w, h, seed):
    from hydrium_amd import synth

    if kind == "gamut":  # samples above 10.0: what the float tests hold to the reference outside [0, 1]
        img = synth.make_image_f32("photo", w, h, seed).copy()
        img[:64, :64] *= 300
        return img
    return synth.make_image_f32(kind, w, h, seed)


def _dwords(kind, w, h, fmt, seed=1234):
    """host (h, w) uint32 of one picture: a float32 picture packed to the nearest fields by the model; dwords of random bits with the
    top bit of every exponent cleared — noise below 2.0 (R11G11B10F: nothing non-finite) or 1.0 (RGB9E5), subnormals and every
    mantissa among it, the range the float tests hold noise to the reference in; all-zeros or all-ones"""
    key = ("dwords", kind, w, h, 0 if kind in ("zeros", "ones") else fmt, seed)
    if key not in _cache:
        if kind in ("photo", "gamut"):
            d = um.pack(_source(kind, w, h, seed), fmt)
        elif kind == "random":
            d = np.random.default_rng(seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)
            d &= np.uint32(~(1 << 10 | 1 << 21 | 1 << 31) & 0xFFFFFFFF if fmt == R11 else 0x7FFFFFFF)
        elif kind in ("zeros", "ones"):
            d = np.full((h, w), 0 if kind == "zeros" else 0xFFFFFFFF, np.uint32)
        else:
            raise KeyError(kind)
        d = np.ascontiguousarray(d, np.uint32)
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    """the widened float32 picture of those dwords"""
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = um.expected_f32(_dwords(kind, w, h, fmt, seed), fmt)
        _cache[key].setflags(write=False)
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234, linear_light=0):
    """the reference's file for the widened float32 picture; made once"""
    return _reference_of(("ufloat", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed), linear_light)


def _surface(dwords, pitch=None):
    """the rows in an allocation of its own that ENDS with the last dword of the last row, 0x5A bytes in the pitch's slack"""
    import torch

    h, w = dwords.shape
    pitch = pitch or w
    host = np.full(pitch * (h - 1) + w, 0x5A5A5A5A, np.uint32)
    for r in range(h):
        host[pitch * r: pitch * r + w] = dwords[r]
    return torch.from_numpy(host.view(np.int32)).cuda().as_strided((h, w), (pitch, 1))


def _wrap(surface, w, fmt):
    from hydrium_amd import device

    return (device.R11g11b10f if fmt == R11 else device.Rgb9e5)(surface, w)


def _picture(dwords, fmt, pitch=None):
    pic = _wrap(_surface(dwords, pitch), dwords.shape[1], fmt)
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


def _frame(ctx, w, h, slots=1, linear_light=0):
    """the file of the frame a DeviceContext has just been given"""
    import torch
    from hydrium_amd import device

    ctx.sync()
    full = torch.zeros(ctx.blob_bound(slots), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the zeros are torch's stream's: they land before the context's stream writes the blob over them)
    ctx.export_frame(slots, full)
    ctx.sync()
    head = device.blob_header(full[:64].cpu().numpy().tobytes())
    return device.frame_from_blobs(api.HYDImageMetadata(w, h, linear_light, -1, -1), [full[: int(head["total_bytes"])].cpu().numpy().tobytes()])


def _file_of(ctx, pic, slots=1, linear_light=0):
    assert ctx.encode_image_tensor(pic) == slots
    return _frame(ctx, pic.width, pic.height, slots, linear_light)


# ---- the widening on the device, and the existing float path ----
def test_every_pattern_is_widened_exactly_on_the_device():
    check_widening(*every_pattern_through(widen_hook(C.CDLL(hbuild.PROBE_PATH).hydt_ufloat_widen_device, 0)))


def test_the_device_build_of_the_definition_equals_the_model():
    check_definition(surface_hook(C.CDLL(hbuild.PROBE_PATH).hydt_ufloat_to_rgb_device, 0))


def _every_pattern_below_two(fmt):
    """256 x 256 dwords.  R11G11B10F: R, G and B each carry every field pattern below 2.0 (exponent 0 ... 15: 1024, 1024 and 512 of
    them, subnormals and zero among them) in a permutation of its own, the rest 0.5.  RGB9E5: the exponent is the pixel's, so the
    pixels are dealt to E = 0 ... 24 in turn, and under every E each channel carries every mantissa in a permutation of its own, the
    rest 256; then the pixels are shuffled"""
    rng = np.random.default_rng(7)
    if fmt == R11:
        planes = []
        for mbits in (6, 6, 5):
            cells = np.full(65536, 14 << mbits, np.uint32)
            cells[:16 << mbits] = np.arange(16 << mbits)
            planes.append(rng.permutation(cells))
        d = planes[0] | planes[1] << 11 | planes[2] << 22
    else:
        e = np.arange(65536, dtype=np.uint32) % 25
        d = e << 27
        for c in range(3):
            m = np.full(65536, 256, np.uint32)
            for k in range(25):
                at = np.flatnonzero(e == k)
                assert at.size >= 512
                cells = np.full(at.size, 256, np.uint32)
                cells[:512] = np.arange(512)
                m[at] = rng.permutation(cells)
            d = d | m << (9 * c)
        d = rng.permutation(d)
    return np.ascontiguousarray(d.astype(np.uint32).reshape(256, 256))


@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_every_pattern_below_two_codes_as_its_float32_widening_does(fmt):
    """the new loader against the existing float path on the same card"""
    import torch
    from hydrium_amd import device

    d = _every_pattern_below_two(fmt)
    if fmt == R11:
        for field, n in zip(um.fields(d, fmt), (1024, 1024, 512)):
            assert np.unique(field).size == n and int(field.max()) == n - 1
    else:
        r, g, b, e = um.fields(d, fmt)
        for m in (r, g, b):
            assert np.unique(e.astype(np.int64) << 9 | m).size == 25 * 512 and int(e.max()) == 24
    wide = um.expected_f32(d, fmt)
    assert np.isfinite(wide).all() and (fmt == E5 or float(wide.max()) < 2) and float(wide.min()) == 0
    t = torch.from_numpy(wide).cuda()
    with device.MixedBatch(2) as mb:
        mb.encode([_picture(d, fmt), t], sample_fmts="each")
        mb.result()
        a, b = (bytes(f) for f in mb.read())
    assert len(a) > 1000 and a == b


# ---- reference parity: whole files through encode_image_tensor ----
SIZES = [(1, 1), (7, 3), (9, 8), (33, 9), (232, 188), (257, 255), (520, 264)]


@pytest.mark.parametrize("linear_light", [0, 1], ids=["srgb", "linear"])
@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_photographs_of_seven_sizes_equal_the_reference(fmt, linear_light):
    """packed by the model to the nearest fields, then widened: the reference codes the float32 picture of exactly those samples"""
    from hydrium_amd import device

    with device.DeviceContext(0, 1, linear_light) as ctx:
        files = set()
        for k, (w, h) in enumerate(SIZES):
            got = _file_of(ctx, _pic("photo", w, h, fmt, 1234 + 17 * k), linear_light=linear_light)
            want = _want("photo", w, h, fmt, 1234 + 17 * k, linear_light)
            assert len(got) == len(want) and got == want, (w, h)
            files.add(want)
        assert len(files) == len(SIZES)


@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_a_picture_with_samples_above_ten_equals_the_reference(fmt):
    from hydrium_amd import device

    w, h = 232, 188
    assert float(_model("gamut", w, h, fmt).max()) > 10
    with device.DeviceContext(0, 1, 0) as ctx:
        got, want = _file_of(ctx, _pic("gamut", w, h, fmt)), _want("gamut", w, h, fmt)
    assert len(got) == len(want) and got == want


def test_all_zero_and_all_ones_surfaces():
    """all-ones is 511 * 2^7 in every channel of RGB9E5; it is a NaN in R11G11B10F, which the non-finite tests hold"""
    from hydrium_amd import device

    assert float(_model("ones", 9, 8, E5).min()) == 511 * 128 and not _model("zeros", 9, 8, R11).any()
    with device.DeviceContext(0, 1, 0) as ctx:
        for kind, fmt in (("zeros", E5), ("ones", E5), ("zeros", R11)):
            for w, h in ((9, 8), (257, 255)):
                got, want = _file_of(ctx, _pic(kind, w, h, fmt)), _want(kind, w, h, fmt)
                assert len(got) == len(want) and got == want, (kind, fmt, w, h)


# ---- non-finite fields ----
W_BAD, H_BAD = 33, 9
BAD = [(field, bits, at) for field in range(3) for bits in ("inf", "nan") for at in ("first", "middle", "last")]


def _with_bad_field(d, field, bits, at):
    """the dwords with an R11G11B10F Inf (exponent 31, mantissa 0) or NaN (mantissa 1 | top bit) in one field of one pixel"""
    shift, mbits = ((0, 6), (11, 6), (22, 5))[field]
    code = 31 << mbits | (0 if bits == "inf" else 1 | 1 << (mbits - 1))
    y, x = {"first": (0, 0), "middle": (H_BAD // 2, W_BAD // 2), "last": (H_BAD - 1, W_BAD - 1)}[at]
    bad = d.copy()
    bad[y, x] = (int(bad[y, x]) & ~(((1 << (mbits + 5)) - 1) << shift) & 0xFFFFFFFF) | code << shift
    return bad, (y, x, field)


@pytest.mark.parametrize("field,bits,at", BAD, ids=[f"{'rgb'[f]}-{b}-{a}" for f, b, a in BAD])
def test_a_non_finite_field_is_what_a_non_finite_float32_sample_is(field, bits, at):
    import torch
    from hydrium_amd import device

    w, h = W_BAD, H_BAD
    good, want = _dwords("photo", w, h, R11, 1234 + 17 * 3), _want("photo", w, h, R11, 1234 + 17 * 3)
    bad, (y, x, c) = _with_bad_field(good, field, bits, at)
    wide_bad = um.expected_f32(bad, R11)
    assert (np.isinf if bits == "inf" else np.isnan)(wide_bad[y, x, c]) and (~np.isfinite(wide_bad)).sum() == 1
    pic_bad, pic_good = _picture(bad, R11), _pic("photo", w, h, R11, 1234 + 17 * 3)
    f32_bad, f32_good = torch.from_numpy(wide_bad).cuda(), torch.from_numpy(_model("photo", w, h, R11, 1234 + 17 * 3).copy()).cuda()
    torch.cuda.synchronize()
    errors = []
    for given in (pic_bad, f32_bad):  # on a context: the same error
        with device.DeviceContext(0, 1, 0) as ctx:
            ctx.encode_image_tensor(given)
            with pytest.raises(device.DeviceError, match="NaN") as e:
                ctx.sync()
            errors.append((e.value.code, str(e.value)))
    assert errors[0] == errors[1] and errors[0][0] == -14
    with device.MixedBatch(4, image_errors=True) as mb:  # an outcome per image: the same status word, the files on both sides intact
        mb.encode([pic_good, pic_bad, f32_bad, f32_good], sample_fmts="each")
        _check_outcomes(mb, [want] * 4, {1, 2})
        status = mb.status().tolist()
        assert status[1] == status[2] != 0
    with device.FrameBatch(w, h, 3, image_errors=True) as fb:
        fb.encode([pic_good, pic_bad, pic_good])
        _check_outcomes(fb, [want] * 3, {1})
        packed_status = fb.status().tolist()
        fb.encode([f32_good, f32_bad, f32_good])
        _check_outcomes(fb, [want] * 3, {1})
        assert fb.status().tolist() == packed_status


# ---- geometry ----
@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_a_picture_of_two_lf_groups(fmt):
    from hydrium_amd import device

    w, h = 2056, 16
    with device.DeviceContext(0, 2, 0) as ctx:
        got = _file_of(ctx, _pic("random", w, h, fmt, 9), 2)
    want = _want("random", w, h, fmt, 9)
    assert len(got) == len(want) and got == want


@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_pitches_wider_than_the_row_and_negative_give_one_file(fmt):
    """232 x 188 and 33 x 9 random dwords: the pitch the width, wider with 0x5A slack (odd and even numbers of dwords, so rows start on
    every residue of the dword modulo 16 bytes: the two 16-byte loads and the per-dword loads both), and negative"""
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


@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_a_crop_at_odd_x0_and_y0_is_the_picture_cut_out_on_the_host(fmt):
    from hydrium_amd import device

    W, H, x0, y0, w, h = 300, 280, 37, 11, 257, 263
    big = _dwords("random", W, H, fmt, 5)
    cut = np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])
    want = _reference_of(("ufloat crop", fmt), um.expected_f32(cut, fmt))
    surface = _surface(big)
    pic = _wrap(surface[y0:y0 + h, x0:], w, fmt)
    assert pic.pointers()[0] == surface.data_ptr() + 4 * (y0 * W + x0) and (pic.pitch, pic.height) == (W, h)
    with device.DeviceContext(0, 1, 0) as ctx:
        assert _file_of(ctx, pic) == want
    with device.MixedBatch(2) as mb:
        mb.encode([pic, _picture(cut, fmt)])
        _check(mb, [want, want])


# ---- entry points ----
def test_a_frame_batch_of_two():
    from hydrium_amd import device

    w, h = 264, 200
    for fmt in FAMILY:
        pics = [_pic("photo", w, h, fmt, s) for s in (11, 12)]
        with device.FrameBatch(w, h, 2) as fb:
            fb.encode(pics)
            _check(fb, [_want("photo", w, h, fmt, s) for s in (11, 12)])


def test_beside_every_other_family_in_one_launch_group_with_an_outcome_per_image():
    """both formats beside one picture of each of the twenty-one older kinds the transform kernel has an instance for — the three
    classes' own samples (RGB8, RGB16, float32) and the eighteen older storage forms: float16 and bfloat16, and every YCbCr family
    (NV12, P016, planar of bytes and of words, packed 4:2:2 of bytes and of words, a dword a pixel, four samples a pixel), nearest and
    interpolated where it has both — so that the launch mask carries all 23 of its bits at once; 27 x 19 with pitches rounded up to a dword, forward and reversed"""
    import torch
    from hydrium_amd import device
    from test_gpu_chroma_filters import _nv12 as _nv12i, _want as _nv12i_want
    from test_gpu_dword_formats import _pic as _dword, _want as _dword_want
    from test_gpu_half_formats import _half
    from test_gpu_p016_formats import _p016, _want as _p016_want
    from test_gpu_packed_formats import _packed as _packed8, _want as _packed8_want
    from test_gpu_planar16_formats import _planar as _planar16, _want as _planar16_want
    from test_gpu_planar_formats import _planar as _planar8, _want as _planar8_want
    from test_gpu_quad_formats import _pic as _quad, _want as _quad_want

    w, h, pitch = 27, 19, 28
    rgb16 = _image("photo", w, h, 16, 43)[0]
    f16, bf16 = _half("photo", w, h, "float16", 45), _half("photo", w, h, "bfloat16", 46)
    imgs = [_pic("photo", w, h, R11, 51), _pic("photo", 232, 188, E5, 52),
            _nv12("photo", w, h, 17, 37, pitch), _nv12i("photo", w, h, 33, 38, pitch),                      # NV12, NV12I
            _p016("photo", w, h, 80, 39, pitch), _p016("photo", w, h, 96, 40, pitch),                        # P016, P016I
            _planar8("photo", w, h, 512, 35), _planar8("photo", w, h, 528, 36),                              # YUVP, YUVPI
            _planar16("photo", w, h, 2112, 47), _planar16("photo", w, h, 2196, 48),                          # YUVP16, YUVP16I
            _packed8("photo", w, h, 8192, "vyuy", 51), _packed8("photo", w, h, 8211, "yuyv", 52),            # YUY2, YUY2I
            _packed16("photo", w, h, 32832, "vyuy", 51), _packed16("photo", w, h, 32912, "yuyv", 52),        # Y216, Y216I
            _dword("photo", w, h, 131072, 51), _dword("photo", w, h, 131147, 53),                            # RGB10, Y410
            _quad("photo", w, h, 524296, 51), _quad("photo", w, h, 524425, 54),                              # AYUV, Y416
            _image("photo", w, h, 8, 42)[0], rgb16 if rgb16.dtype == torch.int16 else rgb16.view(torch.int16),
            _image("photo", w, h, 32, 44)[0], f16[0], bf16[0]]
    wants = [_want("photo", w, h, R11, 51), _want("photo", 232, 188, E5, 52),
             _nv12_want("photo", w, h, 17, 37), _nv12i_want("photo", w, h, 33, 38),
             _p016_want("photo", w, h, 80, 39), _p016_want("photo", w, h, 96, 40),
             _planar8_want("photo", w, h, 512, 35), _planar8_want("photo", w, h, 528, 36),
             _planar16_want("photo", w, h, 2112, 47), _planar16_want("photo", w, h, 2196, 48),
             _packed8_want("photo", w, h, 8192, 51), _packed8_want("photo", w, h, 8211, 52),
             _packed16_want("photo", w, h, 32832, 51), _packed16_want("photo", w, h, 32912, 52),
             _dword_want("photo", w, h, 131072, 51), _dword_want("photo", w, h, 131147, 53),
             _quad_want("photo", w, h, 524296, 51), _quad_want("photo", w, h, 524425, 54),
             _reference("photo", w, h, 8, 42), _reference("photo", w, h, 16, 43), _reference("photo", w, h, 32, 44), f16[1], bf16[1]]
    forms = {device.sample_fmt_of(i) for i in imgs}
    assert len(imgs) == len(wants) == 23 and len(forms) == 23
    with device.MixedBatch(len(imgs), image_errors=True) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        assert mb.status().tolist() == [0] * len(imgs)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check(mb, wants[::-1])
        assert mb.status().tolist() == [0] * len(imgs)


@pytest.mark.parametrize("fmt", FAMILY, ids=IDS)
def test_a_tiled_image_of_256_tiles_equals_the_references_tiled_file(fmt):
    from oracle import refprobe
    from hydrium_amd import device

    w, h = 520, 264
    want = api.encode_image(refprobe.reference_library(optimised=True), np.ascontiguousarray(_model("photo", w, h, fmt, 1234 + 17 * 6)), shift_x=0, shift_y=0)
    with device.TiledImage(w, h, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_pic("photo", w, h, fmt, 1234 + 17 * 6))
        assert bytes(ti.read()) == want


def test_the_callers_own_loop_over_lf_group_at():
    from hydrium_amd import device

    w, h = 2056, 16
    for fmt in FAMILY:
        pic = _pic("random", w, h, fmt, 9)
        with device.DeviceContext(0, 2, 0) as ctx:
            ctx.begin_frame(2)
            for tx in range(2):
                ctx.encode_lf_group_at(tx, pic.pointers(), pic.pitch, pic.pixel_stride, fmt, w, h, tx * 2048, 0, min(2048, w - tx * 2048), h, tx)
            ctx.finish_frame(2)
            got = _frame(ctx, w, h, 2)
        want = _want("random", w, h, fmt, 9)
        assert len(got) == len(want) and got == want


def test_sharded_frames_take_both():
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

    w, h, fmt = 200, 120, R11
    d, want = _dwords("random", w, h, fmt, 31), _want("random", w, h, fmt, 31)
    buf, ptrs, rs = _place(d, w + 4)
    p0 = ptrs[0]
    attempts = [(ptrs, 1, bad, "Invalid Sample Format") for bad in (8388607, 8388610, 2097152)]
    attempts += [(ptrs, ps, f, um.LAYOUT_MSG) for ps in (0, 2, 3, -1) for f in FAMILY]  # the stride
    attempts += [(p, 1, f, um.LAYOUT_MSG) for f in FAMILY for p in (
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
            if message != um.LAYOUT_MSG:
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


def test_the_host_pointer_entry_points_refuse_both():
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
        pic = _pic("photo", 33, 9, R11, 1234 + 17 * 3)  # and the context goes on
        assert _file_of(ctx, pic) == _want("photo", 33, 9, R11, 1234 + 17 * 3)


# ---- the kernel instances ----
def test_the_new_instances_footprint():
    """no more LDS than the float32 instance.  hydamd_debug_transform_footprint reports LDS and registers only: that there is no
    scratch is read off the code object's descriptor, on the CPU (test_ufloat_formats.py, private_segment_fixed_size == 0).  The
    register counts are printed and written down in DESIGN.md, not held to a number"""
    from hydrium_amd import device

    with device.DeviceContext(0, 1, 0) as ctx:
        lds32, regs32 = ctx.transform_footprint(2)
        got = {}
        for fmt in FAMILY:
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers (float32: {lds32} B, {regs32})")
            assert 0 < lds <= lds32 and regs > 0
            got[fmt] = (lds, regs)
    assert len(got) == 2
