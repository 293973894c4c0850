"""GPU: packed 4:2:2 YCbCr pictures of 16-bit words from device memory (HYDAMD_Y210_*, HYDAMD_Y212_*, HYDAMD_Y216_* and their C / L
forms; four word orders by the pointers) on every entry point that reads device pixels.  A pixel is a 16-bit RGB pixel right after
the load: every file is compared whole with what the compiled reference writes for the HYD_UINT16 picture the numpy model of the
definition (packed16_model.py) makes of the same words.  Every surface sits in an allocation that ends with the last group of its
last row, or between 0x5A bytes."""
import ctypes as C

import numpy as np
import pytest

import chroma_model as cm
import packed16_model as p6
import planar16_model as m16
import planar_model as plm
import yuv_model as ym
from conftest import has_gpu
from hydrium_amd import api, build as hbuild
from test_gpu_chroma_filters import _frame_of, _nv12 as _nv12i, _want as _nv12i_want
from test_gpu_half_formats import _half
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference, _reference_of
from test_gpu_p016_formats import _p016, _want as _p016_want
from test_gpu_packed_formats import _packed as _packed8, _want as _packed8_want
from test_gpu_planar16_formats import _device_picture as _planar16_picture, _planar as _planar16, _want as _planar16_want
from test_gpu_planar_formats import _planar as _planar8, _want as _planar8_want
from test_gpu_yuv_formats import _nv12, _want as _nv12_want
from test_packed16_formats import check_definition, hook

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

FAMILY = sorted(p6.FAMILY)
Y210, Y210C, Y210L, Y212C, Y216, Y216C, Y216L = 32832, 32848, 32866, 32913, 32960, 32976, 32994  # what the layout and entry-point tests use
NO_FORMAT = (32767, 32768, 32831, 32836, 32880, 33024)
SHARDED_MSG = "interpolated chroma is not sharded"
_cache = {}


def _planes(kind, w, h, fmt, seed=1234):
    """host (y (h, w), u (h, cw), v (h, cw)) uint16 of one picture, MSB-aligned words: a photograph made 4:2:2 at the format's depth
    and matrix, or crafted content as tests/test_gpu_p016_formats.py builds it; the same planes for every filter and word order"""
    from hydrium_amd import synth

    d, m = p6.depth_of(fmt), p6.matrix_of(fmt)
    key = ("planes", kind, w, h, d, m, seed)
    if key not in _cache:
        cs = (h, (w + 1) // 2)
        rng = np.random.default_rng(seed)
        shift = 16 - p6.BITS[d]
        photo = lambda: tuple(p << shift for p in m16.planes_of_rgb(synth.make_image("photo", w, h, 16, seed), d, m, plm.S422))
        if kind == "photo":  # valid n-bit codes, the low bits zero
            y, u, v = photo()
        elif kind == "random":  # full 16-bit words whatever the depth: the low bits count as stored; most pixels clamp
            y, u, v = (rng.integers(0, 65536, s, dtype=np.uint16) for s in ((h, w), cs, cs))
        elif kind in ("zeros", "ones"):
            y, u, v = (np.full(s, 0 if kind == "zeros" else 65535, np.uint16) for s in ((h, w), cs, cs))
        elif kind == "out of range":  # luma below 4096 and above 60160, chroma beyond 4096 ... 61440, around a photograph's chroma
            y, u, v = photo()
            y = np.where(rng.integers(0, 2, (h, w)) == 0, rng.integers(0, 4096, (h, w)), rng.integers(60161, 65536, (h, w))).astype(np.uint16)
            u, v = u.copy(), v.copy()
            for p in (u, v):
                p[:, ::3] = rng.choice(np.array([0, 1280, 4095, 61441, 64000, 65535], np.uint16), p[:, ::3].shape)
        elif kind == "random chroma":  # smooth luma under random chroma: tells the filters, and every neighbour they read, apart
            y = ((np.add.outer(np.arange(h) * 2, np.arange(w) * 3) // 7 + rng.integers(0, 4, (h, w))) % 256 * 257).astype(np.uint16)
            u, v = (rng.integers(16384, 49152, cs, dtype=np.uint16) for _ in range(2))
        else:
            raise KeyError(kind)
        y, u, v = (np.ascontiguousarray(p, np.uint16) for p in (y, u, v))
        for p in (y, u, v):
            p.setflags(write=False)
        _cache[key] = (y, u, v)
    return _cache[key]


def _rows(kind, w, h, fmt, order="yuyv", seed=1234):
    key = ("rows", kind, w, h, p6.depth_of(fmt), p6.matrix_of(fmt), order, seed)
    if key not in _cache:
        _cache[key] = p6.interleave(_planes(kind, w, h, fmt, seed), order, w)
        _cache[key].setflags(write=False)
    return _cache[key]


def _model(kind, w, h, fmt, seed=1234):
    """the picture every word order of those planes stands for"""
    key = ("model", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = p6.expected_rgb(_rows(kind, w, h, fmt, "yuyv", seed), "yuyv", w, fmt)
        _cache[key].setflags(write=False)
    return _cache[key]


def _want(kind, w, h, fmt, seed=1234):
    """the reference's file for the model's RGB16 picture of those words; made once"""
    return _reference_of(("packed16", kind, w, h, fmt, seed), _model(kind, w, h, fmt, seed))


def _tiled_want(kind, w, h, fmt, seed=1234):
    from oracle import refprobe

    key = ("tiled", kind, w, h, fmt, seed)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), _model(kind, w, h, fmt, seed), shift_x=0, shift_y=0)
    return _cache[key]


def _surface(rows, pitch):
    """the rows in an allocation of its own that ENDS with the last group of the last row, 0x5A5A in the pitch's slack; pitch in words"""
    import torch

    h, row = rows.shape
    host = np.full(pitch * (h - 1) + row, 0x5A5A, np.uint16)
    for r in range(h):
        host[pitch * r: pitch * r + row] = rows[r]
    return torch.from_numpy(host.view(np.int16)).cuda().as_strided((h, row), (pitch, 1))


def _picture(rows, w, fmt, order="yuyv", pitch=None):
    from hydrium_amd import device

    pic = device.PackedYuv16(_surface(rows, pitch or rows.shape[1]), w, 16 + p6.matrix_of(fmt), order, cm.FILTER_NAMES[p6.filter_of(fmt)], p6.bits_of(fmt))
    assert pic.sample_fmt == fmt
    return pic


def _packed(kind, w, h, fmt, order="yuyv", seed=1234, pitch=None):
    """device.PackedYuv16 of the picture; pitch: the row itself (a multiple of 4 words), or as given; made once"""
    import torch

    key = ("dev", kind, w, h, fmt, order, seed, pitch)
    if key not in _cache:
        _cache[key] = _picture(_rows(kind, w, h, fmt, order, seed), w, fmt, order, pitch)
        torch.cuda.synchronize()
    return _cache[key]


def _pointers(base, order):
    y = base + 2 * p6.y_offset(order)
    du, dv = p6.ORDERS[order]
    return [y, y + 2 * du, y + 2 * dv]


def _place(rows, order, pitch, shift=0, flip=False):
    """the surface at a bare address between 0x5A bytes: (buffer to keep alive, [Y, U, V addresses], row stride in words).  pitch in
    words; shift moves the first group by that many BYTES (even) from a 256-byte boundary; flip stores the rows bottom-up: a
    negative pitch"""
    import torch

    assert shift % 2 == 0
    h, row = rows.shape
    host = np.full((32 + pitch * (h + 2) + 127) // 128 * 128, 0x5A5A, np.uint16)
    at = 128 + shift // 2  # in words: 256 bytes in
    for r in range(h):
        o = at + pitch * (h - 1 - r if flip else r)
        host[o: o + row] = rows[r]
    buf = torch.from_numpy(host.view(np.int16)).cuda()
    assert buf.data_ptr() % 256 == 0
    first = buf.data_ptr() + 2 * (at + (pitch * (h - 1) if flip else 0))
    return buf, _pointers(first, order), -pitch if flip else pitch


# ---- the definition on the device ----
def test_the_device_build_of_the_definition_equals_the_model():
    check_definition(hook(C.CDLL(hbuild.PROBE_PATH).hydt_packed16_to_rgb_device, 0), widths=(1, 7, 8, 33))


# ---- reference parity ----
SIZES = [(1, 5), (7, 3), (8, 8), (33, 9), (200, 120), (256, 256), (257, 255), (520, 264)]


@pytest.mark.parametrize("fmt", FAMILY, ids=[p6.name_of(f) for f in FAMILY])
def test_photographs_of_eight_sizes_equal_the_reference(fmt):
    from hydrium_amd import device

    cases = [(w, h, 1234 + 17 * k) for k, (w, h) in enumerate(SIZES)]
    order = p6.ORDER_NAMES[fmt % 4]  # a word order per matrix: the orders themselves have a test of their own
    pics = [_packed("photo", w, h, fmt, order, s) for w, h, s in cases]
    wants = [_want("photo", w, h, fmt, s) for w, h, s in cases]
    assert len(set(wants)) == len(SIZES)
    with device.MixedBatch(len(SIZES)) as mb:
        mb.encode(pics)
        _check_on_device(mb, wants)


EXTREME = [p6.sample_fmt(m, f, d) for d, f, m in ((1, 0, 0), (1, 1, 1), (1, 2, 2), (2, 0, 3), (2, 1, 0), (2, 2, 1), (3, 0, 2), (3, 1, 3), (3, 2, 0))]


@pytest.mark.parametrize("fmt", EXTREME, ids=[p6.name_of(f) for f in EXTREME])
def test_extreme_content_equals_the_reference(fmt):
    """one format per depth x filter, every matrix among them: random full words under every depth (the low bits are used as
    stored), zeros, all-ones and, for limited range, samples outside the nominal range"""
    from hydrium_amd import device

    kinds = ["random", "zeros", "ones"] + (["out of range"] if ym.LIMITED[p6.matrix_of(fmt)] else [])
    y, u, v = _planes("random", 264, 200, fmt)
    low = (1 << (16 - p6.bits_of(fmt))) - 1
    if low:
        assert (y & low != 0).mean() > 0.9 and (u & low != 0).mean() > 0.9  # low bits set in most
    if p6.filter_of(fmt) == cm.NEAREST:
        rgb = _model("random", 264, 200, fmt)
        assert ((rgb == 0) | (rgb == 65535)).any(-1).mean() > 0.5
    if "out of range" in kinds:
        y = _planes("out of range", 264, 200, fmt)[0]
        assert ((y < 4096) | (y > 60160)).all()
    with device.MixedBatch(len(kinds)) as mb:
        mb.encode([_packed(k, 264, 200, fmt, p6.ORDER_NAMES[(fmt >> 4) % 4]) for k in kinds])
        _check(mb, [_want(k, 264, 200, fmt) for k in kinds])


# ---- the loaders ----
@pytest.mark.parametrize("fmt,order", [(Y210, "yuyv"), (Y216C, "uyvy")], ids=["y210-yuyv", "y216c-uyvy"])
def test_the_dword_loader_and_the_word_loader_give_one_file(fmt, order):
    """200 x 120 random words with the first group at every even residue modulo 16 — both sides of whatever alignment the dword
    path asks for — and pitches that keep and that lose it"""
    from hydrium_amd import device

    w, h = 200, 120
    rows, want = _rows("random", w, h, fmt, order, 77), _want("random", w, h, fmt, 77)
    placed = {f"first group at {s} mod 16": _place(rows, order, 400, shift=s) for s in range(0, 16, 2)}
    placed.update({
        "a pitch of an odd number of words": _place(rows, order, 403),
        "a pitch of an even number of words that is no multiple of 8": _place(rows, order, 402),
        "a pitch larger than the row": _place(rows, order, 432),
        "a negative pitch": _place(rows, order, 400, flip=True),
        "a negative pitch of an odd number of words, first group at 6 mod 16": _place(rows, order, 401, shift=6, flip=True),
    })
    group = lambda p: (p[1][0] - 2 * p6.y_offset(order)) % 16  # where the first group starts
    assert [group(placed[f"first group at {s} mod 16"]) for s in range(0, 16, 2)] == list(range(0, 16, 2))
    assert placed["a pitch of an odd number of words"][2] % 2 == 1 and placed["a negative pitch"][2] == -400
    with device.MixedBatch(len(placed) + 1) as mb:
        mb.encode([(ptrs, rs, 2, w, h) for _, ptrs, rs in placed.values()] + [_packed("random", w, h, fmt, order, 77)], sample_fmt=fmt)
        _check(mb, [want] * (len(placed) + 1))
    del placed


# ---- word orders ----
@pytest.mark.parametrize("fmt", [Y210, Y212C, Y216L], ids=[p6.name_of(f) for f in (Y210, Y212C, Y216L)])
def test_the_four_word_orders_of_the_same_planes_give_one_file(fmt):
    from hydrium_amd import device

    w, h = 232, 188
    want = _want("random chroma", w, h, fmt, 21)
    pics = [_packed("random chroma", w, h, fmt, order, 21) for order in p6.ORDER_NAMES]
    assert len({bytes(_rows("random chroma", w, h, fmt, order, 21)) for order in p6.ORDER_NAMES}) == 4
    # U and V swapped under the same order (Y U Y V words read as Y V Y U): the model of the swapped reading, and another file
    swapped = _reference_of(("packed16 swapped", fmt), p6.expected_rgb(_rows("random chroma", w, h, fmt, "yuyv", 21), "yvyu", w, fmt))
    assert swapped != want
    yuyv = pics[0]
    base = yuyv.surface.data_ptr()
    with device.MixedBatch(5) as mb:  # pictures of different word orders in one launch group
        mb.encode(pics + [(_pointers(base, "yvyu"), yuyv.pitch, 2, w, h)], sample_fmt=fmt)
        _check(mb, [want] * 4 + [swapped])
        mb.encode(pics[::-1], sample_fmts="each")  # hydamd_encode_mixed_formats
        _check(mb, [want] * 4)


# ---- identities ----
@pytest.mark.parametrize("filt", cm.FILTERS, ids=[cm.FILTER_NAMES[f] for f in cm.FILTERS])
def test_the_file_is_the_planar_formats_for_the_same_samples(filt):
    """a Y216 picture and its de-interleaved words as I216; a Y210 picture whose low six bits are zero and the words >> 6 as I210;
    and the same Y210 words with the low bits set: another file, the model's"""
    from hydrium_amd import device

    w, h = 264, 200
    y216, y210 = p6.sample_fmt(3, filt, 3), p6.sample_fmt(2, filt, 1)
    words = _rows("random", w, h, y216, "vyuy", 61)
    clean = _rows("photo", w, h, y210, "uyvy", 62)
    assert not (clean & 0x3F).any()
    rng = np.random.default_rng(63)
    dirty = clean | rng.integers(1, 64, clean.shape, dtype=np.uint16)
    pics = [_picture(words, w, y216, "vyuy"), _planar16_picture(p6.deinterleave(words, "vyuy", w), p6.as_i2xx(y216)),
            _picture(clean, w, y210, "uyvy"), _planar16_picture(tuple(p >> 6 for p in p6.deinterleave(clean, "uyvy", w)), p6.as_i2xx(y210)),
            _picture(dirty, w, y210, "uyvy")]
    assert [p.sample_fmt for p in pics] == [y216, 2240 + 4 + 16 * filt + 3, y210, 2112 + 4 + 16 * filt + 2, y210]
    with device.MixedBatch(len(pics)) as mb:
        mb.encode(pics, sample_fmts="each")
        files = [bytes(f) for f in mb.read()]
    assert files[0] == files[1] == _reference_of(("packed16 words", filt), p6.expected_rgb(words, "vyuy", w, y216))
    assert files[2] == files[3] == _want("photo", w, h, y210, 62)
    assert files[4] != files[2]
    assert files[4] == _reference_of(("packed16 dirty", filt), p6.expected_rgb(dirty, "uyvy", w, y210))


# ---- entry points ----
def test_encode_image_and_a_frame_batch_of_three_frames():
    import torch
    from hydrium_amd import device

    w, h = 264, 200
    for fmt, order in ((Y210, "yvyu"), (Y212C, "yuyv"), (Y216L, "uyvy")):
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


def test_packed_words_beside_every_other_form_in_one_launch():
    """one picture of each of the seventeen forms the transform kernel has an instance for, 27 x 19 with pitches rounded up to a
    dword: an interpolated form's blocks 1 and 2 take the dword window, block 0 (the picture's first chroma column) and block 3
    (ragged, odd width) the edge fill; forward and reversed"""
    import torch
    from hydrium_amd import device

    w, h, pitch = 27, 19, 28
    f16, bf16 = _half("photo", w, h, "float16", 45), _half("photo", w, h, "bfloat16", 46)
    rgb16 = _image("photo", w, h, 16, 43)[0]
    imgs = [_packed("photo", w, h, Y210, "vyuy", 51), _packed("photo", w, h, Y212C, "yuyv", 52), _packed("photo", 232, 188, Y216L, "uyvy", 53),
            _packed8("photo", w, h, 8192, "vyuy", 51), _packed8("photo", w, h, 8211, "yuyv", 52),
            _planar8("photo", w, h, 512, 35), _planar8("photo", w, h, 528, 36), _nv12("photo", w, h, 17, 37, pitch),
            _nv12i("photo", w, h, 33, 38, pitch), _p016("photo", w, h, 80, 39, pitch), _p016("photo", w, h, 96, 40, pitch),
            _planar16("photo", w, h, 2112, 47), _planar16("photo", w, h, 2196, 48),
            _image("photo", w, h, 8, 42)[0], rgb16 if rgb16.dtype == torch.int16 else rgb16.view(torch.int16),
            _image("photo", w, h, 32, 44)[0], f16[0], bf16[0]]
    wants = [_want("photo", w, h, Y210, 51), _want("photo", w, h, Y212C, 52), _want("photo", 232, 188, Y216L, 53),
             _packed8_want("photo", w, h, 8192, 51), _packed8_want("photo", w, h, 8211, 52),
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
@pytest.mark.parametrize("fmt", [Y210C, Y216L], ids=[p6.name_of(Y210C), p6.name_of(Y216L)])
def test_chroma_is_continuous_across_the_tiles_of_a_tiled_image(fmt):
    from hydrium_amd import device

    w, h = 520, 300
    rows, whole = _rows("random chroma", w, h, fmt, "yuyv", 5), _model("random chroma", w, h, fmt, 5)
    alone = p6.expected_rgb(np.ascontiguousarray(rows[:256, :512]), "yuyv", 256, fmt)
    assert not np.array_equal(alone, whole[:256, :256])  # the first tile alone clamps where the picture reads on
    with device.TiledImage(w, h, 0, 0) as ti:  # tiles of 256 x 256, every one a frame
        ti.encode(_packed("random chroma", w, h, fmt, "yuyv", 5))
        assert bytes(ti.read()) == _tiled_want("random chroma", w, h, fmt, 5)


@pytest.mark.parametrize("fmt,order", [(Y212C, "uyvy"), (Y210L, "yuyv")], ids=["y212c-uyvy", "y210l-yuyv"])
def test_across_lf_groups_through_lf_group_at(fmt, order):
    """the caller's own loop over hydamd_encode_lf_group_at: two LF groups side by side (4:2:2 has no vertical taps, so a tall
    picture tells nothing)"""
    from hydrium_amd import device

    w, h = 2056, 264
    rows, whole = _rows("random chroma", w, h, fmt, order, 9), _model("random chroma", w, h, fmt, 9)
    first = p6.expected_rgb(np.ascontiguousarray(rows[:, :4096]), order, 2048, fmt)
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
        for fmt, order in ((Y212C, "uyvy"), (Y210L, "yuyv")):
            wide = _packed("random chroma", w, h, fmt, order, 9)
            with pytest.raises(device.DeviceError, match=SHARDED_MSG) as e:
                m.encode([wide, wide])
            assert e.value.code == api.HYD_API_ERROR
        for fmt, order in ((Y210, "vyuy"), (32963, "yuyv")):
            near = _packed("random chroma", w, h, fmt, order, 9)
            m.encode([near, near])
            assert bytes(m.read()) == _want("random chroma", w, h, fmt, 9)


# ---- refusals ----
def test_what_is_no_format_or_no_layout_is_refused_and_the_object_stays_usable():
    from hydrium_amd import device

    w, h, fmt = 200, 120, Y210C
    rows, want = _rows("random chroma", w, h, fmt, "yuyv", 31), _want("random chroma", w, h, fmt, 31)
    buf, ptrs, rs = _place(rows, "yuyv", 400)
    y = ptrs[0]
    attempts = [(ptrs, 2, bad, "Invalid Sample Format") for bad in NO_FORMAT]
    attempts += [(ptrs, ps, f, p6.LAYOUT_MSG) for ps in (1, 4) for f in (Y210, Y210C)]  # the stride
    attempts += [(p, 2, f, p6.LAYOUT_MSG) for f in (Y210, Y216L) for p in (
        [y, y - 2, y - 6], [y, y + 2, y + 2], [y, y + 40000, y + 80000],  # the order
        [y, y + 1, y + 3], [y + 1, y + 3, y + 7], [y, y + 2, y + 7])]       # bytes for words; an odd address; an odd V
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
            if message != p6.LAYOUT_MSG:
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
        for fmt in (Y210, Y216C):
            lds, regs = ctx.transform_footprint(fmt)
            print(f"transform footprint, format {fmt}: {lds} B of LDS, {regs} registers")
            assert 0 < lds <= 26 * 1280 and 0 < regs <= 128
