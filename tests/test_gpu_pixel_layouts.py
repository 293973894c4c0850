"""GPU: the RGB pixel loaders of k_transform_tokenize and the host's origin arithmetic (hyd_fmt_origin) against the oracle
and the compiled reference, for every layout of pixel_layouts.py in every sample type.  The kernel picks its loader from
address bits (pixel_layouts.loader restates the choice); test_pixel_layouts.py proves on the CPU that this matrix reaches
every loader with whole and with ragged widths.

Every buffer is filled with 0x00 or 0xFF wherever no sample of the picture lies: a read outside the picture changes the
bytes (255, 65535) or fails with "Invalid NaN Float" (0xFF.. is a NaN in float32, float16 and bfloat16).  No test needs an
access to fault, and no picture starts or ends an allocation.

Left out: the NV12 family (test_gpu_yuv_formats.py, test_gpu_chroma_filters.py) and layouts on the entry points that take
host pointers, which gather into staging on the host: the kernel never sees those strides."""
import numpy as np
import pytest

import pixel_layouts as pl
from conftest import has_gpu, reference_expected
from hydrium_amd import api
from test_gpu_mixed_batch import _md5, _reference_of
from test_pixel_layouts import host_picture, oracle_view

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ALL_TYPES = list(pl.TYPES)
FILLERS = [0x00, 0xFF]  # every case below runs with both, except the stage test (0xFF) and the far offsets (nothing is filled)
_cache = {}


def _seed(w, h):
    return 1234 + 17 * pl.SHAPES.index((w, h)) if (w, h) in pl.SHAPES else 1234


def _pictures(type_name, w, h):
    """{picture name: stored (H, W, 3) host array}: `photo`, and for uint16 the picture that straddles the sRGB knee"""
    out = {"photo": host_picture(type_name, w, h, _seed(w, h))}
    if type_name == "u16":
        knee = pl.knee_picture(w, h, seed=_seed(w, h))
        assert pl.both_sides_of_the_knee(knee)
        out["knee"] = knee
    return out


def _on_device(name, pic, filler):
    """(the buffer's tensor — keep it alive —, [three addresses], row_stride, pixel_stride) of `pic` in layout `name`"""
    import torch

    buf, offsets, rs, ps = pl.build(name, pic, filler)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 256 == 0  # what the builder's alignment claims rest on
    return t, [t.data_ptr() + o for o in offsets], rs, ps


def _code_lf_group(ctx, ptrs, rs, ps, fmt, w, h):
    ctx.begin_frame(1)
    ctx.encode_lf_group(0, ptrs, rs, ps, fmt, w, h, 0)
    ctx.finish_frame(1)
    ctx.sync()


def _first_difference(got, want):
    c, y, x = (int(v) for v in np.argwhere(got != want)[0])
    return f"first differing XYB word at (channel {c}, y {y}, x {x}): {int(got[c, y, x]):#010x}, oracle {int(want[c, y, x]):#010x}"


# ---- stage level: the XYB plane, then the sections ----
STAGE_SHAPES = [(263, 41), (264, 40)]


@pytest.mark.parametrize("type_name,linear", [("u8", 0), ("u16", 0), ("u16", 1), ("f32", 0)],
                         ids=["u8", "u16", "u16-linear-light", "f32"])
def test_every_layout_leaves_the_oracles_xyb_plane_and_sections(type_name, linear):
    from hydrium_amd import device
    from oracle import binding as orc

    fmt = pl.TYPES[type_name]
    failures = []
    with device.DeviceContext(0, 1, linear, debug_planes=True) as ctx:
        # ragged by 7, and whole blocks: only at a width whose tight rows are dwords does `bgr` hinge on the pointer test
        for (w, h), (pname, pic) in [(wh, p) for wh in STAGE_SHAPES for p in _pictures(type_name, *wh).items()]:
            res, _ = orc.encode_lf_group(pic, linear_light=linear)
            want_xyb = res.xyb.view(np.uint32)
            for name in pl.layout_names(pic.dtype.itemsize):
                t, ptrs, rs, ps = _on_device(name, pic, 0xFF)
                where = f"{pname} {w}x{h}, {name} ({pl.loader(fmt, ptrs, rs, ps)})"
                try:
                    _code_lf_group(ctx, ptrs, rs, ps, fmt, w, h)
                except device.DeviceError as e:
                    failures.append(f"{where}: {e}")
                    continue
                xyb = ctx.read_debug_plane(0, res.stride, res.vbh * 8).view(np.uint32)
                if not np.array_equal(xyb, want_xyb):
                    failures.append(f"{where}: {_first_difference(xyb, want_xyb)}")
                elif ctx.read_payload() != res.stream:
                    failures.append(f"{where}: the XYB plane is the oracle's, the sections are not")
                del t
    assert not failures, "\n".join(failures)


# ---- file level: every layout x shape of a type in one mixed batch ----
@pytest.mark.parametrize("filler", FILLERS, ids=["zeros", "ones"])
@pytest.mark.parametrize("type_name", ALL_TYPES)
def test_every_layout_and_shape_gives_the_reference_file(type_name, filler):
    from hydrium_amd import device

    fmt = pl.TYPES[type_name]
    descs, wants, names, keep, distinct = [], [], [], [], {}
    for w, h in pl.SHAPES:
        for pname, pic in _pictures(type_name, w, h).items():
            want = _reference_of(("layouts", type_name, pname, w, h), oracle_view(type_name, pic))
            distinct[(pname, w, h)] = want
            for name in pl.layout_names(pic.dtype.itemsize):
                t, ptrs, rs, ps = _on_device(name, pic, filler)
                keep.append(t)
                descs.append((ptrs, rs, ps, w, h))
                wants.append(want)
                names.append(f"{pname} {w}x{h}, {name} ({pl.loader(fmt, ptrs, rs, ps)})")
    assert len(set(distinct.values())) == len(distinct)  # distinct pictures, distinct files: no file can stand in for another
    with device.MixedBatch(len(descs)) as mb:
        mb.encode(descs, sample_fmt=fmt)
        total = mb.result()
        files = [bytes(f) for f in mb.read()]
    wrong = [f"{n}: {_md5(g)} ({len(g)} bytes), reference {_md5(x)} ({len(x)} bytes)" for n, g, x in zip(names, files, wants) if g != x]
    assert not wrong, "\n".join(wrong)
    assert len(files) == len(wants) and total == sum(map(len, wants))


# ---- origins: LF groups other than (0, 0) of a generic layout ----
BIG_W, BIG_H = 2056, 2052  # four LF groups; those at (1, 0), (0, 1) and (1, 1) are slivers
ORIGIN_TYPES = ["u8", "u16", "f32"]
ORIGIN_LAYOUTS = ["planes", "rgba", "bgr", "negative pitch, dword rows", "negative pitch, odd rows"]


def _big_picture(type_name):
    """the 2056 x 2052 photo of a type on the host (generated on the device: the host generator takes seconds); made once"""
    from hydrium_amd import synth

    key = ("big", type_name)
    if key not in _cache:
        if type_name == "u8":
            a = synth.make_image("photo", BIG_W, BIG_H, 8, 99, device="cuda").cpu().numpy()
        else:
            a = synth.make_image("photo", BIG_W, BIG_H, 16, 99, device="cuda").cpu().numpy().view(np.uint16)
            if type_name == "f32":  # synth.make_image_f32's arithmetic
                a = (a.astype(np.float32) * np.float32(1.0 / 65535.0)).astype(np.float32)
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def _big_oracle(type_name):
    """the oracle's results for the four LF groups in send order (raster), the running alphabet maximum carried along"""
    from oracle import binding as orc

    key = ("big oracle", type_name)
    if key not in _cache:
        out, mx = [], 0
        for ty in range(2):
            for tx in range(2):
                res, mx = orc.encode_lf_group(_big_picture(type_name), tx, ty, max_alphabet_size=mx)
                out.append(res.stream)
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("name", ORIGIN_LAYOUTS, ids=[n.replace(", ", "_").replace(" ", "_") for n in ORIGIN_LAYOUTS])
@pytest.mark.parametrize("type_name", ORIGIN_TYPES)
def test_lf_groups_off_the_origin_of_a_generic_layout(type_name, name):
    from hydrium_amd import device

    pic = _big_picture(type_name)
    streams = _big_oracle(type_name)
    with device.DeviceContext(0, 4, 0) as ctx:
        for filler in FILLERS:
            t, ptrs, rs, ps = _on_device(name, pic, filler)
            ctx.encode_image(ptrs, rs, ps, pl.TYPES[type_name], BIG_W, BIG_H)
            ctx.sync()
            payload = ctx.read_payload()
            at = 0
            for slot, want in enumerate(streams):
                got = payload[at:at + len(want)]
                assert len(want) > 0 and _md5(got) == _md5(want), \
                    f"filler {filler:#04x}: LF group ({slot % 2}, {slot // 2}), sent as number {slot}, {len(want)} bytes"
                at += len(want)
            assert at == len(payload) and len(streams) == 4  # four LF groups' sections and nothing else


@pytest.mark.parametrize("type_name", ORIGIN_TYPES)
def test_a_picture_of_four_lf_groups_in_planes_through_a_mixed_batch(type_name):
    from hydrium_amd import device

    pic = _big_picture(type_name)
    want = _reference_of(("layouts big", type_name), pic)
    with device.MixedBatch(1, max_lf_groups=4) as mb:
        for filler in FILLERS:
            t, ptrs, rs, ps = _on_device("planes", pic, filler)
            mb.encode([(ptrs, rs, ps, BIG_W, BIG_H)], sample_fmt=pl.TYPES[type_name])
            got = bytes(mb.read(0))
            assert got == want, (filler, _md5(got), _md5(want), len(got), len(want))


# ---- the other entry points that read device pixels (their uint8 cases exist: test_gpu_tiled_device.py, test_gpu_batch_files.py) ----
@pytest.mark.parametrize("type_name", ["u16", "f32"])
def test_planes_and_rgba_through_a_tiled_image(type_name):
    from hydrium_amd import device
    from oracle import refprobe

    assert reference_expected()
    w, h = 520, 300
    pic = host_picture(type_name, w, h, 77)
    want = api.encode_image(refprobe.reference_library(optimised=True), pic, shift_x=0, shift_y=0)
    with device.TiledImage(w, h, 0, 0) as ti:
        for name, filler in [(n, f) for n in ("planes", "rgba") for f in FILLERS]:
            t, ptrs, rs, ps = _on_device(name, pic, filler)
            ti.encode(ptrs, rs, ps, pl.TYPES[type_name])
            got = bytes(ti.read())
            assert got == want, (name, filler, _md5(got), _md5(want), len(got), len(want))


@pytest.mark.parametrize("type_name", ["u16", "f32"])
def test_planes_and_rgba_through_a_frame_batch(type_name):
    from hydrium_amd import device

    w, h = 520, 264
    pics = [host_picture(type_name, w, h, s) for s in (78, 79)]
    wants = [_reference_of(("layouts frames", type_name, s), p) for s, p in zip((78, 79), pics)]
    assert wants[0] != wants[1]
    with device.FrameBatch(w, h, 2) as fb:
        for name, filler in [(n, f) for n in ("planes", "rgba") for f in FILLERS]:
            laid = [_on_device(name, p, filler) for p in pics]
            assert laid[0][2:] == laid[1][2:]
            fb.encode([l[1] for l in laid], laid[0][2], laid[0][3], pl.TYPES[type_name])
            got = [bytes(f) for f in fb.read()]
            assert got == wants, (name, filler, [_md5(g) for g in got], [_md5(x) for x in wants])


# ---- byte offsets beyond 2^31 and 2^32 ----
def test_rows_and_planes_gigabytes_apart():
    """A 72 x 40 picture whose rows lie 2^27 bytes apart (the last ones beyond 2^32 bytes from src[0]), at a pitch that
    keeps the packed rows, one four bytes longer, one that is no dword multiple (per sample), and the first one negated
    from the last row; then three planes 2^31 + 4096 bytes apart.  Only the picture's bytes are written; the rest of the
    5.4 GB is whatever the allocation holds."""
    import torch
    from hydrium_amd import device
    from oracle import binding as orc

    w, h = 72, 40
    far = 1 << 27
    size = h * far
    try:
        buf = torch.empty(size, dtype=torch.uint8, device="cuda")
    except torch.cuda.OutOfMemoryError:
        free, total = torch.cuda.mem_get_info()
        pytest.skip(f"no {size >> 20} MiB in one allocation: {free >> 20} MiB of {total >> 20} MiB are free")
    try:
        base = buf.data_ptr()
        assert base % 256 == 0
        failures = []
        with device.DeviceContext(0, 1, 0) as ctx:
            for type_name in ("u8", "u16"):
                fmt, s = pl.TYPES[type_name], pl.SAMPLE_BYTES[pl.TYPES[type_name]]
                pic = host_picture(type_name, w, h, 55)
                want = orc.encode_lf_group(pic)[0].stream
                rows = torch.from_numpy(pic.copy().view(np.uint8).reshape(h, w * 3 * s)).cuda()
                planes = torch.from_numpy(np.ascontiguousarray(pic.transpose(2, 0, 1)).view(np.uint8).reshape(3, h, w * s)).cuda()
                cases = [("pitch 2^27", far, 1, "packed"), ("pitch 2^27 + 4", far + 4, 1, "packed"),
                         (f"pitch 2^27 + {s}", far + s, 1, "per sample"), ("pitch -2^27", far, -1, "packed")]
                for label, pitch, sign, which in cases:
                    assert 256 + (h - 1) * pitch + w * 3 * s <= size and (h - 1) * pitch > 1 << 32
                    buf.as_strided((h, w * 3 * s), (pitch, 1), 256).copy_(rows if sign > 0 else rows.flip(0))
                    first = base + 256 + ((h - 1) * pitch if sign < 0 else 0)
                    ptrs, rs = [first, first + s, first + 2 * s], sign * pitch // s
                    assert rs * s == sign * pitch and pl.loader(fmt, ptrs, rs, 3) == which
                    torch.cuda.synchronize()
                    _code_lf_group(ctx, ptrs, rs, 3, fmt, w, h)
                    if ctx.read_payload() != want:
                        failures.append(f"{type_name}, {label} ({which})")
                apart = (1 << 31) + 4096
                assert 256 + 2 * apart + h * w * s <= size
                buf.as_strided((3, h, w * s), (apart, w * s, 1), 256).copy_(planes)
                torch.cuda.synchronize()
                ptrs = [base + 256 + c * apart for c in range(3)]
                assert pl.loader(fmt, ptrs, w, 1) == "per sample"
                _code_lf_group(ctx, ptrs, w, 1, fmt, w, h)
                if ctx.read_payload() != want:
                    failures.append(f"{type_name}, planes 2^31 + 4096 bytes apart")
        assert not failures, failures
    finally:
        del buf
        torch.cuda.empty_cache()
