"""CPU-only: the planar YCbCr formats of 16-bit words (HYDAMD_I010_* ... HYDAMD_I416_* and their C / L forms) where no device is
needed — the numpy model's equivalences (I010 planes are the P010 picture of the shifted, interleaved planes; bits above the depth
do not count); the per-pixel definition as the host compiler built it (csrc/hip/hydk_yuvp16.h, through the probe library, and as
plain C++ under address and UB sanitizers) against the model; the predicates, the storage-form round trip, origins, the pitch
helper and the alignment check of csrc/hyd_sample_fmt.h and csrc/hip/hydk_store.h; device.PlanarYuv16's reading of its planes;
the drop-in API's refusal; the header's constants; and what the six new instances of the transform kernel ask of a compute unit."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import chroma_model as cm
import format_dump
import format_model as fm
import p016_model as p16
import planar16_model as m16
import planar_model as plm
import yuv_model as ym
from kernel_descriptors import kernel_descriptors
from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 2), (3, 5), (33, 9), (17, 32)]
MATRIX_NAMES = ("BT709", "BT709_FULL", "BT601", "BT601_FULL")


def random_planes(sub, depth, w, h, seed=2048, full_words=False):
    """(y, u, v) of random n-bit codes, or (full_words) of random 16-bit words whatever the depth"""
    rng = np.random.default_rng(seed + 1000 * w + 10 * h + sub + 100000 * depth)
    top = 1 << (16 if full_words else m16.BITS[depth])
    ch, cw = plm.chroma_shape(sub, w, h)
    return tuple(rng.integers(0, top, s, dtype=np.uint16) for s in ((h, w), (ch, cw), (ch, cw)))


def check_definition(to_rgb):
    """to_rgb(sub, filter, depth, matrix, (y, u, v), w, h) -> (h, w, 3) uint16, held to the model on random n-bit planes, on random
    16-bit words (bits above the depth set) and on all-ones in n bits.  Shared with the on-device test."""
    for w, h in SIZES:
        for sub, filt in plm.FORMS:
            for depth in m16.DEPTHS:
                matrix = (w + h + sub + filt + depth) % 4
                fmt = m16.sample_fmt(matrix, sub, filt, depth)
                ones = tuple(np.full_like(p, (1 << m16.BITS[depth]) - 1) for p in random_planes(sub, depth, w, h))
                for planes in (random_planes(sub, depth, w, h), random_planes(sub, depth, w, h, full_words=True), ones):
                    got, want = to_rgb(sub, filt, depth, matrix, planes, w, h), m16.expected_rgb(planes, fmt)
                    assert got.dtype == np.uint16 and got.shape == want.shape == (h, w, 3)
                    wrong = np.argwhere(got != want)
                    assert wrong.size == 0, (m16.name_of(fmt), w, h, [(tuple(p), int(got[tuple(p)]), int(want[tuple(p)])) for p in wrong[:8]])


def hook(fn, *device):
    """a probe-flavour entry of the definition as to_rgb(sub, filter, depth, matrix, planes, w, h)"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(device) + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def to_rgb(sub, filt, depth, matrix, planes, w, h):
        packed = np.ascontiguousarray(np.concatenate([p.reshape(-1) for p in planes]))
        out = np.full((h, w, 3), 0xA5A5, np.uint16)
        assert fn(*device, sub, filt, depth, matrix, packed.ctypes.data, out.ctypes.data, w, h) == 0
        return out

    return to_rgb


@pytest.fixture(scope="module")
def probe():
    hbuild.build()
    return C.CDLL(hbuild.PROBE_PATH)


# ---- the definition ----
def test_i010_planes_are_the_p010_picture_of_the_shifted_interleaved_planes():
    """exact, in the model, for all three filters and all three depths: what makes the family "P01x's arithmetic on the planar
    family's geometry".  Holds on the parent too: it checks the models alone."""
    for w, h in SIZES + [(200, 120)]:
        for depth in m16.DEPTHS:
            y, u, v = random_planes(plm.S420, depth, w, h)
            pair = m16.interleave(m16.samples(depth, u), m16.samples(depth, v))
            for filt in cm.FILTERS:
                for matrix in ym.MATRICES:
                    want = p16.expected_rgb((m16.samples(depth, y), pair), p16.sample_fmt(depth, matrix, filt))
                    assert np.array_equal(m16.expected_rgb((y, u, v), m16.sample_fmt(matrix, plm.S420, filt, depth)), want)


def test_bits_above_the_depth_do_not_count():
    for w, h in SIZES:
        for sub, filt in plm.FORMS:
            for depth in (1, 2):
                planes = random_planes(sub, depth, w, h, full_words=True)
                mask = (1 << m16.BITS[depth]) - 1
                masked = tuple(p & mask for p in planes)
                assert any((p != q).any() for p, q in zip(planes, masked)) or w * h < 4
                fmt = m16.sample_fmt(1, sub, filt, depth)
                assert np.array_equal(m16.expected_rgb(planes, fmt), m16.expected_rgb(masked, fmt))
    # depth 16 takes the word as stored: an MSB-aligned 10-bit plane under I016 is the P010 picture
    y, u, v = (p << 6 for p in random_planes(plm.S420, 1, 33, 9))
    assert np.array_equal(m16.expected_rgb((y, u, v), m16.sample_fmt(0, plm.S420, 0, 3)), p16.expected_rgb((y, m16.interleave(u, v)), p16.sample_fmt(3, 0, 0)))
    # and the 4:2:2 route of the 16-bit taps is the 8-bit model's on small values
    for filt in cm.FILTERS:
        small = np.random.default_rng(7).integers(0, 256, plm.chroma_shape(plm.S422, 33, 9), dtype=np.uint16)
        assert np.array_equal(m16.upsample16(plm.S422, filt, small, 33, 9), plm.upsample(plm.S422, filt, small.astype(np.uint8), 33, 9))


def test_the_host_build_of_the_definition_equals_the_model(probe):
    check_definition(hook(probe.hydt_planar16_to_rgb_host))
    one = np.zeros(8, np.uint16)
    fn = probe.hydt_planar16_to_rgb_host
    for sub, filt, depth, matrix in ((-1, 0, 1, 0), (3, 0, 1, 0), (0, 3, 1, 0), (2, 1, 1, 0), (0, 0, 0, 0), (0, 0, 4, 0), (0, 0, 1, 4), (0, 0, 1, -1)):
        assert fn(sub, filt, depth, matrix, one.ctypes.data, one.ctypes.data, 1, 1) == api.HYD_API_ERROR


def test_the_hooks_are_in_the_probe_flavour_only():
    hbuild.build()
    probe, shipped = open(hbuild.PROBE_PATH, "rb").read(), open(hbuild.LIB_PATH, "rb").read()
    for name in (b"hydt_planar16_to_rgb_host", b"hydt_planar16_to_rgb_device"):
        assert name in probe and name not in shipped


# ---- the headers as plain C++ under address and UB sanitizers ----
@pytest.fixture(scope="module")
def program():
    return format_dump.sanitized_program("planar16_formats")


def test_the_predicates_the_round_trip_origins_pitches_and_alignment(program):
    lo, hi = -8, 4101
    got = program("geometry")
    at = 0

    def take(dtype, *shape):
        nonlocal at
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = got[at:at + n].view(dtype).reshape(shape)
        at += n
        return a

    origins, pitches, aligned = take(np.int64, 3, 2, 2, 3), take(np.int32, 2, 3, 3, 2), take(np.int32, 8)
    assert at == got.size
    rows, _ = format_dump.formats()  # hyd_fmt_describe and hydk_decode_fmt of every number, from the sanitized sample_formats program
    # (a) every predicate for -8 ... 4100, the 8-bit planar family's and this family's, read off the descriptor
    family = []
    for fmt in range(lo, hi):
        d, _ = rows[fmt]
        assert d == fm.describe(fmt), (fmt, d)
        planes = d.layout == fm.PLANES
        planar, p16 = planes and d.depth == 0, planes and d.depth > 0
        older = (int(planar), d.sub if planar else 0, d.filter if planar else 0, d.matrix if planar else 0, int(planar and d.filter != 0),
                 d.bytes, d.device, d.host)
        assert older == m16.older_row(fmt), (fmt, d)
        newer = (1, d.sub, d.filter, d.matrix, d.depth, d.bits, d.sx, d.sy, int(d.filter != 0)) if p16 else (0,) * 9
        assert newer == m16.predicate_row(fmt), (fmt, d)
        if p16:
            family.append(fmt)
            assert not planar and d.layout != fm.PAIRS and not d.is_float and not d.host, (fmt, d)  # not the 8-bit planar family's, nor NV12's, P016's, the float class's
        assert d.is_float == int(2 <= fmt <= 4)
    assert tuple(family) == tuple(sorted(m16.FAMILY)) == tuple(sorted(fm.PLANAR16_FAMILY)) and len(family) == 84 and family[0] == 2112
    per_depth = list(range(0, 12)) + list(range(16, 24)) + list(range(32, 40))
    assert family == [2048 + 64 * d + k for d in (1, 2, 3) for k in per_depth]
    for fmt in (2048, 2060, 2111, 2124, 2127, 2136, 2143, 2152, 2175, 2188, 2216, 2239, 2252, 2280, 2304, 4096, 4100, 576, 640, 1024, 1100):
        assert rows[fmt] == (fm.NOTHING, (0, -1, 0, 0, 0, 0)), fmt
    # (b) decode and encode: -8 ... 4100 round-trips exactly where a format is a device format, and nowhere else
    for fmt in range(lo, hi):
        d, (ok, back, cls, storage, matrix, variant) = rows[fmt]
        assert ok == d.device and back == (fmt if d.device else -1), (fmt, rows[fmt])
        if m16.is_format(fmt):
            filt = m16.filter_of(fmt)
            assert (cls, storage, matrix, variant) == (1, 9 + (filt != 0), m16.matrix_of(fmt) + 4 * m16.depth_of(fmt), 1024 if filt else 512), (fmt, rows[fmt])
            assert (d.filter, d.sub, d.sx, d.sy) == (filt, m16.sub_of(fmt), *plm.shifts(m16.sub_of(fmt)))  # what the job's fields are copied from
        elif not d.device:
            assert (cls, storage, matrix, variant) == (0, 0, 0, 0) and d == fm.NOTHING
    # (c) origins at (256, 512), in bytes: I010C, I212L, I416 under Y pitch +-1024 and chroma pitch +-520 words
    for k, (sx, sy) in enumerate(((1, 1), (1, 0), (0, 0))):
        for i, yp in enumerate((1024, -1024)):
            for j, cp in enumerate((520, -520)):
                chroma = 2 * ((512 >> sy) * cp + (256 >> sx))
                assert origins[k, i, j].tolist() == [2 * (512 * yp + 256), chroma, chroma], (k, i, j)
    # (d) the pitch rule at |pitch| = cw - 1, cw, cw + 1, both signs, W = 199 and 200
    assert pitches.tolist() == [[[[0, 0], [1, 1], [1, 1]]] * 3] * 2
    # (e) the alignment check: only three even addresses pass
    assert aligned.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_the_definition_stays_inside_planes_of_exactly_their_samples(program):
    """every plane a malloc of exactly its words, top-down and bottom-up: the sanitizer is the bounds check"""
    cases, blob = [], []
    for w, h in SIZES:
        for sub, filt in plm.FORMS:
            for depth in m16.DEPTHS:
                matrix = (w + sub + filt + depth) % 4
                planes = random_planes(sub, depth, w, h, 77, full_words=depth < 3 and (w + h) % 2 == 0)
                cases.append((m16.sample_fmt(matrix, sub, filt, depth), w, h, m16.expected_rgb(planes, m16.sample_fmt(matrix, sub, filt, depth))))
                blob.append(struct.pack("<IIIIII", sub, filt, depth, matrix, w, h) + b"".join(p.tobytes() for p in planes))
    assert len(cases) == 5 * 7 * 3
    got = program("planes", data=struct.pack("<I", len(cases)) + b"".join(blob)).view(np.uint16)
    at = 0
    for fmt, w, h, want in cases:
        assert np.array_equal(got[at:at + w * h * 3].reshape(h, w, 3), want), (m16.name_of(fmt), w, h)
        at += w * h * 3
    assert at == got.size


# ---- names ----
def test_the_headers_constants_are_the_python_layers():
    from hydrium_amd import device

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define (HYDAMD_I[024]1[026][CL]?_\w+) (\d+)\s*$", text, re.M)}
    want = {}
    for fmt in m16.FAMILY:
        stem = m16.public_name(fmt)
        assert getattr(device, stem) == fmt, stem
        sub, filt, m = m16.sub_of(fmt), m16.filter_of(fmt), m16.matrix_of(fmt)
        assert device.planar16_fmt(16 + m, ("420", "422", "444")[sub], cm.FILTER_NAMES[filt], m16.bits_of(fmt)) == fmt
        want["HYDAMD_" + stem] = fmt
    assert found == want and len(want) == 84
    assert device.I010_BT709 == 2112 and device.I210L_BT709_FULL == 2149 and device.I416_BT601_FULL == 2251
    assert sorted(device.PLANAR16_FAMILY) == sorted(m16.FAMILY)
    assert not set(device.PLANAR16_FAMILY) & (set(device.NV12_FAMILY) | set(device.P016_FAMILY) | set(device.PLANAR_FAMILY) | set(range(2112)))
    assert "I010" not in open(os.path.join(ROOT, "include", "libhydrium", "libhydrium.h")).read()
    fmt_h = open(os.path.join(hbuild.CSRC, "hyd_sample_fmt.h")).read()
    # the C side's reading of each number spells the public name: layout and depth the stem, the filter the infix, the matrix the suffix
    assert {"HYDAMD_" + fm.public_name(v, format_dump.described(v)): v for v in want.values()} == want
    assert all(format_dump.described(v) == fm.describe(v) and format_dump.described(v).device for v in want.values())
    message = re.search(r'#define HYD_FMT_PLANAR16_ALIGN_MSG "([^"]+)"', fmt_h).group(1)
    assert fmt_h.count('"' + message + '"') == 1 and " ".join(message.split()) in " ".join(text.replace(" *", " ").split())
    with pytest.raises(ValueError, match="depth"):
        device.planar16_fmt(16, "420", None, 8)
    # the two remarks that kept 512 + 64 * depth for deeper planes are gone
    assert "is kept for deeper planes" not in text and "is kept for deeper planes" not in fmt_h


def test_planar_yuv16_names_its_format_and_fills_a_descriptor():
    import torch
    from hydrium_amd import device

    for w, h in ((8, 8), (33, 9)):
        for fmt in m16.FAMILY:
            sub, filt, m = m16.sub_of(fmt), m16.filter_of(fmt), m16.matrix_of(fmt)
            ch, cw = plm.chroma_shape(sub, w, h)
            ybuf, ubuf, vbuf = torch.zeros(h * (w + 5), dtype=torch.int16), torch.zeros(ch * (cw + 3), dtype=torch.int16), torch.zeros(ch * (cw + 3), dtype=torch.int16)
            y, u, v = ybuf.as_strided((h, w), (w + 5, 1)), ubuf.as_strided((ch, cw), (cw + 3, 1)), vbuf.as_strided((ch, cw), (cw + 3, 1))
            pic = device.PlanarYuv16(y, u, v, 16 + m, ("420", "422", "444")[sub], cm.FILTER_NAMES[filt], m16.bits_of(fmt))
            assert isinstance(pic, device.Nv12) and device.sample_fmt_of(pic) == fmt == pic.sample_fmt and pic.shape == (h, w, 3)
            assert pic.pointers() == [ybuf.data_ptr(), ubuf.data_ptr(), vbuf.data_ptr()]
            descs, fmts = device.mixed_descriptors([pic])
            d = descs[0]
            assert fmts == [fmt] and (d.row_stride, d.pixel_stride, d.width, d.height) == (w + 5, cw + 3, w, h)  # in words
            assert [d.src[0], d.src[1], d.src[2]] == pic.pointers()
    y, u, v = torch.zeros((120, 200), dtype=torch.int16), torch.zeros((60, 100), dtype=torch.int16), torch.zeros((60, 100), dtype=torch.int16)
    pic = device.PlanarYuv16(y, u, v)
    assert device.sample_fmt_of(pic) == device.I010_BT709 == 2112  # the defaults
    rgb16 = torch.zeros((120, 200, 3), dtype=torch.int16)
    assert device.mixed_descriptors([pic, rgb16], sample_fmts="each")[1] == [2112, 1]
    with pytest.raises(ValueError, match="share one sample format"):
        device.mixed_descriptors([pic, rgb16])
    for given in (2112, 2279, 2251):  # the "disagrees with a tensor's dtype" rule covers the new numbers
        with pytest.raises(ValueError, match="disagrees with a tensor's dtype"):
            device.mixed_descriptors([rgb16], sample_fmts=[given])
    assert device.mixed_descriptors([rgb16], sample_fmts=[2048])[1] == [2048]  # no format at all: left to the library to refuse
    assert device.mixed_descriptors([rgb16], sample_fmts=[2124])[1] == [2124]


def test_planar_yuv16_refuses_what_is_no_such_picture():
    import torch
    from hydrium_amd import device

    w, h = 34, 10
    z = lambda *shape, dtype=torch.int16: torch.zeros(shape, dtype=dtype)
    y, u, v = z(h, w), z(5, 17), z(5, 17)
    assert device.PlanarYuv16(y, u, v).pixel_stride == 17
    for planes in ((y, u[:4], v[:4]), (y, u, v[:, :16])):  # a wrong chroma shape
        with pytest.raises(ValueError, match="chroma planes"):
            device.PlanarYuv16(*planes)
    with pytest.raises(ValueError, match="chroma planes"):
        device.PlanarYuv16(y, u, v, subsampling="422")
    wide = z(5, 40)
    with pytest.raises(ValueError, match="one pitch"):  # u and v strides that differ
        device.PlanarYuv16(y, u, wide[:, :17])
    with pytest.raises(ValueError, match="unit column stride"):
        device.PlanarYuv16(y, wide[:, :34:2], wide[:, :34:2])
    full = z(h, w)
    assert device.PlanarYuv16(y, full, full, subsampling="444", depth=12).sample_fmt == device.I412_BT709 == 2184
    for chroma in ("centre", "left"):
        with pytest.raises(ValueError, match="4:4:4"):
            device.PlanarYuv16(y, full, full, subsampling="444", chroma=chroma)
    with pytest.raises(ValueError):
        device.PlanarYuv16(y, u, v, chroma="bilinear")
    for depth in (8, 14, 1):
        with pytest.raises(ValueError, match="depth"):
            device.PlanarYuv16(y, u, v, depth=depth)
    for bad in (0, 80, 512, 2112):  # the matrix is one of the four
        with pytest.raises(ValueError):
            device.PlanarYuv16(y, u, v, bad)
    for planes in ((y.to(torch.uint8), u, v), (y.to(torch.float16), u, v), (y, z(5, 17, 1), v), (y, u, v.to(torch.int32))):
        with pytest.raises(ValueError, match="16-bit integers"):
            device.PlanarYuv16(*planes)
    with pytest.raises(ValueError, match="8-bit"):  # and PlanarYuv stays 8-bit only
        device.PlanarYuv(y, u, v)


def test_the_drop_in_api_refuses_the_formats():
    """they name DEVICE pixels: hyd_send_tile reads host pointers and keeps the reference's three"""
    hbuild.build()
    lib = api.Library()
    img = np.zeros((24, 8), np.uint16)
    for fmt in (2112, 2149, 2251, 2279):
        with api.Encoder(lib) as enc:
            assert enc.set_metadata(8, 8) == api.HYD_OK
            p = img.ctypes.data
            assert enc.send_tile_ptrs([p, p + 128, p + 256], 0, 0, 8, 8, -1, fmt) == api.HYD_API_ERROR
            assert enc.error_message() == "Invalid Sample Format"


# ---- the code object ----
def test_the_six_new_instances_have_symbols_of_their_own_and_keep_the_transform_kernels_contract():
    """k_transform_tokenize_yuvp16<mode, HYDK_STORE_YUVP16 | _YUVP16I>: none under an older symbol name, no scratch, and the
    co-residency line the NV12 instances are held to (26 granules of 1280 bytes of static LDS, 128 registers)"""
    res = kernel_descriptors()
    new = {k: v for k, v in res.items() if "k_transform_tokenize_yuvp16" in k}
    assert sorted(re.match(r"_Z27k_transform_tokenize_yuvp16ILi(\d)ELi(\d+)EE", k).groups() for k in new) == \
        sorted((mode, store) for mode in "012" for store in ("9", "10")), sorted(res)
    older = ("k_transform_tokenize_planar", "k_transform_tokenize_p016", "_Z20k_transform_tokenizeI")
    assert not any(o in k for k in new for o in older)
    count = lambda part: sum(part in k for k in res)
    assert (count("k_transform_tokenize_planar"), count("k_transform_tokenize_p016")) == (6, 6)
    assert sum(re.match(r"_Z20k_transform_tokenizeILi1ELi\dELi0EE", k) is not None for k in res) == 5  # RGB16: one per XYB mode
    for name, d in sorted(new.items()):
        print(name, d)
        assert d["private_segment_fixed_size"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 26 * 1280 and d["next_free_vgpr"] <= 128, (name, d)
