"""CPU-only: the layout table of pixel_layouts.py before anything on the GPU trusts it.  For every layout, sample type and
shape of the GPU matrix: the builder is right on its own; the oracle, reading the built buffer through the layout's
pointers and strides, gives the stream it gives for the contiguous picture; and the model of the kernel's loader choice
says that the matrix reaches every loader the way test_gpu_pixel_layouts.py relies on."""
import numpy as np
import pytest

import pixel_layouts as pl
from hydrium_amd import synth

TYPE_NAMES = list(pl.TYPES)
FILLERS = [0x00, 0xFF]
_cache = {}


def host_picture(type_name, w, h, seed):
    """the contiguous (H, W, 3) picture of a type as stored (half types: uint16 bit patterns), read-only; made once"""
    key = (type_name, w, h, seed)
    if key not in _cache:
        if type_name == "u8":
            a = synth.make_image("photo", w, h, 8, seed)
        elif type_name == "u16":
            a = synth.make_image("photo", w, h, 16, seed)
        else:
            a = synth.make_image_f32("photo", w, h, seed)
            if type_name == "f16":
                a = a.astype(np.float16).view(np.uint16)
            elif type_name == "bf16":  # truncation: any bfloat16 picture serves
                a = (a.view(np.uint32) >> 16).astype(np.uint16)
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def oracle_view(type_name, pic):
    """what the oracle codes for a stored picture: itself, or a half picture's exact float32 widening"""
    return pl.widen_half_bits(pic, type_name) if type_name in ("f16", "bf16") else pic


def _cases():
    return [(t, name, w, h) for t in TYPE_NAMES for name in pl.layout_names(pl.SAMPLE_BYTES[pl.TYPES[t]]) for w, h in pl.SHAPES]


def _id(case):
    return f"{case[0]}-{case[1].replace(', ', '_').replace(' ', '_')}-{case[2]}x{case[3]}"


@pytest.mark.parametrize("filler", FILLERS, ids=["zeros", "ones"])
@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_the_builder_places_the_picture_and_nothing_else(case, filler):
    type_name, name, w, h = case
    pic = host_picture(type_name, w, h, 1234)
    buf, offsets, rs, ps = pl.build(name, pic, filler)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and len(offsets) == 3
    back, used = pl.gather(buf, offsets, rs, ps, w, h, pic.dtype)
    assert np.array_equal(back, pic)
    assert used.sum() == pic.nbytes  # no two samples share a byte
    assert (buf[~used] == filler).all()
    assert not used[:pl.MARGIN].any() and not used[-pl.MARGIN:].any()
    s = pic.dtype.itemsize
    assert all(o % s == 0 for o in offsets)  # sample-aligned wherever the base is


def test_the_layouts_are_what_their_names_say():
    for type_name in TYPE_NAMES:
        s = pl.SAMPLE_BYTES[pl.TYPES[type_name]]
        w, h = 263, 41
        pic = host_picture(type_name, w, h, 1234)
        got = {name: pl.build(name, pic, 0)[1:] for name in pl.layout_names(s)}
        o, rs, ps = got["interleaved"]
        assert (o, rs, ps) == ([pl.MARGIN, pl.MARGIN + s, pl.MARGIN + 2 * s], 3 * w, 3)
        for k in {1: (1, 2, 3), 2: (2,), 4: (4,)}[s]:
            assert got[f"interleaved, base + {k} bytes"][0][0] == pl.MARGIN + k
        for sign, prefix in ((1, "padded"), (-1, "negative")):
            o, rs, ps = got[f"{prefix} pitch, dword rows"]
            assert rs * sign > 3 * w and rs * s % 4 == 0 and ps == 3 and o[1] - o[0] == s == o[2] - o[1]
            o, rs, ps = got[f"{prefix} pitch, odd rows"]
            assert rs * sign > 3 * w and (rs * s % 4 != 0 if s < 4 else rs % 2 == 1) and ps == 3
        o, rs, ps = got["bgr"]
        assert o[0] % 4 == 0 and o[0] - o[1] == s == o[1] - o[2] and (rs, ps) == (3 * w, 3)
        assert got["rgba"][1:] == (4 * w, 4)
        o, rs, ps = got["crop"]
        assert rs > 3 * w and ps == 3 and ((o[0] - pl.MARGIN) // s // 3) % (rs // 3) % 2 == 1  # an odd x of the surface
        for name in ("planes", "planes, odd pitch", "planes in B, G, R order", "planes, negative pitch"):
            o, rs, ps = got[name]
            assert ps == 1 and abs(rs) >= w and min(abs(o[1] - o[0]), abs(o[2] - o[1])) >= h * abs(rs) * s
            assert o[1] - o[0] != o[2] - o[1]  # no plane's place follows from the other two
        assert got["planes"][1] == w
        assert got["planes, odd pitch"][1] * s % 4 != 0 if s < 4 else got["planes, odd pitch"][1] % 2 == 1
        o = got["planes in B, G, R order"][0]
        assert o[0] > o[1] > o[2]
        assert got["planes, negative pitch"][1] < 0


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_the_oracle_reads_every_layout_as_the_contiguous_picture(case):
    """orc.encode_lf_group_ptrs on the host buffer against orc.encode_lf_group on the contiguous picture: the oracle's own
    addressing and the builder.  The filler is 0xFF: a float read outside the picture is a NaN, which the oracle refuses.
    A half picture goes as its float32 widening: the whole buffer is widened, pattern by pattern, and the offsets doubled."""
    from oracle import binding as orc

    type_name, name, w, h = case
    pic = host_picture(type_name, w, h, 1234)
    key = ("stream", type_name, w, h)
    if key not in _cache:
        _cache[key] = orc.encode_lf_group(np.ascontiguousarray(oracle_view(type_name, pic)))[0]
    want = _cache[key]
    buf, offsets, rs, ps = pl.build(name, pic, 0xFF)
    fmt = pl.TYPES[type_name]
    if type_name in ("f16", "bf16"):
        assert buf.size % 2 == 0
        buf = pl.widen_half_bits(buf.view(np.uint16), type_name).view(np.uint8)
        offsets = [2 * o for o in offsets]
        fmt = 2
    got, _ = orc.encode_lf_group_ptrs([buf.ctypes.data + o for o in offsets], rs, ps, fmt, 0, w, h, 0, 1)
    assert np.array_equal(got.xyb.view(np.uint32), want.xyb.view(np.uint32))
    assert len(want.stream) > 0 and got.stream == want.stream


def _reached(type_name):
    """{loader: [(layout, width)]} over the table and the shapes, for a buffer on a multiple of 256"""
    fmt = pl.TYPES[type_name]
    out = {}
    for name in pl.layout_names(pl.SAMPLE_BYTES[fmt]):
        for w, h in pl.SHAPES:
            _, offsets, rs, ps = pl.build(name, host_picture(type_name, w, h, 1234), 0)
            out.setdefault(pl.loader(fmt, [0x7F0000000000 + 256 + o for o in offsets], rs, ps), []).append((name, w))
    return out


REACHABLE = {"u8": {"packed", "per sample"}, "u16": {"packed", "per sample"}, "f32": {"per sample"},
             "f16": {"half run", "half planes", "per sample"}, "bf16": {"half run", "half planes", "per sample"}}


@pytest.mark.parametrize("type_name", TYPE_NAMES)
def test_the_matrix_reaches_every_loader(type_name):
    reached = _reached(type_name)
    assert set(reached) == REACHABLE[type_name] <= set(pl.LOADERS)
    for which, hits in reached.items():
        assert len({name for name, _ in hits}) >= 2, (which, hits)
        assert any(w % 8 == 0 for _, w in hits) and any(w % 8 != 0 for _, w in hits), (which, hits)
    by_layout = {}
    for which, hits in reached.items():
        for name, w in hits:
            by_layout.setdefault(name, set()).add(which)
    if type_name == "f32":
        assert all(v == {"per sample"} for v in by_layout.values())
    if type_name in ("u8", "u16"):  # refused by the pointer test alone, and by the base's bits alone
        for name, v in by_layout.items():
            if name == "bgr" or name.startswith("interleaved, base + "):
                assert v == {"per sample"}, (name, v)
        assert by_layout["padded pitch, dword rows"] == by_layout["negative pitch, dword rows"] == {"packed"}
        # bgr at a width whose rows are dwords: everything but the pointer order says "packed"
        s = pl.SAMPLE_BYTES[pl.TYPES[type_name]]
        _, o, rs, ps = pl.build("bgr", host_picture(type_name, 264, 40, 1234), 0)
        assert ps == 3 and (o[0] | (rs * s)) & 3 == 0 and o[0] > o[2]
        assert pl.loader(pl.TYPES[type_name], [o[0], o[0] + s, o[0] + 2 * s], rs, ps) == "packed"
        assert by_layout["padded pitch, odd rows"] == by_layout["negative pitch, odd rows"] == {"per sample"}
    if type_name in ("f16", "bf16"):
        assert by_layout["padded pitch, dword rows"] == by_layout["negative pitch, dword rows"] == {"half run"}
        assert by_layout["planes in B, G, R order"] == by_layout["planes, negative pitch"] == {"half planes"}
        assert by_layout["planes, odd pitch"] == by_layout["rgba"] == by_layout["bgr"] == {"per sample"}


def test_the_loader_model_on_addresses_the_table_does_not_hold():
    a = 0x7F0000001000
    assert pl.loader(0, [a, a + 1, a + 2], 792, 3) == "packed"
    assert pl.loader(0, [a, a + 1, a + 2], -792, 3) == "packed"  # the pitch's low bits, whatever its sign
    assert pl.loader(0, [a, a + 1, a + 2], -791, 3) == "per sample"
    assert pl.loader(0, [a + 2, a + 1, a], 792, 3) == "per sample"
    assert pl.loader(0, [a, a + 1, a + 2], 792, 4) == "per sample"
    assert pl.loader(1, [a, a + 2, a + 4], 790, 3) == "packed"
    assert pl.loader(1, [a, a + 2, a + 4], 789, 3) == "per sample"
    assert pl.loader(1, [a + 2, a + 4, a + 6], 790, 3) == "per sample"
    assert pl.loader(2, [a, a + 4, a + 8], 792, 3) == "per sample"
    for fmt in (3, 4):
        assert pl.loader(fmt, [a, a + 2, a + 4], 790, 3) == "half run"
        assert pl.loader(fmt, [a, a + 2, a + 4], 789, 3) == "per sample"
        assert pl.loader(fmt, [a, a + 4096, a + 8192], 264, 1) == "half planes"
        assert pl.loader(fmt, [a + 8192, a + 4096, a], -264, 1) == "half planes"
        assert pl.loader(fmt, [a, a + 4098, a + 8192], 264, 1) == "per sample"
        assert pl.loader(fmt, [a, a + 4096, a + 8192], 263, 1) == "per sample"


def test_the_knee_picture_straddles_the_knee_in_every_block_row():
    for w, h in pl.SHAPES:
        pic = pl.knee_picture(w, h)
        assert pic.dtype == np.uint16 and pic.shape == (h, w, 3) and pl.both_sides_of_the_knee(pic)
        # in a whole block and in the ragged last one, from the array itself
        for x0 in ([0, w // 8 * 8] if w % 8 else [0]):
            row = pic[0, x0:x0 + 8].ravel()
            assert (row <= 2650).any() and (row > 2650).any()
    assert not pl.both_sides_of_the_knee(np.zeros((8, 16, 3), np.uint16))
