"""GPU: tile-mode images from device-resident pixels, frames built on the GPU — hydamd_tiled_* (csrc/host/tiled.c,
csrc/hip/assemble_tiles.hip) through device.TiledImage.  Every tile is a frame of its own (reference
libhydrium.c:147-203); every case compares the whole file with the reference's for the same pixels and shifts."""
import hashlib

import numpy as np
import pytest

from conftest import has_gpu, reference_expected
from hydrium_amd import api

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

_cache = {}


def _image(kind, w, h, depth):
    import torch
    from hydrium_amd import synth

    key = (kind, w, h, depth)
    if key not in _cache:
        if depth == 32:
            host = synth.make_image_f32(kind, w, h)
            _cache[key] = (torch.from_numpy(host).cuda(), host)
        else:
            t = synth.make_image(kind, w, h, depth, device="cuda")
            torch.cuda.synchronize()
            a = t.cpu().numpy()
            _cache[key] = (t, np.ascontiguousarray(a.view(np.uint16) if depth == 16 else a))
    return _cache[key]


def _reference(host, sx, sy, linear_light=0):
    from oracle import refprobe

    assert reference_expected()
    key = ("ref", id(host), sx, sy, linear_light)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), host, shift_x=sx, shift_y=sy,
                                       linear_light=linear_light)
    return _cache[key]


def _md5(b):
    return hashlib.md5(bytes(b)).hexdigest()


CASES = [
    ("photo", 1000, 700, 8, 0, 0, 0, 0),    # 12 frames, all of one group, ragged right and bottom edges
    ("photo", 1000, 700, 8, 0, 0, 5, 0),    # launch groups of 5, 5, 2: the running offset across launch groups
    ("photo", 1000, 700, 8, 1, 1, 0, 0),    # 2 x 2 frames of several groups with TOC; edge frames of 2 and 1 groups... and 4
    ("photo", 2100, 520, 8, 3, 0, 0, 0),    # 8-group frames and 52-pixel single-group frames in one launch group; last row 8 px
    ("photo", 520, 300, 16, 1, 0, 0, 0),    # other sample width, unequal shifts
    ("photo", 520, 300, 16, 1, 0, 0, 1),    # ... linear light
    ("photo", 300, 280, 32, 0, 0, 0, 0),    # float records in a batch
]


@pytest.mark.parametrize("kind,w,h,depth,sx,sy,per_launch,linear", CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}b-shift{c[4]}{c[5]}-launch{c[6]}-lin{c[7]}" for c in CASES])
def test_tiled_file_equals_the_reference(kind, w, h, depth, sx, sy, per_launch, linear):
    from hydrium_amd import device

    t, host = _image(kind, w, h, depth)
    want = _reference(host, sx, sy, linear)
    with device.TiledImage(w, h, sx, sy, linear_light=linear, tiles_per_launch=per_launch) as ti:
        ti.encode(t)
        got = bytes(ti.read())
        assert ti.device_ptr() != 0
    assert len(got) == len(want) and got == want, (_md5(got), _md5(want), len(got), len(want))


def test_planar_and_padded_interleaved_tensors():
    import torch
    from hydrium_amd import device

    t, host = _image("photo", 1000, 700, 8)
    want = _reference(host, 0, 0)
    planes = [t[:, :, c].contiguous() for c in range(3)]
    padded = torch.zeros((700, 1000, 4), dtype=t.dtype, device="cuda")
    padded[:, :, :3] = t
    torch.cuda.synchronize()
    with device.TiledImage(1000, 700, 0, 0) as ti:
        ti.encode(planes)
        a = bytes(ti.read())
        ti.encode(padded)  # pixel_stride = 4
        b = bytes(ti.read())
    assert a == want and b == want


def test_a_launch_group_that_reruns_leaves_later_frames_at_the_right_offsets(monkeypatch):
    from hydrium_amd import device

    monkeypatch.setenv("HYDAMD_TOKEN_CAP", "40000")
    t, host = _image("noise", 600, 520, 32)
    want = _reference(host, 0, 0)
    with device.TiledImage(600, 520, 0, 0, tiles_per_launch=2) as ti:
        ti.encode(t)
        got = bytes(ti.read())
        assert ti.overflow_reruns() >= 1, "the case did not exercise the rerun"
    assert got == want, (_md5(got), _md5(want), len(got), len(want))


def test_a_strip_one_frame_mode_refuses():
    """262144 x 8: 128 LF groups in one-frame mode, which hydamd_encode_image refuses; 128 tiles of 2048 x 8 here — more
    tiles than a launch group holds."""
    from hydrium_amd import device

    w, h = 262144, 8
    t, host = _image("photo", w, h, 8)
    want = _reference(host, 3, 0)
    with device.DeviceContext(0, 128) as ctx:
        with pytest.raises(device.DeviceError, match="unsupported number of LF groups"):
            ctx.encode_image_tensor(t)
    with device.TiledImage(w, h, 3, 0) as ti:
        ti.encode(t)
        got = bytes(ti.read())
    assert got == want, (_md5(got), _md5(want), len(got), len(want))


def test_nan_in_a_middle_tile_fails_the_image_and_leaves_the_object_usable():
    import torch
    from hydrium_amd import device

    t, host = _image("photo", 300, 280, 32)
    want = _reference(host, 0, 0)
    bad = t.clone()
    bad[100, 270, 1] = float("nan")  # tile (1, 0) of 2 x 2
    torch.cuda.synchronize()
    with device.TiledImage(300, 280, 0, 0) as ti:
        ti.encode(bad)
        with pytest.raises(device.DeviceError, match="NaN"):
            ti.result()
        ti.encode(t)
        assert bytes(ti.read()) == want


def test_argument_and_protocol_errors():
    from hydrium_amd import device

    t, _ = _image("photo", 300, 280, 32)
    with pytest.raises(device.DeviceError, match="tile_size_shift"):
        device.TiledImage(300, 280, -1, 0)
    with pytest.raises(device.DeviceError, match="tile_size_shift"):
        device.TiledImage(300, 280, 0, -1)
    with device.TiledImage(300, 280, 0, 0) as ti:
        with pytest.raises(device.DeviceError, match="no image in flight"):
            ti.result()
        with pytest.raises(device.DeviceError, match="no finished image"):
            ti._ck(ti.d.hydamd_tiled_read(ti.h, None, 0))
        p = t.data_ptr()
        with pytest.raises(device.DeviceError, match="null pixel pointer"):
            ti.encode([p, None, p + 8], 900, 3, 2)
        with pytest.raises(device.DeviceError, match="Invalid Sample Format"):
            ti.encode([p, p + 4, p + 8], 900, 3, 7)
        ti.encode(t)
        with pytest.raises(device.DeviceError, match="in flight"):
            ti.encode(t)
        size = ti.result()
        with pytest.raises(device.DeviceError, match="too small"):
            ti._ck(ti.d.hydamd_tiled_read(ti.h, np.empty(8, np.uint8).ctypes.data_as(device.C.POINTER(device.C.c_uint8)), 8))
        assert size == len(ti.read())


def test_one_object_twice_and_two_objects_interleaved():
    from hydrium_amd import device

    a_t, a_host = _image("photo", 1000, 700, 8)
    b_t, b_host = _image("photo", 520, 300, 16)
    want_a, want_b = _reference(a_host, 0, 0), _reference(b_host, 1, 0)
    with device.TiledImage(1000, 700, 0, 0, tiles_per_launch=5) as a, device.TiledImage(520, 300, 1, 0) as b:
        a.encode(a_t)
        b.encode(b_t)
        got_b = bytes(b.read())
        got_a = bytes(a.read())
        a.encode(a_t)
        again = bytes(a.read())
    assert got_a == want_a and again == want_a and got_b == want_b
