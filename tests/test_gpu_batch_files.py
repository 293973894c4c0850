"""GPU: batches of device-resident one-frame images to finished files, built on the GPU — hydamd_batch_*
(csrc/host/batch.c, csrc/hip/assemble_batch.hip) through device.FrameBatch.  The pictures of a batch are distinct
(different seeds); every file is compared whole with what the compiled reference writes for that picture alone."""
import hashlib

import numpy as np
import pytest

from conftest import has_gpu, reference_expected
from hydrium_amd import api

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

_cache = {}


def _image(kind, w, h, depth, seed=1234):
    """(device tensor, host array) of one picture; made once"""
    import torch
    from hydrium_amd import synth

    key = (kind, w, h, depth, seed)
    if key not in _cache:
        if depth == 32:
            host = synth.make_image_f32(kind, w, h, seed)
            _cache[key] = (torch.from_numpy(host).cuda(), host)
        else:
            t = synth.make_image(kind, w, h, depth, seed, device="cuda")
            torch.cuda.synchronize()
            a = t.cpu().numpy()
            _cache[key] = (t, np.ascontiguousarray(a.view(np.uint16) if depth == 16 else a))
    return _cache[key]


def _reference(kind, w, h, depth, seed=1234, linear_light=0, icc=None):
    """the reference's file for that picture alone; made once and never changed"""
    from oracle import refprobe

    assert reference_expected()
    key = ("ref", kind, w, h, depth, seed, linear_light, icc)
    if key not in _cache:
        host = _image(kind, w, h, depth, seed)[1]
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), host, shift_x=-1, shift_y=-1,
                                       linear_light=linear_light, icc=icc)
    return _cache[key]


def _md5(b):
    return hashlib.md5(bytes(b)).hexdigest()


def _check(fb, files, wants):
    assert len(files) == len(wants)
    for k, (got, want) in enumerate(zip(files, wants)):
        got = bytes(got)
        assert len(got) == len(want) and got == want, (k, _md5(got), _md5(want), len(got), len(want))
    off = fb.offsets()
    assert off[0] == 0 and [int(off[k + 1] - off[k]) for k in range(len(wants))] == [len(w) for w in wants]


CASES = [
    ("photo", 2100, 300, 8, 3, 0),     # two LF groups per frame, 16 + 2 groups, two tails; files start off word boundaries
    ("photo", 2348, 2088, 16, 2, 0),   # 2 x 2 LF groups, four LF-group shapes, the TOC permutation over 4 presets
    ("smooth", 2056, 16, 8, 5, 0),     # tiny LF streams (simple prefix codes), odd F, frames of a few hundred bytes
    ("photo", 2100, 300, 32, 2, 0),    # float records; the running alphabet must not leak from frame k to k + 1
    ("photo", 2100, 300, 16, 2, 1),    # ... linear light
    ("photo", 700, 500, 8, 3, 0),      # one LF group, six groups, TOC: the hydk_tiles.h path
    ("photo", 200, 120, 8, 4, 0),      # one group: a single bit-contiguous section
]


@pytest.mark.parametrize("kind,w,h,depth,frames,linear", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}b-F{c[4]}-lin{c[5]}" for c in CASES])
def test_every_file_of_a_batch_equals_the_reference(kind, w, h, depth, frames, linear):
    from hydrium_amd import device

    seeds = [1234 + 17 * k for k in range(frames)]
    imgs = [_image(kind, w, h, depth, s)[0] for s in seeds]
    wants = [_reference(kind, w, h, depth, s, linear) for s in seeds]
    assert len(set(wants)) == frames  # distinct pictures
    with device.FrameBatch(w, h, frames, linear_light=linear) as fb:
        fb.encode(imgs)
        total = fb.result()
        assert total == sum(len(x) for x in wants) and fb.device_ptr() != 0 and fb.offsets_device_ptr() != 0
        _check(fb, fb.read(), wants)


def test_one_object_over_batches_of_different_sizes_and_two_objects_interleaved():
    """max_frames = 4: three frames, then one, then four other pictures — stale done counters, scratch and offsets would
    show; and a second object (another shape, the one-LF-group path) working in between."""
    from hydrium_amd import device

    shape = ("photo", 2100, 300, 8)
    other = ("photo", 700, 500, 8)
    seeds = [1234 + 17 * k for k in range(8)]
    imgs = [_image(*shape, s)[0] for s in seeds]
    wants = [_reference(*shape, s) for s in seeds]
    o_imgs = [_image(*other, s)[0] for s in seeds[:3]]
    o_wants = [_reference(*other, s) for s in seeds[:3]]
    with device.FrameBatch(2100, 300, 4) as a, device.FrameBatch(700, 500, 3) as b:
        a.encode(imgs[:3])
        b.encode(o_imgs)
        _check(a, a.read(), wants[:3])
        a.encode(imgs[3:4])
        _check(b, b.read(), o_wants)
        b.encode(o_imgs[1:])
        _check(a, a.read(), wants[3:4])
        a.encode(imgs[4:])
        _check(b, b.read(), o_wants[1:])
        _check(a, a.read(), wants[4:])


def test_icc_profile_in_every_file():
    from hydrium_amd import device

    icc = bytes(range(256)) * 3 + b"tail"
    seeds = [1234, 1251]
    imgs = [_image("photo", 520, 300, 8, s)[0] for s in seeds]
    wants = [_reference("photo", 520, 300, 8, s, icc=icc) for s in seeds]
    assert wants[0] != _reference("photo", 520, 300, 8, seeds[0])
    with device.FrameBatch(520, 300, 2, icc=icc) as fb:
        fb.encode(imgs)
        _check(fb, fb.read(), wants)


def test_planar_and_padded_interleaved_tensors():
    import torch
    from hydrium_amd import device

    seeds = [1234, 1251]
    ts = [_image("photo", 2100, 300, 8, s)[0] for s in seeds]
    wants = [_reference("photo", 2100, 300, 8, s) for s in seeds]
    planes = [[t[:, :, c].contiguous() for c in range(3)] for t in ts]
    padded = []
    for t in ts:
        p = torch.zeros((300, 2100, 4), dtype=t.dtype, device="cuda")
        p[:, :, :3] = t
        padded.append(p)
    torch.cuda.synchronize()
    with device.FrameBatch(2100, 300, 2) as fb:
        fb.encode(planes)
        _check(fb, fb.read(), wants)
        fb.encode(padded)  # pixel_stride = 4
        _check(fb, fb.read(), wants)


def test_a_batch_that_reruns_is_exported_and_assembled_again(monkeypatch):
    from hydrium_amd import device

    monkeypatch.setenv("HYDAMD_TOKEN_CAP", "40000")
    seeds = [1234, 1251]
    imgs = [_image("noise", 2100, 264, 32, s)[0] for s in seeds]
    wants = [_reference("noise", 2100, 264, 32, s) for s in seeds]
    with device.FrameBatch(2100, 264, 2) as fb:
        fb.encode(imgs)
        files = fb.read()
        print("overflow reruns:", fb.overflow_reruns())
        assert fb.overflow_reruns() >= 1, "the case did not exercise the rerun"
        _check(fb, files, wants)


def test_nan_in_one_frame_fails_the_batch_and_leaves_the_object_usable():
    import torch
    from hydrium_amd import device

    seeds = [1234, 1251, 1268]
    imgs = [_image("photo", 2100, 300, 32, s)[0] for s in seeds]
    wants = [_reference("photo", 2100, 300, 32, s) for s in seeds]
    bad = imgs[1].clone()
    bad[100, 2070, 1] = float("nan")  # frame 1 of 3, its second LF group
    torch.cuda.synchronize()
    with device.FrameBatch(2100, 300, 3) as fb:
        fb.encode([imgs[0], bad, imgs[2]])
        with pytest.raises(device.DeviceError, match="NaN") as e:
            fb.result()
        assert e.value.code == -14
        with pytest.raises(device.DeviceError, match="no batch in flight"):
            fb.result()
        fb.encode(imgs)
        _check(fb, fb.read(), wants)


def test_argument_and_protocol_errors():
    from hydrium_amd import device

    C = device.C
    t, _ = _image("photo", 2100, 300, 32)
    md, st = api.HYDImageMetadata(2100, 300, 0, 0, 0), C.c_int(0)  # (the class itself always passes -1, -1)
    assert not device.dll().hydamd_batch_create(0, C.byref(md), 2, None, 0, C.byref(st))
    assert st.value == -14 and b"tile_size_shift" in device.dll().hydamd_batch_error(None)
    with pytest.raises(device.DeviceError, match="255"):
        device.FrameBatch(2100, 300, 128)
    with device.FrameBatch(2100, 300, 2) as fb:
        u8 = C.POINTER(C.c_uint8)
        small = np.empty(8, np.uint8)

        def api_error(match, call):
            with pytest.raises(device.DeviceError, match=match) as e:
                call()
            assert e.value.code == -14

        api_error("no batch in flight", fb.result)
        api_error("no finished batch", lambda: fb._ck(fb.d.hydamd_batch_read(fb.h, 0, small.ctypes.data_as(u8), 8)))
        api_error("no finished batch", lambda: fb._ck(fb.d.hydamd_batch_offsets(fb.h, None)))
        assert fb.device_ptr() == 0 and fb.offsets_device_ptr() == 0
        p = t.data_ptr()
        api_error("null pixel pointer", lambda: fb.encode([[p, None, p + 8]], 6300, 3, 2))
        api_error("null pixel pointer", lambda: fb._ck(fb.d.hydamd_encode_batch(fb.h, 1, None, 6300, 3, 2)))
        api_error("Invalid Sample Format", lambda: fb.encode([[p, p + 4, p + 8]], 6300, 3, 7))
        api_error("frames must be between 1 and max_frames", lambda: fb.encode([t, t, t]))
        api_error("frames must be between 1 and max_frames", lambda: fb.encode([]))
        fb.encode([t])
        api_error("in flight", lambda: fb.encode([t]))
        total = fb.result()
        api_error("too small", lambda: fb._ck(fb.d.hydamd_batch_read(fb.h, 0, small.ctypes.data_as(u8), 8)))
        api_error("too small", lambda: fb._ck(fb.d.hydamd_batch_read(fb.h, -1, small.ctypes.data_as(u8), 8)))
        api_error("null output pointer", lambda: fb._ck(fb.d.hydamd_batch_read(fb.h, 0, None, 1 << 20)))
        api_error("null output pointer", lambda: fb._ck(fb.d.hydamd_batch_offsets(fb.h, None)))
        api_error("no such frame", lambda: fb._ck(fb.d.hydamd_batch_read(fb.h, 1, small.ctypes.data_as(u8), 8)))
        assert total == len(fb.read(0)) == len(_reference("photo", 2100, 300, 32))


def test_offsets_on_the_host_and_on_the_device_and_single_reads():
    import torch
    from hydrium_amd import device

    seeds = [1234 + 17 * k for k in range(3)]
    imgs = [_image("photo", 2100, 300, 8, s)[0] for s in seeds]
    wants = [_reference("photo", 2100, 300, 8, s) for s in seeds]
    with device.FrameBatch(2100, 300, 4) as fb:  # fewer frames than the object holds
        fb.encode(imgs)
        total = fb.result()
        off = fb.offsets()
        assert off.dtype == np.uint64 and off.shape == (4,) and off[0] == 0 and off[3] == total
        assert all(off[k] < off[k + 1] for k in range(3))
        on_device = _device_bytes(fb.offsets_device_ptr(), 4 * 8).cpu().numpy().view(np.uint64)
        assert (on_device == off).all()
        whole = fb.read()
        for k in range(3):
            one = fb.read(k)
            assert bytes(one) == bytes(whole[k]) == wants[k]
        files = _device_bytes(fb.device_ptr(), total).cpu().numpy()
        assert bytes(files) == b"".join(wants)
        torch.cuda.synchronize()


def _device_bytes(ptr, nbytes):
    """uint8 CUDA tensor aliasing `nbytes` of device memory at `ptr`"""
    import torch

    class _View:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    return torch.as_tensor(_View(), device="cuda")
