"""GPU: batches of device-resident one-frame images, each of its own size, to finished files built on the GPU —
hydamd_mixed_* (csrc/host/mixed.c, k_batch_prepare_mixed in csrc/hip/assemble_batch.hip) through device.MixedBatch.
The pictures of a batch are distinct (different seeds); every file is compared whole with what the compiled reference
writes for that picture alone with both tile_size_shift -1."""
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


def _reference_of(key, host, linear_light=0):
    """the reference's file for the picture `host` alone; made once per key and never changed"""
    from oracle import refprobe

    assert reference_expected()
    key = ("ref", key, linear_light)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), np.ascontiguousarray(host), shift_x=-1, shift_y=-1,
                                       linear_light=linear_light)
    return _cache[key]


def _reference(kind, w, h, depth, seed=1234, linear_light=0):
    return _reference_of((kind, w, h, depth, seed), _image(kind, w, h, depth, seed)[1], linear_light)


def _pictures(kind, depth, sizes, first_seed=1234, linear_light=0):
    """device tensors and reference files of one picture per size, every one with a seed of its own"""
    seeds = [first_seed + 17 * k for k in range(len(sizes))]
    imgs = [_image(kind, w, h, depth, s)[0] for (w, h), s in zip(sizes, seeds)]
    wants = [_reference(kind, w, h, depth, s, linear_light) for (w, h), s in zip(sizes, seeds)]
    return imgs, wants


def _md5(b):
    return hashlib.md5(bytes(b)).hexdigest()


def _device_bytes(ptr, nbytes):
    """uint8 CUDA tensor aliasing `nbytes` of device memory at `ptr`"""
    import torch

    class _View:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    return torch.as_tensor(_View(), device="cuda")


def _check(mb, wants):
    """total, host offsets, the files one copy and one by one — all against the concatenated references"""
    total = mb.result()
    files = mb.read()
    assert len(files) == len(wants)
    for k, (got, want) in enumerate(zip(files, wants)):
        got = bytes(got)
        assert len(got) == len(want) and got == want, (k, _md5(got), _md5(want), len(got), len(want))
    off = mb.offsets()
    assert off.dtype == np.uint64 and off.shape == (len(wants) + 1,)
    assert [int(o) for o in off] == [sum(map(len, wants[:k])) for k in range(len(wants) + 1)]
    assert total == int(off[-1]) == sum(map(len, wants))
    return total, off


def _check_on_device(mb, wants):
    import torch

    total, off = _check(mb, wants)
    assert mb.device_ptr() != 0 and mb.offsets_device_ptr() != 0
    on_device = _device_bytes(mb.offsets_device_ptr(), (len(wants) + 1) * 8).cpu().numpy().view(np.uint64)
    assert (on_device == off).all()
    assert bytes(_device_bytes(mb.device_ptr(), total).cpu().numpy()) == b"".join(wants)
    for k in (0, len(wants) - 1):
        assert bytes(mb.read(k)) == wants[k]
    torch.cuda.synchronize()


CASES = [
    # one-group layouts (a single bit-contiguous section), several-group ones, the widest LF group; seven shapes > 4
    ("photo", 8, 0, [(8, 8), (200, 120), (256, 256), (257, 256), (700, 500), (2048, 16), (33, 9)]),
    ("photo", 16, 0, [(232, 188), (520, 264), (264, 520)]),
    ("photo", 32, 0, [(200, 120), (700, 500)]),
    ("photo", 16, 1, [(232, 188), (520, 264)]),  # linear light: another file header in every prefix, other curves
]


@pytest.mark.parametrize("kind,depth,linear,sizes", CASES, ids=[f"{c[0]}-{c[1]}b-lin{c[2]}-{len(c[3])}imgs" for c in CASES])
def test_every_file_of_a_mixed_batch_equals_the_reference(kind, depth, linear, sizes):
    from hydrium_amd import device

    imgs, wants = _pictures(kind, depth, sizes, linear_light=linear)
    assert len(set(wants)) == len(sizes)
    with device.MixedBatch(len(sizes), linear_light=linear) as mb:
        mb.encode(imgs)
        _check_on_device(mb, wants)


def test_one_object_over_changing_size_lists_and_other_objects_in_between():
    """max_frames = 4: three images, then one, then four of other sizes, then the first list of sizes again with other
    pictures (the plan already on the device is reused) — stale plans, scratch or offsets would show; a second MixedBatch
    and a FrameBatch working in between."""
    from hydrium_amd import device

    first = [(200, 120), (520, 264), (33, 9)]
    a_imgs, a_wants = _pictures("photo", 8, first)
    b_imgs, b_wants = _pictures("photo", 8, [(257, 256)], 2001)
    c_imgs, c_wants = _pictures("photo", 8, [(264, 520), (8, 8), (700, 500), (256, 256)], 3001)
    d_imgs, d_wants = _pictures("photo", 8, first, 4001)
    assert a_wants != d_wants
    o_imgs, o_wants = _pictures("photo", 8, [(232, 188), (520, 264)], 5001)
    f_seeds = [1234, 1251, 1268]
    f_imgs = [_image("photo", 700, 500, 8, s)[0] for s in f_seeds]
    f_wants = [_reference("photo", 700, 500, 8, s) for s in f_seeds]
    with device.MixedBatch(4) as mb, device.MixedBatch(4) as other, device.FrameBatch(700, 500, 3) as fb:
        mb.encode(a_imgs)
        other.encode(o_imgs)
        fb.encode(f_imgs)
        _check(mb, a_wants)
        mb.encode(b_imgs)
        _check(other, o_wants)
        other.encode(o_imgs[::-1])
        _check(mb, b_wants)
        mb.encode(c_imgs)
        assert [bytes(f) for f in fb.read()] == f_wants
        _check(other, o_wants[::-1])
        _check_on_device(mb, c_wants)
        mb.encode(a_imgs)
        _check(mb, a_wants)
        mb.encode(d_imgs)  # the same list of sizes as the batch before: no new plan
        _check_on_device(mb, d_wants)
        assert mb.overflow_reruns() == 0


def test_repeated_shapes_and_their_order():
    from hydrium_amd import device

    sizes = [(200, 120), (520, 264), (200, 120), (520, 264)]  # A, B, A', B'
    imgs, wants = _pictures("photo", 8, sizes)
    assert len(set(wants)) == 4
    with device.MixedBatch(4) as mb:
        mb.encode(imgs)
        _check(mb, wants)
        mb.encode(imgs[::-1])
        _check_on_device(mb, wants[::-1])


def test_every_image_its_own_layout():
    """one interleaved tensor, one set of three planes, one padded interleaved tensor (pixel stride 4) and one crop of a
    larger tensor (row pitch > 3 x width, the pointer inside it) — in one batch"""
    import torch
    from hydrium_amd import device

    hwc, want_hwc = _image("photo", 200, 120, 8, 1234)[0], _reference("photo", 200, 120, 8, 1234)
    t = _image("photo", 257, 256, 8, 1251)[0]
    planes, want_planes = [t[:, :, c].contiguous() for c in range(3)], _reference("photo", 257, 256, 8, 1251)
    t = _image("photo", 33, 9, 8, 1268)[0]
    padded, want_padded = torch.zeros((9, 33, 4), dtype=t.dtype, device="cuda"), _reference("photo", 33, 9, 8, 1268)
    padded[:, :, :3] = t
    big, big_host = _image("photo", 700, 500, 8, 1285)
    crop = big[40:304, 100:620, :]  # 520 x 264 out of 700 x 500
    assert crop.stride(0) == 2100 and not crop.is_contiguous()
    want_crop = _reference_of("crop-520x264-of-700x500-1285", big_host[40:304, 100:620, :])
    torch.cuda.synchronize()
    wants = [want_hwc, want_planes, want_padded, want_crop]
    with device.MixedBatch(4) as mb:
        mb.encode([hwc, planes, padded, crop])
        _check(mb, wants)
        # ... and the same four as bare addresses with their strides and sizes
        mb.encode([([hwc.data_ptr() + c for c in range(3)], 600, 3, 200, 120),
                   ([p.data_ptr() for p in planes], 257, 1, 257, 256),
                   ([padded.data_ptr() + c for c in range(3)], 132, 4, 33, 9),
                   ([crop.data_ptr() + c for c in range(3)], 2100, 3, 520, 264)], sample_fmt=0)
        _check(mb, wants)


def test_a_mixed_batch_that_reruns_is_exported_and_assembled_again(monkeypatch):
    from hydrium_amd import device

    monkeypatch.setenv("HYDAMD_TOKEN_CAP", "40000")
    sizes = [(2048, 264), (700, 264)]
    imgs, wants = _pictures("noise", 32, sizes)
    with device.MixedBatch(2) as mb:
        mb.encode(imgs)
        mb.result()
        print("overflow reruns:", mb.overflow_reruns())
        assert mb.overflow_reruns() >= 1, "the case did not exercise the rerun"
        _check_on_device(mb, wants)


def test_nan_in_one_image_fails_the_batch_and_leaves_the_object_usable():
    import torch
    from hydrium_amd import device

    imgs, wants = _pictures("photo", 32, [(200, 120), (520, 264), (257, 256)])
    bad = imgs[1].clone()
    bad[130, 300, 1] = float("nan")
    torch.cuda.synchronize()
    with device.MixedBatch(3) as mb:
        mb.encode([imgs[0], bad, imgs[2]])
        with pytest.raises(device.DeviceError, match="NaN") as e:
            mb.result()
        assert e.value.code == -14
        with pytest.raises(device.DeviceError, match="no batch in flight"):
            mb.result()
        mb.encode(imgs)  # the same sizes: the plan of the failed batch serves
        _check(mb, wants)


def test_argument_and_protocol_errors():
    from hydrium_amd import device

    C = device.C
    t, _ = _image("photo", 200, 120, 32)
    want = _reference("photo", 200, 120, 32)
    with pytest.raises(device.DeviceError, match="max_frames") as e:
        device.MixedBatch(256)
    assert e.value.code == -14
    with device.MixedBatch(2) as mb:
        u8 = C.POINTER(C.c_uint8)
        small = np.empty(8, np.uint8)

        def api_error(match, call):
            with pytest.raises(device.DeviceError, match=match) as e:
                call()
            assert e.value.code == -14

        api_error("no batch in flight", mb.result)
        api_error("no finished batch", lambda: mb._ck(mb.d.hydamd_mixed_read(mb.h, 0, small.ctypes.data_as(u8), 8)))
        api_error("no finished batch", lambda: mb._ck(mb.d.hydamd_mixed_offsets(mb.h, None)))
        assert mb.device_ptr() == 0 and mb.offsets_device_ptr() == 0
        p = t.data_ptr()
        ok = [p, p + 4, p + 8]
        api_error("null image descriptors", lambda: mb._ck(mb.d.hydamd_encode_mixed(mb.h, 1, None, 2)))
        api_error("null pixel pointer", lambda: mb.encode([([p, None, p + 8], 600, 3, 200, 120)], sample_fmt=2))
        api_error("null pixel pointer", lambda: mb.encode([t, ([p, p + 4, None], 600, 3, 200, 120)], sample_fmt=2))
        for w, h in [(2049, 120), (200, 0), (0, 120), (200, 2049)]:
            api_error("must be between 1 and 2048 pixels in each direction", lambda: mb.encode([(ok, 600, 3, w, h)], sample_fmt=2))
        api_error("Invalid Sample Format", lambda: mb.encode([(ok, 600, 3, 200, 120)], sample_fmt=7))
        api_error("frames must be between 1 and max_frames", lambda: mb.encode([t, t, t]))
        api_error("frames must be between 1 and max_frames", lambda: mb.encode([]))
        api_error("no batch in flight", mb.result)  # nothing of the refused calls was enqueued
        mb.encode([t])
        api_error("in flight", lambda: mb.encode([t]))
        total = mb.result()
        api_error("too small", lambda: mb._ck(mb.d.hydamd_mixed_read(mb.h, 0, small.ctypes.data_as(u8), 8)))
        api_error("too small", lambda: mb._ck(mb.d.hydamd_mixed_read(mb.h, -1, small.ctypes.data_as(u8), 8)))
        api_error("null output pointer", lambda: mb._ck(mb.d.hydamd_mixed_read(mb.h, 0, None, 1 << 20)))
        api_error("null output pointer", lambda: mb._ck(mb.d.hydamd_mixed_offsets(mb.h, None)))
        api_error("no such frame", lambda: mb._ck(mb.d.hydamd_mixed_read(mb.h, 1, small.ctypes.data_as(u8), 8)))
        assert total == len(want) and bytes(mb.read(0)) == want
