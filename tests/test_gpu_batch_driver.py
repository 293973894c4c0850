"""GPU: the one host driver under both device-batch objects (csrc/host/batchrun.c) — the same protocol walk over
device.FrameBatch and device.MixedBatch with the same expectations, on two small pictures: what each call answers before a
batch, while one is in flight and once it has settled, every file compared whole with what the compiled reference writes
for that picture alone, and the two objects' files with each other."""
import contextlib
import faulthandler
import re

import numpy as np
import pytest

from conftest import has_gpu, reference_expected
from hydrium_amd import api

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

W, H, SEEDS = 64, 48, (1234, 1251)
_cache = {}
_files = {}  # kind -> the files that object wrote


@contextlib.contextmanager
def _deadline(seconds=120):
    """Around a step that waits for the device.  Such a wait cannot be called off: if it does not come back the run ends
    here, with every thread's traceback, and nothing more is started on a device that hangs."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _pictures():
    """(device tensors, the reference's file for each picture alone); made once and never changed"""
    from hydrium_amd import synth
    from oracle import refprobe
    import torch

    if not _cache:
        assert reference_expected()
        with _deadline():
            imgs = [synth.make_image("photo", W, H, 8, s, device="cuda") for s in SEEDS]
            torch.cuda.synchronize()
            hosts = [np.ascontiguousarray(t.cpu().numpy()) for t in imgs]
        lib = refprobe.reference_library(optimised=True)
        _cache["imgs"] = imgs
        _cache["wants"] = [api.encode_image(lib, h, shift_x=-1, shift_y=-1, linear_light=0) for h in hosts]
    return _cache["imgs"], _cache["wants"]


def _device_u64(ptr, n):
    import torch

    class _View:
        __cuda_array_interface__ = {"shape": (n * 8,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    return torch.as_tensor(_View(), device="cuda").cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("kind", ["batch", "mixed"])
def test_protocol_walk(kind):
    from hydrium_amd import device

    C = device.C
    imgs, wants = _pictures()
    assert len(set(wants)) == 2
    frames = len(imgs)
    with (device.FrameBatch(W, H, frames) if kind == "batch" else device.MixedBatch(frames)) as b:
        u8 = C.POINTER(C.c_uint8)
        first = f"hydamd_{kind}_result first"

        def raw(name, *args):
            return b._ck(getattr(b.d, f"hydamd_{kind}_{name}")(b.h, *args))

        def api_error(text, call):
            with pytest.raises(device.DeviceError, match=re.escape(text)) as e:
                call()
            assert e.value.code == -14

        # before any encode
        room = np.empty(1 << 16, np.uint8)
        api_error("no batch in flight", b.result)
        api_error("no finished batch: " + first, lambda: raw("offsets", np.zeros(frames + 1, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))))
        api_error("no finished batch: " + first, lambda: raw("read", 0, room.ctypes.data_as(u8), room.nbytes))
        api_error("no finished batch: " + first, lambda: raw("image_status", np.zeros(frames, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))))
        # a batch in flight
        with _deadline():
            b.encode(imgs)
        api_error("a batch is in flight: " + first, lambda: b.encode(imgs))
        api_error("a batch is in flight: " + first, lambda: b.set_image_errors(True))
        # settled
        with _deadline():
            total = b.result()
        assert b.result() == total
        with _deadline():
            files = [bytes(f) for f in b.read()]
            assert files == [bytes(b.read(k)) for k in range(frames)]
            off = b.offsets()
        assert int(off[-1]) == total == sum(map(len, files))
        api_error("no such frame", lambda: raw("read", frames, room.ctypes.data_as(u8), room.nbytes))
        api_error("output buffer too small", lambda: raw("read", 0, room.ctypes.data_as(u8), len(files[0]) - 1))
        with _deadline():
            assert (_device_u64(b.offsets_device_ptr(), frames + 1) == off).all()
        for k, (got, want) in enumerate(zip(files, wants)):
            assert got == want, (kind, k, len(got), len(want))
    _files[kind] = files
    assert all(other == files for other in _files.values())
