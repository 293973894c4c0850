"""The binding of the two device-batch objects, without a device: device.FrameBatch and device.MixedBatch take every call
behind encode() from one class, and TiledImage.encode, FrameBatch.encode and mixed_descriptors read an image with one
function — held here to what each of them computed from a tensor, a plane triple and device addresses, error texts included."""
import os
import subprocess

import numpy as np
import pytest
import torch

from hydrium_amd import device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHARED = ("close", "__enter__", "__exit__", "_ck", "result", "offsets", "read", "device_ptr", "offsets_device_ptr",
          "set_image_errors", "status", "status_device_ptr", "overflow_reruns")


def test_both_batch_classes_take_the_shared_methods_from_one_class():
    for name in SHARED:
        assert name not in device.FrameBatch.__dict__ and name not in device.MixedBatch.__dict__, name
        assert getattr(device.FrameBatch, name) is getattr(device.MixedBatch, name), name
    assert (device.FrameBatch._prefix, device.MixedBatch._prefix) == ("batch", "mixed")
    for cls in (device.FrameBatch, device.MixedBatch):  # their own: how a batch is described
        assert "__init__" in cls.__dict__ and "encode" in cls.__dict__ and cls.__doc__


def test_the_driver_alone_on_scripted_results_under_host_sanitizers(tmp_path):
    """csrc/host/batchrun.c and tests/batchrun_main.c, whose stub context and assembler answer OK, RETRY then OK, NaN, SPACE
    and four RETRYs: a stand-alone host program, compiled with the address and undefined-behaviour sanitizers."""
    from hydrium_amd import build as hbuild

    exe = str(tmp_path / "batchrun_main")
    cmd = [hbuild.CC, "-std=c99", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DHYDRIUM_INTERNAL_BUILD", f"-I{os.path.join(ROOT, 'include')}",
           f"-I{os.path.join(hbuild.CSRC, 'host')}", os.path.join(ROOT, "tests", "batchrun_main.c"),
           os.path.join(hbuild.CSRC, "host", "batchrun.c"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert made.returncode == 0 and not made.stderr, made.stderr  # no warning either
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert (ran.returncode, ran.stdout, ran.stderr) == (0, "ok\n", ""), (ran.stdout, ran.stderr)


def test_the_image_reader_on_every_kind_of_image():
    t = torch.arange(4 * 6 * 3, dtype=torch.uint8).reshape(4, 6, 3)
    p = t.data_ptr()
    assert device._read_image(t) == ([p, p + 1, p + 2], 18, 3, 4, 6, 0)
    assert device._read_image(t, 99, 99, 2) == ([p, p + 1, p + 2], 18, 3, 4, 6, 0)  # a tensor says everything itself
    wide = torch.zeros((4, 6, 4), dtype=torch.float32)  # the first three of four channels: pixel stride 4, steps of 4 bytes
    q = wide.data_ptr()
    assert device._read_image(wide) == ([q, q + 4, q + 8], 24, 4, 4, 6, 2)
    crop = torch.zeros((8, 16, 3), dtype=torch.int16)[2:6, 3:9]  # a view keeps its parent's pitch
    c = crop.data_ptr()
    assert device._read_image(crop) == ([c, c + 2, c + 4], 48, 3, 4, 6, 1)
    planes = [torch.zeros((4, 6), dtype=torch.float16) for _ in range(3)]
    assert device._read_image(planes) == ([x.data_ptr() for x in planes], 6, 1, 4, 6, device.FLOAT16)
    # device addresses: three of them and the caller's layout (TiledImage, FrameBatch), or the described form (MixedBatch)
    assert device._read_image([p, p + 1, np.int64(p + 2)], 18, 3, 0) == ([p, p + 1, p + 2], 18, 3, None, None, 0)
    assert device._read_image([p, None, p + 2], 18, 3, 0)[0] == [p, None, p + 2]  # a null pointer is the library's to refuse
    assert device._read_image(([p, p + 1, p + 2], 18, 3, 6, 4), sample_fmt=1) == ([p, p + 1, p + 2], 18, 3, 4, 6, 1)
    assert device._read_image(((p, p + 1, p + 2), 18, 3, 6, 4), 7, 7, 1)[1:3] == (18, 3)  # its own strides


def test_the_callers_hand_on_what_the_reader_says():
    t = torch.zeros((4, 6, 3), dtype=torch.uint8)
    wide = torch.zeros((4, 6, 4), dtype=torch.uint8)
    planes = [torch.zeros((4, 6), dtype=torch.uint8) for _ in range(3)]
    tup = ([t.data_ptr()] * 3, 18, 3, 6, 4)
    descs, fmts = device.mixed_descriptors([t, wide, planes, tup], sample_fmt=0)
    assert fmts == [0, 0, 0, 0]
    for d, img in zip(descs, (t, wide, planes, tup)):
        ptrs, rs, ps, h, w, _ = device._read_image(img, sample_fmt=0)
        assert ([d.src[0], d.src[1], d.src[2]], d.row_stride, d.pixel_stride, d.height, d.width) == (ptrs, rs, ps, h, w)

    class Recorder:  # stands where the library does: what encode() would pass to C
        def __getattr__(self, name):
            return lambda *args: self.__dict__.setdefault("calls", []).append((name, args)) or 0

    for cls, call in ((device.FrameBatch, "hydamd_encode_batch"), (device.TiledImage, "hydamd_encode_image_tiled")):
        for img in (t, wide, planes):
            obj = object.__new__(cls)
            obj.d, obj.h = Recorder(), 1
            obj.encode([img] if cls is device.FrameBatch else img)
            (name, args), = obj.d.calls
            arr, got = args[-4], args[-3:]
            ptrs, rs, ps, _, _, fmt = device._read_image(img)
            assert name == call and [arr[0], arr[1], arr[2]] == ptrs and got == (rs, ps, fmt)
        obj = object.__new__(cls)
        obj.d, obj.h = Recorder(), 1
        addresses = [t.data_ptr(), t.data_ptr() + 1, t.data_ptr() + 2]
        obj.encode([addresses] if cls is device.FrameBatch else addresses, 18, 3, 0)
        assert obj.d.calls[0][1][-3:] == (18, 3, 0)


def test_every_refusal_keeps_its_text():
    t = torch.zeros((4, 6, 3), dtype=torch.uint8)
    wide = torch.zeros((4, 6, 4), dtype=torch.uint8)
    f32 = torch.zeros((4, 6, 3), dtype=torch.float32)
    p = t.data_ptr()
    need_all = "device addresses need row_stride, pixel_stride and sample_fmt"
    for args in ((), (18,), (18, 3), (None, 3, 0)):
        with pytest.raises(ValueError, match=need_all):
            device._read_image([p, p, p], *args)
    with pytest.raises(ValueError, match=need_all):
        device.TiledImage.encode(object.__new__(device.TiledImage), [p, p, p], 18, 3)
    with pytest.raises(ValueError, match=need_all):
        device.FrameBatch.encode(object.__new__(device.FrameBatch), [[p, p, p]], 18)
    with pytest.raises(ValueError, match="device addresses need sample_fmt$"):
        device.mixed_descriptors([([p, p, p], 18, 3, 6, 4)])
    shapes = [torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((4, 5), dtype=torch.uint8)]
    pitches = [torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((4, 8), dtype=torch.uint8)[:, :6]]
    for bad in (shapes, pitches):
        with pytest.raises(ValueError, match="the three planes of an image share one shape and one layout"):
            device.mixed_descriptors([bad])
    with pytest.raises(ValueError, match="no sample format for pixels of type"):
        device._read_image(torch.zeros((4, 6, 3), dtype=torch.float64))
    for pair in ([t, wide], [t, f32]):
        with pytest.raises(ValueError, match="the frames of a batch share one layout and sample format"):
            device.FrameBatch.encode(object.__new__(device.FrameBatch), pair)
    with pytest.raises(ValueError, match="the images of a batch share one sample format"):
        device.mixed_descriptors([t, f32])
    with pytest.raises(ValueError, match="sample_fmts disagrees with a tensor's dtype"):
        device.mixed_descriptors([t, f32], sample_fmts=[0, 1])
    with pytest.raises(ValueError, match="sample_fmts names one format per image"):
        device.mixed_descriptors([t, f32], sample_fmts=[0])
    with pytest.raises(ValueError, match='sample_fmts is None, "each" or one format per image'):
        device.mixed_descriptors([t], sample_fmts="all")
    for cls in (device.FrameBatch, device.MixedBatch):
        obj = object.__new__(cls)
        obj.frames, obj.offsets = 2, lambda: np.array([0, 5, 9], np.uint64)
        for k in (-1, 2):
            with pytest.raises(IndexError, match="no such frame in the batch"):
                obj.read(k)
