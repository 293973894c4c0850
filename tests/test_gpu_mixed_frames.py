"""GPU: mixed-size batches whose images hold SEVERAL LF groups (up to 28) beside images of one — hydamd_mixed_create_slots
(csrc/host/mixed.c, k_batch_prepare_frames in csrc/hip/assemble_batch.hip) through device.MixedBatch(max_lf_groups=...),
and the launch group under it, hydamd_begin_batch_frames, by itself.  Strips 8 or 16 pixels high keep many LF groups
cheap.  Every picture of a batch has a seed of its own; every file is compared whole with what the compiled reference
writes for that picture alone with both tile_size_shift -1."""
import numpy as np
import pytest

import mixed_frames_content as mc
from conftest import has_gpu
from test_gpu_mixed_batch import _check, _check_on_device, _image, _pictures, _reference, _reference_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# LF groups 2, 1, 3, 1, 4, 1, 2 (preset fields of 1, 0, 2, 0, 2, 0, 1 bits); the 2 x 2 image's LF groups hold 64, 8, 8 and 1
# groups; one-group frames between the others; files that start off word boundaries
SEVEN = [(2049, 8), (200, 120), (8, 4097), (256, 256), (2049, 2049), (520, 264), (2049, 8)]


def _lf_groups(sizes):
    return [-(-w // 2048) * -(-h // 2048) for w, h in sizes]


def test_layouts_side_by_side():
    from hydrium_amd import device

    imgs, wants = _pictures("photo", 8, SEVEN)
    assert len(set(wants)) == len(SEVEN) and _lf_groups(SEVEN) == [2, 1, 3, 1, 4, 1, 2]
    with device.MixedBatch(7, max_lf_groups=14) as mb:
        mb.encode(imgs)
        _check_on_device(mb, wants)
        assert mb.overflow_reruns() == 0


@pytest.mark.parametrize("sizes,slots", [([(2048 * 4 + 1, 8), (8, 2048 * 8 + 1), (2048 * 16 + 1, 8)], 31),
                                         ([(33, 9), (2048 * 27 + 1, 8)], 29)], ids=["5-9-17", "1-28"])
def test_larger_preset_fields(sizes, slots):
    """5, 9 and 17 LF groups: preset fields of 3, 4 and 5 bits; 28, the cap, behind an image of one"""
    from hydrium_amd import device

    assert sum(_lf_groups(sizes)) == slots
    imgs, wants = _pictures("photo", 16, sizes)
    with device.MixedBatch(len(sizes), max_lf_groups=slots) as mb:
        mb.encode(imgs)
        _check_on_device(mb, wants)


def test_the_running_maximum_restarts_with_every_image_and_carries_inside_one():
    import torch
    from hydrium_amd import device

    hosts = mc.restart_pictures()  # N: noise, one LF group; S: smooth | smooth | smooth; Q: smooth | noise | smooth
    alone = [[max(5, mc.log_alphabet(m)) for _, m in mc.oracle_lf_groups(h, alone=True)] for h in hosts]
    noise, smooth = [alone[0][0], alone[2][1]], alone[1] + [alone[2][0], alone[2][2]]
    assert min(noise) > max(smooth), (alone, "the noise parts must size larger tables than the smooth ones, or the case proves nothing")
    carried = [[r.log_alphabet_size for r, _ in mc.oracle_lf_groups(h)] for h in hosts]
    assert carried[1] == [max(smooth)] * 3 and carried[2] == [alone[2][0], noise[1], noise[1]]  # a restart in S, a carry in Q
    wants = [_reference_of(("restart", k), h) for k, h in enumerate(hosts)]
    imgs = [torch.from_numpy(h).cuda() for h in hosts]
    torch.cuda.synchronize()
    with device.MixedBatch(3, max_lf_groups=7) as mb:
        mb.encode(imgs)
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1])
        _check_on_device(mb, wants[::-1])


def test_a_batch_that_reruns_is_exported_and_assembled_again(monkeypatch):
    from hydrium_amd import device

    monkeypatch.setenv("HYDAMD_TOKEN_CAP", "40000")
    imgs, wants = _pictures("noise", 32, [(2100, 264), (700, 264)])
    with device.MixedBatch(2, max_lf_groups=3) as mb:
        mb.encode(imgs)
        mb.result()
        print("overflow reruns:", mb.overflow_reruns())
        assert mb.overflow_reruns() >= 1, "the case did not exercise the rerun"
        _check_on_device(mb, wants)


def test_nan_in_a_second_lf_group_fails_the_batch_and_leaves_the_object_usable():
    import torch
    from hydrium_amd import device

    imgs, wants = _pictures("photo", 32, [(200, 120), (2049, 64), (257, 256)])
    bad = imgs[1].clone()
    bad[30, 2048, 1] = float("nan")  # the one column of the image's second LF group
    torch.cuda.synchronize()
    with device.MixedBatch(3, max_lf_groups=4) as mb:
        mb.encode([imgs[0], bad, imgs[2]])
        with pytest.raises(device.DeviceError, match="NaN") as e:
            mb.result()
        assert e.value.code == -14
        with pytest.raises(device.DeviceError, match="no batch in flight"):
            mb.result()
        mb.encode(imgs)  # the same sizes: the plan of the failed batch serves
        _check(mb, wants)


def test_input_layouts_across_lf_group_borders():
    """an interleaved tensor, three planes, a pixel-stride-4 tensor and a crop of a larger tensor (row pitch > 3 x width,
    the pointer inside it), every one of several LF groups: the LF groups' pointers come from the image's own strides"""
    import torch
    from hydrium_amd import device

    hwc, want_hwc = _image("photo", 2049, 8, 8, 1234)[0], _reference("photo", 2049, 8, 8, 1234)
    t = _image("photo", 8, 4097, 8, 1268)[0]
    planes, want_planes = [t[:, :, c].contiguous() for c in range(3)], _reference("photo", 8, 4097, 8, 1268)
    t = _image("photo", 2049, 8, 8, 1336)[0]
    padded, want_padded = torch.zeros((8, 2049, 4), dtype=t.dtype, device="cuda"), _reference("photo", 2049, 8, 8, 1336)
    padded[:, :, :3] = t
    big, big_host = _image("photo", 2300, 64, 8, 1285)
    crop = big[12:52, 200:2249, :]  # 2049 x 40 out of 2300 x 64
    assert crop.stride(0) == 6900 and not crop.is_contiguous() and tuple(crop.shape[:2]) == (40, 2049)
    want_crop = _reference_of("crop-2049x40-of-2300x64-1285", big_host[12:52, 200:2249, :])
    torch.cuda.synchronize()
    wants = [want_hwc, want_planes, want_padded, want_crop]
    with device.MixedBatch(4, max_lf_groups=9) as mb:
        mb.encode([hwc, planes, padded, crop])
        _check(mb, wants)
        mb.encode([([hwc.data_ptr() + c for c in range(3)], 3 * 2049, 3, 2049, 8),
                   ([p.data_ptr() for p in planes], 8, 1, 8, 4097),
                   ([padded.data_ptr() + c for c in range(3)], 4 * 2049, 4, 2049, 8),
                   ([crop.data_ptr() + c for c in range(3)], 6900, 3, 2049, 40)], sample_fmt=0)
        _check_on_device(mb, wants)


def test_one_object_over_changing_lists_and_other_objects_in_between():
    """max_frames 4, eight slots: lists of other lengths, sizes and LF-group counts one after another, then the first list
    again with other pictures (the plan on the device is reused) — stale plans, scratch, counters or offsets would show; an
    object of the other constructor and a FrameBatch working in between"""
    from hydrium_amd import device

    first = [(2049, 8), (200, 120)]
    a_imgs, a_wants = _pictures("photo", 8, first)
    b_imgs, b_wants = _pictures("photo", 8, [(8, 4097)], 1268)
    c_imgs, c_wants = _pictures("photo", 8, [(2049, 2049), (256, 256), (33, 9), (2049, 8)], 1302)
    d_imgs, d_wants = _pictures("photo", 8, first, 4001)
    assert a_wants != d_wants
    o_imgs, o_wants = _pictures("photo", 8, [(232, 188), (520, 264)], 5001)
    f_seeds = [1234, 1251, 1268]
    f_imgs = [_image("photo", 700, 500, 8, s)[0] for s in f_seeds]
    f_wants = [_reference("photo", 700, 500, 8, s) for s in f_seeds]
    with device.MixedBatch(4, max_lf_groups=8) as mb, device.MixedBatch(4) as other, device.FrameBatch(700, 500, 3) as fb:
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
        mb.encode(d_imgs)  # the first list of sizes again
        _check(mb, d_wants)
        mb.encode(a_imgs)  # the same list as the batch before: no new plan
        _check_on_device(mb, a_wants)
        assert mb.overflow_reruns() == 0


def test_argument_errors_enqueue_nothing():
    from hydrium_amd import device

    t, _ = _image("photo", 200, 120, 8)
    p = t.data_ptr()
    ok = [p, p + 1, p + 2]

    def api_error(mb, match, call):
        with pytest.raises(device.DeviceError, match=match) as e:
            call()
        assert e.value.code == -14
        with pytest.raises(device.DeviceError, match="no batch in flight"):
            mb.result()

    with device.MixedBatch(3, max_lf_groups=4) as mb:
        api_error(mb, "28 LF groups", lambda: mb.encode([(ok, 600, 3, 2048 * 28 + 1, 8)], sample_fmt=0))
        api_error(mb, "28 LF groups", lambda: mb.encode([(ok, 600, 3, 2048 * 5 + 1, 2048 * 5 + 1)], sample_fmt=0))
        api_error(mb, "more LF groups than the object has slots", lambda: mb.encode([t, (ok, 600, 3, 2049, 4097)], sample_fmt=0))
        api_error(mb, "more LF groups than the object has slots", lambda: mb.encode([(ok, 600, 3, 2048 * 4 + 1, 8)], sample_fmt=0))
        for w, h in [(0, 120), (200, 0)]:
            api_error(mb, "at least 1 pixel", lambda: mb.encode([t, (ok, 600, 3, w, h)], sample_fmt=0))
        mb.encode([t])  # and the object works
        assert bytes(mb.read(0)) == _reference("photo", 200, 120, 8)
    with device.MixedBatch(2) as old:  # the other constructor's objects refuse what they refused
        api_error(old, "must be between 1 and 2048 pixels in each direction", lambda: old.encode([(ok, 600, 3, 2049, 120)], sample_fmt=0))


def test_the_launch_group_by_itself():
    """hydamd_begin_batch_frames with counts 2, 1, 3: per slot, the table kernel's running maximum and the section bit counts
    (which hold the preset field) are the oracle's for that image alone"""
    import ctypes as C
    from hydrium_amd import device

    sizes = SEVEN[:3]
    counts = _lf_groups(sizes)
    pics = [_image("photo", w, h, 8, 1234 + 17 * k) for k, (w, h) in enumerate(sizes)]
    want = [mc.oracle_lf_groups(host) for _, host in pics]
    assert [len(x) for x in want] == counts == [2, 1, 3]
    with device.DeviceContext(0, 6) as ctx:
        for bad in ([2, 0, 3], [29], [3, 3, 1], []):
            with pytest.raises(device.DeviceError) as e:
                ctx.begin_batch_frames(bad)
            assert e.value.code == -14
        assert ctx.d.hydamd_begin_batch_frames(ctx.h, 1, None) == -14
        ctx.begin_batch_frames(counts)
        slot = 0
        for (t, host), (w, h) in zip(pics, sizes):
            lfx = -(-w // 2048)
            for i in range(lfx * -(-h // 2048)):
                x0, y0 = (i % lfx) * 2048, (i // lfx) * 2048
                p = t.data_ptr() + (y0 * w + x0) * 3
                ctx.encode_lf_group(slot, [p, p + 1, p + 2], 3 * w, 3, 0, min(2048, w - x0), min(2048, h - y0), i)
                slot += 1
        with pytest.raises(device.DeviceError, match="preset out of range"):  # an image's presets are its own
            p = pics[1][0].data_ptr()
            ctx.encode_lf_group(2, [p, p + 1, p + 2], 600, 3, 0, 200, 120, 1)
        ctx.finish_frame(6)
        with pytest.raises(device.DeviceError, match="batch") as e:
            ctx.export_frame_owned(6)
        assert e.value.code == -14
        assert ctx.d.hydamd_replay_frame(ctx.h) == -14
        ctx.sync()
        slot = 0
        for per_image in want:
            for r, mx in per_image:
                freq, alpha, log_alpha, run_max = ctx.read_tables(slot)
                assert (log_alpha, run_max) == (r.log_alphabet_size, mx), slot
                bits, _ = ctx.read_sections(slot)
                assert np.array_equal(bits[:r.num_groups], r.group_bits), slot
                slot += 1
