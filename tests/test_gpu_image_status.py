"""GPU: an outcome per image for the device batches — FrameBatch / MixedBatch(image_errors=True), hydamd_*_set_image_errors
(csrc/host/batch.c, mixed.c; k_batch_place in csrc/hip/assemble_batch.hip) and the per-slot bad-sample flag underneath
(hydamd_set_bad_sample_per_slot, the float instance of k_transform_tokenize).  An image with a non-finite float sample
yields no bytes and a status word; every other file is compared whole with what the compiled reference writes for that
picture alone, and the device buffer with those files back to back — the files on both sides of a skipped image meet at
byte granularity."""
import numpy as np
import pytest

from conftest import has_gpu
from test_gpu_mixed_batch import _device_bytes, _image, _md5, _pictures, _reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def _with_nan(img, y, x, c=1, value=float("nan")):
    import torch

    bad = img.clone()
    bad[y, x, c] = value
    torch.cuda.synchronize()
    return bad


def _check_outcomes(b, wants, flagged):
    """`b`: a batch object with a batch in flight; wants[k]: the reference's file of image k; flagged: the images that must
    yield no bytes.  Total, files, offsets and statuses on the host and on the device, the device buffer whole."""
    import torch

    n = len(wants)
    kept = [b"" if k in flagged else wants[k] for k in range(n)]
    total = b.result()
    status = b.status()
    assert status.dtype == np.uint32 and [int(s) for s in status] == [1 if k in flagged else 0 for k in range(n)]
    off = b.offsets()
    assert [int(o) for o in off] == [sum(map(len, kept[:k])) for k in range(n + 1)]
    assert total == int(off[-1]) == sum(map(len, kept))
    files = b.read()
    assert len(files) == n
    for k, (got, want) in enumerate(zip(files, kept)):
        got = bytes(got)
        assert len(got) == len(want) and got == want, (k, _md5(got), _md5(want), len(got), len(want))
    for k in range(n):
        one = b.read(k)
        assert one.dtype == np.uint8 and bytes(one) == kept[k], k
    assert b.device_ptr() != 0 and b.offsets_device_ptr() != 0 and b.status_device_ptr() != 0
    assert (_device_bytes(b.offsets_device_ptr(), (n + 1) * 8).cpu().numpy().view(np.uint64) == off).all()
    assert (_device_bytes(b.status_device_ptr(), n * 4).cpu().numpy().view(np.uint32) == status).all()
    if total:
        assert bytes(_device_bytes(b.device_ptr(), total).cpu().numpy()) == b"".join(kept)
    torch.cuda.synchronize()
    return total


# ---- the context: a flag per slot ----
def _three_lf_groups(ctx, imgs):
    ctx.begin_batch(1, len(imgs))
    for k, t in enumerate(imgs):
        ctx.encode_lf_group(k, [t.data_ptr() + 4 * c for c in range(3)], t.stride(0), t.stride(1), 2, t.shape[1], t.shape[0], 0)
    ctx.finish_frame(len(imgs))


def _slot_results(ctx, slot):
    lf = ctx.read_lf_streams(1, first=slot)[0]
    bits, offs = ctx.read_sections(slot)
    payload = ctx.read_payload()
    sections = [payload[int(o):int(o) + ((int(n) + 7) >> 3)] for n, o in zip(bits, offs)]
    lf_bytes = bytes(ctx.read_lf_payload()[int(lf["offset"]):int(lf["offset"]) + ((int(lf["bit_count"]) + 7) >> 3)])
    freq, alpha, log_alpha, run_max = ctx.read_tables(slot)
    return (bits.tolist(), sections, freq.tobytes(), alpha.tolist(), log_alpha, run_max, int(lf["bit_count"]), int(lf["alphabet"]),
            int(lf["run_pairs"]), int(lf["error"]), lf["lengths"].tobytes(), lf_bytes)


def test_a_flag_per_slot_and_untouched_neighbours():
    from hydrium_amd import device

    imgs = [_image("photo", 64, 40, 32, s)[0] for s in (1234, 1251, 1268)]
    bad = _with_nan(imgs[1], 17, 33)
    with device.DeviceContext(0, 3) as ctx:
        ctx.set_lf_coder(2)
        _three_lf_groups(ctx, [imgs[0], imgs[2]])
        ctx.sync()
        assert ctx.read_bad_slots(2).tolist() == [0, 0]
        alone = [_slot_results(ctx, 0), _slot_results(ctx, 1)]
        _three_lf_groups(ctx, [imgs[0], bad, imgs[2]])  # the mode is off: as ever
        with pytest.raises(device.DeviceError, match="NaN") as e:
            ctx.sync()
        assert e.value.code == -14
        ctx.set_bad_sample_per_slot(True)
        _three_lf_groups(ctx, [imgs[0], bad, imgs[2]])
        ctx.sync()
        assert ctx.read_bad_slots(3).tolist() == [0, 1, 0]
        assert ctx.read_bad_slots(1, first=1).tolist() == [1]
        assert _slot_results(ctx, 0) == alone[0] and _slot_results(ctx, 2) == alone[1]
        assert ctx.overflow_reruns() == 0
        _three_lf_groups(ctx, imgs)  # the flags are cleared with the frame's accumulators
        ctx.sync()
        assert ctx.read_bad_slots(3).tolist() == [0, 0, 0]
        ctx.set_bad_sample_per_slot(False)
        _three_lf_groups(ctx, [imgs[0], bad, imgs[2]])
        with pytest.raises(device.DeviceError, match="NaN"):
            ctx.sync()


# ---- MixedBatch, one LF group each ----
ONE = [(8, 8), (256, 256), (300, 200), (33, 9)]  # (256, 256): the single bit-contiguous section


@pytest.mark.parametrize("where", [0, 1, 2, 3], ids=["first", "single-section", "middle", "last-next-to-the-padding"])
def test_a_flagged_image_of_a_mixed_batch_yields_no_bytes(where):
    from hydrium_amd import device

    imgs, wants = _pictures("photo", 32, ONE)
    w, h = ONE[where]
    given = list(imgs)
    given[where] = _with_nan(imgs[where], h - 1, w - 1, 2) if where == 3 else _with_nan(imgs[where], h // 2, w // 3)
    with device.MixedBatch(4, image_errors=True) as mb:
        mb.encode(given)
        _check_outcomes(mb, wants, {where})
        assert mb.overflow_reruns() == 0


# ---- MixedBatch, images of several LF groups ----
def test_a_nan_in_a_second_lf_group_flags_its_image_and_either_frame_kernel_skips():
    from hydrium_amd import device

    imgs, wants = _pictures("photo", 32, [(200, 120), (2049, 64), (257, 256)])
    with device.MixedBatch(3, max_lf_groups=4, image_errors=True) as mb:
        mb.encode([imgs[0], _with_nan(imgs[1], 30, 2048), imgs[2]])  # the one column of the image's second LF group
        _check_outcomes(mb, wants, {1})
        mb.encode([imgs[0], imgs[1], _with_nan(imgs[2], 100, 100)])  # an image of one LF group: the other kernel's
        _check_outcomes(mb, wants, {2})
        mb.encode([_with_nan(imgs[0], 0, 0, 0, float("-inf")), _with_nan(imgs[1], 63, 5), imgs[2]])
        _check_outcomes(mb, wants, {0, 1})
        assert mb.overflow_reruns() == 0


# ---- FrameBatch ----
@pytest.mark.parametrize("w,h", [(256, 256), (300, 200), (2049, 16)], ids=["single-section", "one-lf-group", "two-lf-groups"])
def test_a_flagged_frame_of_a_frame_batch_yields_no_bytes(w, h):
    from hydrium_amd import device

    seeds = [1234, 1251, 1268, 1285]
    imgs = [_image("photo", w, h, 32, s)[0] for s in seeds]
    wants = [_reference("photo", w, h, 32, s) for s in seeds]
    with device.FrameBatch(w, h, 4, image_errors=True) as fb:
        fb.encode([imgs[0], _with_nan(imgs[1], h - 1, w - 1), imgs[2], imgs[3]])  # (2049 wide: the second LF group)
        _check_outcomes(fb, wants, {1})
        fb.encode([imgs[0], imgs[1], imgs[2], _with_nan(imgs[3], 0, 0, 0)])
        _check_outcomes(fb, wants, {3})
        fb.encode(imgs)
        _check_outcomes(fb, wants, set())
        assert fb.overflow_reruns() == 0


# ---- all flagged, none flagged, and Inf ----
def test_all_flagged_none_flagged_and_a_picture_of_infinities():
    import torch
    from hydrium_amd import device

    sizes = [(200, 120), (300, 200), (33, 9)]
    imgs, wants = _pictures("photo", 32, sizes)
    inf = torch.full_like(imgs[1], float("inf"))  # EVERY sample: nothing of it may reach the launch group's tables or status
    torch.cuda.synchronize()
    with device.MixedBatch(3, image_errors=True) as mb:
        mb.encode([_with_nan(t, 1, 1) for t in imgs])
        assert _check_outcomes(mb, wants, {0, 1, 2}) == 0
        mb.encode(imgs)
        _check_outcomes(mb, wants, set())
        mb.encode([imgs[0], inf, imgs[2]])
        _check_outcomes(mb, wants, {1})
        assert mb.overflow_reruns() == 0
    with device.MixedBatch(3) as mb:  # without the switch: all zeros after a good batch
        mb.encode(imgs)
        _check_outcomes(mb, wants, set())
    w, h = sizes[0]
    f_wants = [wants[0], _reference("photo", w, h, 32, 1251)]
    f_imgs = [imgs[0], _image("photo", w, h, 32, 1251)[0]]
    with device.FrameBatch(w, h, 2, image_errors=True) as fb:
        fb.encode([_with_nan(t, 2, 2) for t in f_imgs])
        assert _check_outcomes(fb, f_wants, {0, 1}) == 0
    with device.FrameBatch(w, h, 2) as fb:
        fb.encode(f_imgs)
        _check_outcomes(fb, f_wants, set())


# ---- a batch that reruns arrives at the same outcomes ----
def test_a_batch_that_reruns_arrives_at_the_same_outcomes(monkeypatch):
    from hydrium_amd import device

    monkeypatch.setenv("HYDAMD_TOKEN_CAP", "40000")
    imgs, wants = _pictures("noise", 32, [(2100, 264), (700, 264)])
    small, small_want = _image("photo", 200, 120, 32)[0], _reference("photo", 200, 120, 32)
    with device.MixedBatch(3, max_lf_groups=4, image_errors=True) as mb:
        mb.encode([imgs[0], _with_nan(small, 60, 100), imgs[1]])
        mb.result()
        print("overflow reruns:", mb.overflow_reruns())
        assert mb.overflow_reruns() >= 1, "the case did not exercise the rerun"
        _check_outcomes(mb, [wants[0], small_want, wants[1]], {1})


# ---- the object stays usable; the switch ----
def test_the_object_stays_usable_and_the_switch_is_refused_in_flight():
    from hydrium_amd import device

    imgs, wants = _pictures("photo", 32, [(200, 120), (520, 264), (257, 256)])
    bad = _with_nan(imgs[1], 130, 300)
    with device.MixedBatch(3, image_errors=True) as mb:
        mb.encode([imgs[0], bad, imgs[2]])
        with pytest.raises(device.DeviceError, match="in flight") as e:
            mb.set_image_errors(False)
        assert e.value.code == -14
        _check_outcomes(mb, wants, {1})
        mb.encode(imgs)  # the same sizes: the plan is reused
        _check_outcomes(mb, wants, set())
        mb.set_image_errors(False)
        mb.encode([imgs[0], bad, imgs[2]])
        with pytest.raises(device.DeviceError, match="NaN") as e:
            mb.result()
        assert e.value.code == -14
        mb.encode(imgs)
        _check_outcomes(mb, wants, set())
    with device.FrameBatch(200, 120, 2, image_errors=True) as fb:
        fb.encode([imgs[0], imgs[0]])
        with pytest.raises(device.DeviceError, match="in flight"):
            fb.set_image_errors(False)
        _check_outcomes(fb, [wants[0], wants[0]], set())
        fb.set_image_errors(False)
        fb.encode([imgs[0], _with_nan(imgs[0], 3, 3)])
        with pytest.raises(device.DeviceError, match="NaN"):
            fb.result()
        fb.encode([imgs[0], imgs[0]])
        _check_outcomes(fb, [wants[0], wants[0]], set())
