"""GPU: a sample format per image in one mixed-size batch — hydamd_encode_mixed_formats (csrc/host/mixed.c) through
device.MixedBatch.encode(sample_fmts=...).  8-bit, 16-bit and float pictures share one launch group; every file is compared
whole with what the compiled reference writes for that picture alone in its own format."""
import pytest

from conftest import has_gpu
from test_gpu_image_status import _check_outcomes, _with_nan
from test_gpu_mixed_batch import _check, _check_on_device, _image, _reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def _mix(spec):
    """spec: (depth, (w, h)) per picture, each with a seed of its own -> device tensors, reference files"""
    seeds = [1234 + 17 * k for k in range(len(spec))]
    imgs = [_image("photo", w, h, depth, s)[0] for (depth, (w, h)), s in zip(spec, seeds)]
    wants = [_reference("photo", w, h, depth, s) for (depth, (w, h)), s in zip(spec, seeds)]
    return imgs, wants


FOUR = [(8, (200, 120)), (16, (232, 188)), (32, (200, 120)), (8, (256, 256))]


def test_three_formats_in_one_batch_forward_and_reversed():
    from hydrium_amd import device

    imgs, wants = _mix(FOUR)
    assert len(set(wants)) == 4
    with device.MixedBatch(4) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check_on_device(mb, wants[::-1])
        with pytest.raises(ValueError, match="share one sample format"):  # without sample_fmts: as before
            mb.encode(imgs)
        assert mb.overflow_reruns() == 0


def test_an_integer_only_mix_keeps_the_lane_form_chains():
    from hydrium_amd import device

    imgs, wants = _mix([(8, (200, 120)), (16, (232, 188)), (16, (520, 264)), (8, (33, 9))])
    with device.MixedBatch(4) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        tuples = [([t.data_ptr() + c * t.element_size() for c in range(3)], t.stride(0), t.stride(1), t.shape[1], t.shape[0]) for t in imgs]
        mb.encode(tuples, sample_fmts=[0, 1, 1, 0])  # the formats named explicitly, for bare addresses
        _check(mb, wants)


def test_formats_and_lf_group_counts_mixed():
    from hydrium_amd import device

    spec = [(8, (200, 120)), (16, (2049, 64)), (32, (200, 120)), (8, (256, 256)), (32, (2049, 16))]
    imgs, wants = _mix(spec)
    with device.MixedBatch(5, max_lf_groups=7) as mb:
        mb.encode(imgs, sample_fmts="each")
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1], sample_fmts="each")
        _check_on_device(mb, wants[::-1])


def test_a_nan_in_the_float_picture_of_a_mixed_format_batch():
    from hydrium_amd import device

    imgs, wants = _mix(FOUR)
    given = [imgs[0], imgs[1], _with_nan(imgs[2], 60, 100), imgs[3]]
    with device.MixedBatch(4, image_errors=True) as mb:
        mb.encode(given, sample_fmts="each")
        _check_outcomes(mb, wants, {2})
        mb.encode(imgs, sample_fmts="each")
        _check_outcomes(mb, wants, set())
    with device.MixedBatch(4) as mb:  # without the switch the batch fails as a one-format batch does
        mb.encode(given, sample_fmts="each")
        with pytest.raises(device.DeviceError, match="NaN"):
            mb.result()


def test_a_bad_format_is_refused_and_nothing_is_enqueued():
    from hydrium_amd import device

    imgs, wants = _mix(FOUR[:2])
    tuples = [([t.data_ptr() + c * t.element_size() for c in range(3)], t.stride(0), t.stride(1), t.shape[1], t.shape[0]) for t in imgs]
    with device.MixedBatch(2) as mb:
        for fmts in ([0, 7], [7, 1], [0, -1]):
            with pytest.raises(device.DeviceError, match="Invalid Sample Format") as e:
                mb.encode(tuples, sample_fmts=fmts)
            assert e.value.code == -14
            with pytest.raises(device.DeviceError, match="no batch in flight"):
                mb.result()
        assert mb.d.hydamd_encode_mixed_formats(mb.h, 2, None, None) == -14
        mb.encode(tuples, sample_fmts=[0, 1])
        _check(mb, wants)


def test_one_object_alternating_between_mixed_and_one_format_batches_of_the_same_sizes():
    from hydrium_amd import device

    sizes = [(200, 120), (232, 188)]
    mixed, mixed_wants = _mix([(8, sizes[0]), (32, sizes[1])])
    plain8, plain8_wants = _mix([(8, sizes[0]), (8, sizes[1])])
    plain32, plain32_wants = _mix([(32, sizes[0]), (32, sizes[1])])
    with device.MixedBatch(2) as mb:  # one plan for all five batches: it depends on the sizes only
        mb.encode(plain8)
        _check(mb, plain8_wants)
        mb.encode(mixed, sample_fmts="each")
        _check_on_device(mb, mixed_wants)
        mb.encode(plain32)
        _check(mb, plain32_wants)
        mb.encode(mixed[::-1], sample_fmts="each")  # other sizes per position: a new plan
        _check(mb, mixed_wants[::-1])
        mb.encode(plain8, sample_fmts="each")
        _check_on_device(mb, plain8_wants)
