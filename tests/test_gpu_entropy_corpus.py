"""GPU: the ANS table kernel (k_build_tables) and the rANS chains (k_rans_encode, k_rans_lanes, k_rans_emit) on the pictures
of tests/entropy_corpus.py, which reach what no other picture of the suite does: every branch of the normalisation's
excess loop, 64-entry tables and the steps of the table size at running maxima of 32/33 and 64/65, a running maximum handed
to an LF group whose own alphabet is 1, and chains whose lengths sit on the kernels' own boundaries (16, 64, 128, each with
one less and one more).  tests/test_entropy_corpus.py proves on the CPU that the pictures reach all that.

Stage level: tables, symbol counts, section bits, offsets and bytes against the CPU oracle, per slot.  File level: the four
device-side file builders and hyd_send_tile against the compiled reference.  Bit-exact everywhere; nothing thinned."""
import numpy as np
import pytest

import entropy_corpus as ec
from conftest import has_gpu, reference_expected
from hydrium_amd import api
from test_gpu_assembler import _assemble_on_device, _blobs_on_device, _cuda, _host_assembly
from test_gpu_mixed_batch import _check_on_device

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

_cache = {}


def _tensor(img):
    """the picture on the device; made once"""
    import torch

    if id(img) not in _cache:
        _cache[id(img)] = (_cuda(img), img)
        torch.cuda.synchronize()
    return _cache[id(img)][0]


def _float_photo(w, h):
    """synth's photo in float32, samples in [0, 1]: log_alphabet_size 5"""
    from hydrium_amd import synth

    key = ("photo", w, h)
    if key not in _cache:
        img = synth.make_image_f32("photo", w, h)
        img.setflags(write=False)
        _cache[key] = img
    return _cache[key]


def _reference(img):
    """the compiled reference's file for that picture alone; made once per picture and never changed"""
    from oracle import refprobe

    assert reference_expected()
    key = ("ref", id(img))
    if key not in _cache:
        _cache[key] = (api.encode_image(refprobe.reference_library(optimised=True), img, out_buf_size=1 << 22), img)
    return _cache[key][0]


# ---- stage level -----------------------------------------------------------------------------------------------------------
def _check_slots(ctx, results, what):
    """every slot of the frame the context has just coded against the oracle's result for that LF group: tables (frequencies,
    alphabets, log_alphabet_size, running maximum), symbol counts, section bits and offsets, section bytes"""
    payload = ctx.read_payload()
    at = 0
    for slot, res in enumerate(results):
        freq, alpha, log_alpha, run_max = ctx.read_tables(slot)
        ncl = res.cluster_to - res.cluster_from
        assert (log_alpha, run_max) == (res.log_alphabet_size, res.max_alphabet_size), (what, slot)
        assert np.array_equal(alpha[:ncl], res.alphabet_size[res.cluster_from:res.cluster_to]), (what, slot)
        assert np.array_equal(freq[:ncl], res.freqs[res.cluster_from:res.cluster_to]), (what, slot)
        assert np.array_equal(ctx.read_symbol_counts(slot)[:res.num_groups], res.group_symbols), (what, slot)
        bits, offs = ctx.read_sections(slot)
        assert np.array_equal(bits[:res.num_groups], res.group_bits), (what, slot)
        assert np.array_equal(offs[:res.num_groups], res.group_offset + at), (what, slot)
        assert payload[at:at + len(res.stream)] == res.stream, (what, slot)
        at += len(res.stream)
    assert at == len(payload), what


STAGE = [(name, form) for name in ec.NAMES for form in ((4,) if ec.is_float(name) else (4, 5))]


@pytest.mark.parametrize("name,form", STAGE, ids=[f"{n}-form{f}" for n, f in STAGE])
def test_every_corpus_picture_stage_by_stage(name, form):
    """integer pictures by the wave form (4) and the lane form (5), float pictures by form 4's self-emitting chain; pictures
    of two LF groups carry the running maximum in send order"""
    from hydrium_amd import device

    results = ec.stage(name)
    t = _tensor(ec.picture(name))
    with device.DeviceContext(0, len(results), 0, debug_planes=False) as ctx:
        ctx.set_rans_waves(form)
        ctx.encode_image_tensor(t)
        ctx.sync()
        _check_slots(ctx, results, name)


@pytest.mark.parametrize("form", [4, 5])
def test_one_context_codes_excess_then_log6_then_a_photo_then_excess_again(image, form):
    """tables of a 64-entry frame must not survive into a 32-entry one, nor flattened frequencies into the next frame"""
    from hydrium_amd import device
    from oracle import binding as orc

    photo = image("photo", 264, 200, 8)
    want_photo, _ = orc.encode_lf_group(photo)
    assert want_photo.log_alphabet_size == 5
    frames = [("excess_flatten", ec.picture("excess_flatten"), ec.stage("excess_flatten")),
              ("noise_36", ec.picture("noise_36"), ec.stage("noise_36")),
              ("photo", photo, (want_photo,)),
              ("excess_coef", ec.picture("excess_coef"), ec.stage("excess_coef")),
              ("max_64", ec.picture("max_64"), ec.stage("max_64")),
              ("excess_flatten", ec.picture("excess_flatten"), ec.stage("excess_flatten"))]
    with device.DeviceContext(0, 1, 0, debug_planes=False) as ctx:
        ctx.set_rans_waves(form)
        for what, img, results in frames:
            ctx.encode_image_tensor(_tensor(img))
            ctx.sync()
            _check_slots(ctx, results, what)


# ---- whole files against the compiled reference -------------------------------------------------------------------------------
def _mixed_pictures():
    """log_alphabet_size 5, 6, 7, 6, 5, 6, 7 beside each other"""
    return [_float_photo(64, 48), ec.picture("noise_36"), ec.picture("max_65"), ec.picture("max_33"), ec.picture("max_32"),
            ec.picture("max_64"), (ec.picture("noise_36") * np.float32(1e5)).astype(np.float32)]


def test_mixed_batch_of_log5_log6_and_log7_pictures_forward_and_reversed():
    from hydrium_amd import device
    from oracle import binding as orc

    pictures = _cache.setdefault("mixed", _mixed_pictures())
    assert [orc.encode_lf_group(p)[0].log_alphabet_size for p in pictures] == [5, 6, 7, 6, 5, 6, 7]
    imgs, wants = [_tensor(p) for p in pictures], [_reference(p) for p in pictures]
    assert len(set(wants)) == len(wants)
    with device.MixedBatch(len(pictures)) as mb:
        for order in (slice(None), slice(None, None, -1)):
            mb.encode(imgs[order])
            _check_on_device(mb, wants[order])


def test_frame_batch_of_log6_log5_log6_frames():
    """the middle frame's 32-entry tables between two frames of 64-entry ones, and the same batch rotated by one"""
    from hydrium_amd import device

    pictures = [ec.picture("noise_36"), _float_photo(64, 48), ec.picture("noise_49")]
    imgs, wants = [_tensor(p) for p in pictures], [_reference(p) for p in pictures]
    with device.FrameBatch(64, 48, 3) as fb:
        fb.encode(imgs)
        _check_on_device(fb, wants)
        fb.encode(imgs[1:] + imgs[:1])
        _check_on_device(fb, wants[1:] + wants[:1])


@pytest.mark.parametrize("name", ec.HANDOVER)
@pytest.mark.parametrize("parts", [[[0, 1]], [[0], [1]]], ids=["one-shard", "two-shards"])
def test_assembler_on_the_handover_pictures(name, parts):
    """two LF groups whose table sizes differ or are handed on, as one shard and as two (the running maximum then crosses
    from shard to shard on the device)"""
    img = ec.picture(name)
    h, w, _ = img.shape
    blobs = _blobs_on_device(_tensor(img), w, h, parts)
    md = api.HYDImageMetadata(w, h, 0, -1, -1)
    got = _assemble_on_device(md, blobs, parts)
    assert got == _host_assembly(md, blobs)
    assert got == _reference(img)


@pytest.mark.parametrize("name", ["noise_36", "max_64", "excess_flatten", "excess_coef"] + list(ec.HANDOVER))
def test_hyd_send_tile_files(name):
    img = ec.picture(name)
    got = api.encode_image(api.Library(), img, out_buf_size=1 << 22)
    want = _reference(img)
    assert len(got) == len(want) and got == want
