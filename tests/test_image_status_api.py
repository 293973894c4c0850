"""An outcome per image and a sample format per image for the device batches, without a GPU: the shipped library exports
the new entry points (and no hook), the Python binding agrees with the header, the batched layout with a SKIPPED frame —
hydk_tiles.h's hydk_frame_flagged / hydk_place_piece, what k_batch_place runs, compiled for the host — is held to the host
assembler's files for the frames that remain, and MixedBatch.encode's reading of sample_fmts."""
import ctypes as C

import numpy as np
import pytest

from hydrium_amd import build as hbuild, device

import test_mixed_sections as ms
from test_mixed_batch_layout import _ctypes_kind, _exported, _kind, _prototype

SYMBOLS = ["hydamd_set_bad_sample_per_slot", "hydamd_read_bad_slots", "hydamd_mixed_set_image_errors", "hydamd_mixed_image_status",
           "hydamd_mixed_image_status_device", "hydamd_batch_set_image_errors", "hydamd_batch_image_status",
           "hydamd_batch_image_status_device", "hydamd_encode_mixed_formats"]
PIECES = 8  # HYDK_TILE_PIECES


def test_the_shipped_library_exports_the_new_entry_points_and_no_hook():
    shipped = _exported(hbuild.build())
    assert not [s for s in SYMBOLS if s not in shipped]
    assert not [s for s in shipped if s.startswith("hydt_") or s.startswith("hydk_")]
    assert "hydt_mixed_from_streams_skip" in _exported(hbuild.PROBE_PATH)  # the probe flavour is where the hook lives


@pytest.mark.parametrize("name", SYMBOLS)
def test_binding_and_header_agree(name):
    d = device.dll()
    ret, args = _prototype(name)
    fn = getattr(d, name)
    assert len(fn.argtypes) == len(args), (name, args)
    for decl, t in zip(args, fn.argtypes):
        assert _ctypes_kind(t) == _kind(decl), (name, decl, t)
    assert _ctypes_kind(fn.restype) == _kind(ret + " x"), (name, ret, fn.restype)


def test_the_status_word_is_the_header_s():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hydrium_amd.h")).read()
    assert int(re.search(r"#define HYDAMD_IMAGE_BAD_SAMPLE (\d+)u", text).group(1)) == device.IMAGE_BAD_SAMPLE == 1


# ---- the layout with a skipped frame ----
@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    d = C.CDLL(hbuild.HOSTTEST_PATH)
    d.hydt_mixed_from_streams_skip.restype = C.c_int
    d.hydt_mixed_from_streams_skip.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
    d.hydt_free.argtypes = [C.c_void_p]
    return d


def _skipping(lib, sizes, stages, flagged):
    """the batch with the images of `flagged` marked as the context marks a slot: (bytes, offsets, statuses, pieces)"""
    n = len(stages)
    freq = np.zeros((n, ms.MAXC, ms.ALPHA), np.uint32)
    alpha = np.zeros((n, ms.MAXC), np.uint32)
    bits = np.zeros((n, ms.GPL), np.uint32)
    mxs = np.zeros(n, np.uint32)
    keep, arr = [], (ms.glue.LfStream * n)()
    for s, (r, mx, _) in enumerate(stages):
        ncl = r.cluster_to - r.cluster_from
        freq[s, :ncl] = r.freqs[r.cluster_from:r.cluster_to]
        alpha[s, :ncl] = r.alphabet_size[r.cluster_from:r.cluster_to]
        bits[s, :r.num_groups] = r.group_bits
        mxs[s] = mx
        _, lengths, alphabet, pairs, packed, nbits = ms.lf_model.model(np.ascontiguousarray(r.dc, np.int32))
        lengths = np.ascontiguousarray(lengths, np.uint8)
        packed = np.ascontiguousarray(packed, np.uint8)
        keep.append((lengths, packed))
        arr[s] = ms.glue.LfStream(lengths.ctypes.data, alphabet, pairs, packed.ctypes.data if nbits else None, nbits)
    payload = b"".join(r.stream for r, _, _ in stages)
    ws = np.array([w for w, _ in sizes], np.uint32)
    hs = np.array([h for _, h in sizes], np.uint32)
    flags = np.array([7 if k in flagged else 0 for k in range(n)], np.uint32)  # any non-zero word flags the slot
    offs = np.zeros(n + 1, np.uint64)
    status = np.full(n, 99, np.uint32)
    pieces = np.zeros((n * PIECES, 2), np.uint64)
    out, out_len, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p(None)
    ret = lib.hydt_mixed_from_streams_skip(n, ws.ctypes.data, hs.ctypes.data, arr, freq.ctypes.data, alpha.ctypes.data, bits.ctypes.data,
                                           mxs.ctypes.data, payload, len(payload), flags.ctypes.data, offs.ctypes.data, status.ctypes.data,
                                           pieces.ctypes.data, C.byref(out), C.byref(out_len), C.byref(err))
    assert ret == 0, err.value
    data = bytes((C.c_uint8 * out_len.value).from_address(out.value)) if out_len.value else b""
    lib.hydt_free(out)
    return data, [int(o) for o in offs], status.tolist(), pieces.astype(object)


def _hold(lib, sizes, stages, flagged):
    n = len(stages)
    kept = [b"" if k in flagged else want for k, (_, _, want) in enumerate(stages)]
    got, offs, status, pieces = _skipping(lib, sizes, stages, flagged)
    assert status == [1 if k in flagged else 0 for k in range(n)]
    assert offs == [sum(map(len, kept[:k])) for k in range(n + 1)]
    assert got == b"".join(kept)
    # the piece list keeps its length and its order: starts and ends never go back (what the copy kernel's search rests on),
    # a skipped frame's pieces are empty at its offset, every other frame's stay inside its file
    dst, ends = [int(p[0]) for p in pieces], [int(p[0]) + int(p[1]) for p in pieces]
    assert dst == sorted(dst) and ends == sorted(ends)
    for f in range(n):
        mine = range(f * PIECES, (f + 1) * PIECES)
        if f in flagged:
            assert all(dst[i] == ends[i] == 8 * offs[f] for i in mine), f
        else:
            assert all(8 * offs[f] <= dst[i] <= ends[i] <= 8 * offs[f + 1] for i in mine), f
            assert any(ends[i] > dst[i] for i in mine)
    return offs


@pytest.mark.parametrize("flagged", [{0}, {2}, {3}, {4}, {5}, {1, 2}, {0, 1, 2, 3, 4, 5}, set()],
                         ids=lambda s: "skip-" + ("".join(map(str, sorted(s))) or "none"))
def test_a_skipped_frame_yields_no_bytes_and_its_neighbours_meet(lib, image, flagged):
    """one-group frames (8x8, 200x120, 256x256, 33x9: one bit-contiguous section) and several-group ones (257x256, 520x264)
    skipped first, in the middle and last; the files on both sides are what the host assembler writes for them alone"""
    sizes = ms.SIX_SHAPES
    stages = [ms._picture(image, k, w, h) for k, (w, h) in enumerate(sizes)]
    assert [r.num_groups for r, _, _ in stages] == [1, 1, 1, 2, 6, 1]
    _hold(lib, sizes, stages, flagged)
    if not flagged:
        assert _skipping(lib, sizes, stages, flagged)[0] == ms._mixed(lib_plain(), sizes, stages)[0]


def test_some_neighbours_of_a_skipped_frame_meet_inside_an_output_word(image):
    """what the cases above are for: where the file before a skipped frame ends off a word boundary, the file behind it
    starts inside the same output word"""
    lens = [len(ms._picture(image, k, w, h)[2]) for k, (w, h) in enumerate(ms.SIX_SHAPES)]
    assert any(sum(lens[:k]) % 4 for k in (2, 3, 4, 5))  # the skipped frames 2, 3, 4, 5 start (and end) there


_plain = []


def lib_plain():
    if not _plain:
        d = C.CDLL(hbuild.HOSTTEST_PATH)
        d.hydt_mixed_from_streams.restype = C.c_int
        d.hydt_mixed_from_streams.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                              C.POINTER(C.c_char_p)]
        d.hydt_free.argtypes = [C.c_void_p]
        _plain.append(d)
    return _plain[0]


# ---- MixedBatch.encode's sample_fmts, as far as the device is not needed ----
def _tensors():
    import torch

    return [torch.zeros((5, 7, 3), dtype=torch.uint8), torch.zeros((6, 4, 3), dtype=torch.int16), torch.zeros((3, 9, 4), dtype=torch.float32)]


def test_sample_fmts_each_takes_every_tensor_s_own_dtype():
    ts = _tensors()
    descs, fmts = device.mixed_descriptors(ts, sample_fmts="each")
    assert fmts == [0, 1, 2]
    assert [(d.width, d.height, d.row_stride, d.pixel_stride) for d in descs] == [(7, 5, 21, 3), (4, 6, 12, 3), (9, 3, 36, 4)]
    assert [d.src[1] - d.src[0] for d in descs] == [1, 2, 4] and descs[2].src[0] == ts[2].data_ptr()
    planes = [ts[2][:, :, c].contiguous() for c in range(3)]
    assert device.mixed_descriptors([ts[0], planes], sample_fmts="each")[1] == [0, 2]


def test_a_list_names_the_formats_of_address_tuples():
    ts = _tensors()
    tuples = [([t.data_ptr() + c * t.element_size() for c in range(3)], t.stride(0), t.stride(1), t.shape[1], t.shape[0]) for t in ts]
    descs, fmts = device.mixed_descriptors(tuples, sample_fmts=[0, 1, 2])
    assert fmts == [0, 1, 2] and [d.width for d in descs] == [7, 4, 9]
    assert device.mixed_descriptors([ts[0], tuples[2]], sample_fmts=(0, 2))[1] == [0, 2]
    assert device.mixed_descriptors(tuples[:2], sample_fmts=[0, 7])[1] == [0, 7]  # no format: the library's to refuse
    assert device.mixed_descriptors(tuples[:2], sample_fmt=1, sample_fmts="each")[1] == [1, 1]
    with pytest.raises(ValueError, match="one format per image"):
        device.mixed_descriptors(tuples, sample_fmts=[0, 1])
    with pytest.raises(ValueError, match="disagrees"):
        device.mixed_descriptors(ts, sample_fmts=[0, 2, 2])
    with pytest.raises(ValueError, match="need sample_fmt"):
        device.mixed_descriptors(tuples, sample_fmts="each")
    with pytest.raises(ValueError, match="each"):
        device.mixed_descriptors(ts, sample_fmts="all")


def test_without_sample_fmts_a_call_has_one_format_as_before():
    ts = _tensors()
    with pytest.raises(ValueError, match="share one sample format"):
        device.mixed_descriptors(ts)
    with pytest.raises(ValueError, match="share one sample format"):
        device.mixed_descriptors(ts[:1], sample_fmt=2)
    assert device.mixed_descriptors([ts[0], ts[0]])[1] == [0, 0]
    assert device.mixed_descriptors([], None)[1] == []
    t = ts[2]
    with pytest.raises(ValueError, match="need sample_fmt"):
        device.mixed_descriptors([([t.data_ptr()] * 3, 36, 4, 9, 3)])
    assert device.mixed_descriptors([([t.data_ptr()] * 3, 36, 4, 9, 3)], sample_fmt=2)[1] == [2]
