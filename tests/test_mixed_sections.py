"""The mixed-size batch layout — the product's own mixed planner (csrc/host/mixed.c) and the batched frame layout of
csrc/hip/hydk_tiles.h, what k_batch_prepare_mixed runs — compiled for the host and held, byte for byte, to the host
assembler's file for each image ALONE (frame.c through hydamd_frame_from_streams: file header, one frame, is_last, both
shifts -1).  CPU only: the stage results come from the oracle and the numpy model of the LF coder, as in
test_tiled_sections.py."""
import ctypes as C

import numpy as np
import pytest

from hydrium_amd import api, build as hbuild
from oracle import binding as orc

import content_corpus as cc
import glue
import lf_model

MAXC, ALPHA, GPL = 9, 128, 64

SIX_SHAPES = [(8, 8), (200, 120), (256, 256), (257, 256), (520, 264), (33, 9)]
REPEATED = [(200, 120), (520, 264), (200, 120), (264, 520)]


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    d = C.CDLL(hbuild.HOSTTEST_PATH)
    d.hydt_mixed_from_streams.restype = C.c_int
    d.hydt_mixed_from_streams.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_char_p)]
    d.hydt_mixed_plan_counts.restype = C.c_int
    d.hydt_mixed_plan_counts.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
    d.hydt_free.argtypes = [C.c_void_p]
    return d


_made = {}


def _picture(image, k, w, h):
    """(oracle result, running maximum, the host assembler's file for this picture alone); made once, never changed.
    Picture k of a list has its own seed: equal sizes are still different pictures."""
    key = (k, w, h)
    if key not in _made:
        img = image("photo", w, h, 8, 1234 + 17 * k)
        p = img.ctypes.data
        r, mx = orc.encode_lf_group_ptrs([p, p + 1, p + 2], 3 * w, 3, orc.FMT[img.dtype], 0, w, h, 0, 1, 0)
        md = api.HYDImageMetadata(w, h, 0, -1, -1)
        _made[key] = (r, mx, glue.frame_from_stages(md, True, True, [(0, 0)], [r], mx, None, coded_lf=True))
    return _made[key]


def _mixed(lib, sizes, stages):
    n = len(stages)
    freq = np.zeros((n, MAXC, ALPHA), np.uint32)
    alpha = np.zeros((n, MAXC), np.uint32)
    bits = np.zeros((n, GPL), np.uint32)
    mxs = np.zeros(n, np.uint32)
    keep, arr = [], (glue.LfStream * n)()
    for s, (r, mx, _) in enumerate(stages):
        ncl = r.cluster_to - r.cluster_from
        freq[s, :ncl] = r.freqs[r.cluster_from:r.cluster_to]
        alpha[s, :ncl] = r.alphabet_size[r.cluster_from:r.cluster_to]
        bits[s, :r.num_groups] = r.group_bits
        mxs[s] = mx
        _, lengths, alphabet, pairs, packed, nbits = lf_model.model(np.ascontiguousarray(r.dc, np.int32))
        lengths = np.ascontiguousarray(lengths, np.uint8)
        packed = np.ascontiguousarray(packed, np.uint8)
        keep.append((lengths, packed))
        arr[s] = glue.LfStream(lengths.ctypes.data, alphabet, pairs, packed.ctypes.data if nbits else None, nbits)
    payload = b"".join(r.stream for r, _, _ in stages)
    ws = np.array([w for w, _ in sizes], np.uint32)
    hs = np.array([h for _, h in sizes], np.uint32)
    offs = np.zeros(n + 1, np.uint64)
    out, out_len, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p(None)
    ret = lib.hydt_mixed_from_streams(n, ws.ctypes.data, hs.ctypes.data, arr, freq.ctypes.data, alpha.ctypes.data, bits.ctypes.data,
                                      mxs.ctypes.data, payload, len(payload), offs.ctypes.data, C.byref(out), C.byref(out_len),
                                      C.byref(err))
    assert ret == 0, err.value
    data = bytes((C.c_uint8 * out_len.value).from_address(out.value))
    lib.hydt_free(out)
    return data, [int(o) for o in offs]


def _shapes_planned(lib, sizes):
    ws = np.array([w for w, _ in sizes], np.uint32)
    hs = np.array([h for _, h in sizes], np.uint32)
    n, nbytes = C.c_uint32(0), C.c_size_t(0)
    assert lib.hydt_mixed_plan_counts(len(sizes), ws.ctypes.data, hs.ctypes.data, C.byref(n), C.byref(nbytes)) == 0
    return n.value, nbytes.value


def _hold(lib, sizes, stages):
    wants = [want for _, _, want in stages]
    got, offs = _mixed(lib, sizes, stages)
    # every file starts where the lengths of all files before it put it: the running sum of the reference lengths
    assert offs == [sum(map(len, wants[:k])) for k in range(len(wants) + 1)]
    for k, want in enumerate(wants):
        assert got[offs[k]:offs[k + 1]] == want, (k, sizes[k])
    assert got == b"".join(wants)
    return got, offs


def test_six_shapes_in_one_batch_each_file_what_the_host_writes_for_it_alone(lib, image):
    """more shapes than a tile plan holds; one-group layouts (8x8, 200x120, 256x256, 33x9: one bit-contiguous section)
    beside several-group ones (257x256: two groups, 520x264: six); files that start off word boundaries"""
    stages = [_picture(image, k, w, h) for k, (w, h) in enumerate(SIX_SHAPES)]
    assert [r.num_groups for r, _, _ in stages] == [1, 1, 1, 2, 6, 1]
    assert _shapes_planned(lib, SIX_SHAPES)[0] == 6 > 4
    _, offs = _hold(lib, SIX_SHAPES, stages)
    assert any(o % 4 for o in offs[1:-1])


def test_a_repeated_shape_shares_its_record_and_keeps_its_own_prefix(lib, image):
    stages = [_picture(image, k, w, h) for k, (w, h) in enumerate(REPEATED)]
    assert _shapes_planned(lib, REPEATED)[0] == 3  # 200x120 twice, and 520x264 is not 264x520
    got, offs = _hold(lib, REPEATED, stages)
    a, b = got[offs[0]:offs[1]], got[offs[2]:offs[3]]
    assert a != b  # the same size, other pictures
    # ... and every one of them opens with a file header of its own: the signature, then the same size fields
    assert a[:2] == b[:2] == b"\xff\x0a" and a[:6] == b[:6]
    assert got[offs[1]:offs[1] + 2] == got[offs[3]:offs[3] + 2] == b"\xff\x0a"
    assert got[offs[1]:offs[1] + 6] != got[offs[3]:offs[3] + 6]  # 520x264 against 264x520


def test_the_same_pictures_in_reversed_order_give_the_reversed_files(lib, image):
    stages = [_picture(image, k, w, h) for k, (w, h) in enumerate(SIX_SHAPES)]
    fwd, foffs = _hold(lib, SIX_SHAPES, stages)
    rev, roffs = _hold(lib, SIX_SHAPES[::-1], stages[::-1])
    n = len(stages)
    assert [rev[roffs[k]:roffs[k + 1]] for k in range(n)] == [fwd[foffs[k]:foffs[k + 1]] for k in range(n)][::-1]


def test_one_image_and_the_largest_side(lib, image):
    """a batch of one; and 2048 x 16, the widest one LF group gets (eight groups in a row)"""
    for sizes in ([(232, 188)], [(2048, 16), (16, 300)]):
        _hold(lib, sizes, [_picture(image, 40 + k, w, h) for k, (w, h) in enumerate(sizes)])


@pytest.mark.parametrize("depth", sorted(cc.MIXED))
def test_the_content_corpus_forward_and_reversed(lib, depth):
    """one batch per sample format of the pictures that move the layout's own fields furthest (tests/content_corpus.py):
    files of 102 bytes beside files of 250 KB in one offsets table, HF sections of 4 bytes beside ones above 100 KB, TOCs
    of 10-bit entries only and of 10- and 22-bit ones, an empty LF stream, token 28, log_alphabet_size 7 beside 5 — each
    file what frame.c writes for that picture alone"""
    pictures = cc.MIXED[depth]
    sizes = [(w, h) for _, w, h, _, _ in pictures]
    stages = [(r, mx, want) for r, mx, _, want in (cc.stage(*p) for p in pictures)]
    assert len({want for _, _, want in stages}) == len(stages)
    fwd, foffs = _hold(lib, sizes, stages)
    rev, roffs = _hold(lib, sizes[::-1], stages[::-1])
    n = len(stages)
    assert [rev[roffs[k]:roffs[k + 1]] for k in range(n)] == [fwd[foffs[k]:foffs[k + 1]] for k in range(n)][::-1]
    lens = [len(want) for _, _, want in stages]
    print(f"{depth}-bit corpus batch: files of", lens, "bytes")
    if depth == 8:
        assert min(lens) < 128 and max(lens) > 200 * 1024  # the extremes of one offsets table
    if depth == 32:
        assert [r.log_alphabet_size for r, _, _ in stages] == [7, 5, 5, 7]


def test_what_the_hook_refuses(lib):
    ws, hs = np.array([2049], np.uint32), np.array([8], np.uint32)
    out, out_len, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p(None)
    ret = lib.hydt_mixed_from_streams(1, ws.ctypes.data, hs.ctypes.data, None, None, None, None, None, b"", 0, None, C.byref(out),
                                      C.byref(out_len), C.byref(err))
    assert ret == -14 and b"between 1 and 2048" in err.value
