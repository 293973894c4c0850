"""The batched tile-frame layout (csrc/hip/hydk_tiles.h, what the kernels of assemble_tiles.hip run) compiled for
the host and held to the host assembler (frame.c through hydamd_frame_from_streams), byte for byte.  CPU only: the
stage results come from the oracle and the numpy model of the LF coder, as in test_host_glue.py."""
import ctypes as C

import numpy as np
import pytest

from hydrium_amd import api, build as hbuild
from oracle import binding as orc

import content_corpus as cc
import glue
import lf_model

MAXC, ALPHA, GPL = 9, 128, 64


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    d = C.CDLL(hbuild.HOSTTEST_PATH)
    d.hydt_tiles_from_streams.restype = C.c_int
    d.hydt_tiles_from_streams.argtypes = [C.POINTER(api.HYDImageMetadata), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
    d.hydt_free.argtypes = [C.c_void_p]
    return d


def _stages(img, sx, sy):
    """[(tile, oracle result, running maximum)] for every tile of the image, raster order."""
    h, w, _ = img.shape
    tw, th = api.tile_dims(w, h, sx, sy)
    ntx, nty = -(-w // tw), -(-h // th)
    out = []
    for ty in range(nty):
        for tx in range(ntx):
            x0, y0 = tx * tw, ty * th
            p = img.ctypes.data + (y0 * w + x0) * 3 * img.dtype.itemsize
            isz = img.dtype.itemsize
            r, mx = orc.encode_lf_group_ptrs([p, p + isz, p + 2 * isz], 3 * w, 3, orc.FMT[img.dtype], 0, min(tw, w - x0),
                                             min(th, h - y0), 0, 1, 0)
            out.append(((tx, ty), r, mx))
    return out


def _host_frames(md, stages):
    """every tile's frame from the host assembler: file header once, is_last on the final tile"""
    return [glue.frame_from_stages(md, i == 0, i == len(stages) - 1, [t], [r], mx, None, coded_lf=True)
            for i, (t, r, mx) in enumerate(stages)]


def _batched(lib, md, stages):
    n = len(stages)
    freq = np.zeros((n, MAXC, ALPHA), np.uint32)
    alpha = np.zeros((n, MAXC), np.uint32)
    bits = np.zeros((n, GPL), np.uint32)
    mxs = np.zeros(n, np.uint32)
    keep, arr = [], (glue.LfStream * n)()
    for s, (_, r, mx) in enumerate(stages):
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
    payload = b"".join(r.stream for _, r, _ in stages)
    offs = np.zeros(n + 1, np.uint64)
    out, out_len, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p(None)
    ret = lib.hydt_tiles_from_streams(C.byref(md), n, arr, freq.ctypes.data, alpha.ctypes.data, bits.ctypes.data, mxs.ctypes.data,
                                      payload, len(payload), offs.ctypes.data, C.byref(out), C.byref(out_len), C.byref(err))
    assert ret == 0, err.value
    data = bytes((C.c_uint8 * out_len.value).from_address(out.value))
    lib.hydt_free(out)
    return data, [int(o) for o in offs]


@pytest.mark.parametrize("w,h", [(8, 8), (256, 256), (232, 188)])
def test_single_group_frame_equals_the_host_assembler(lib, image, w, h):
    img = image("photo", w, h)
    md = api.HYDImageMetadata(w, h, 0, 0, 0)
    st = _stages(img, 0, 0)
    assert len(st) == 1 and st[0][1].num_groups == 1
    want = _host_frames(md, st)
    got, offs = _batched(lib, md, st)
    assert offs == [0, len(want[0])]
    assert got == want[0]


def test_three_frames_single_and_four_group_mixed(lib, image):
    # 2056 x 256 in 1024 x 256 tiles: two four-group frames (TOC, padded sections) and one 8 x 256 single-group frame
    w, h = 2056, 256
    img = image("photo", w, h)
    md = api.HYDImageMetadata(w, h, 0, 2, 0)
    st = _stages(img, 2, 0)
    assert [r.num_groups for _, r, _ in st] == [4, 4, 1]
    want = _host_frames(md, st)
    got, offs = _batched(lib, md, st)
    # every frame starts where the sizes of all frames before it put it
    assert offs == [0, len(want[0]), len(want[0]) + len(want[1]), sum(map(len, want))]
    assert got == b"".join(want)
    # the file header once, in front of tile 0: the other frames are what the host builds without it
    alone = glue.frame_from_stages(md, False, False, [st[1][0]], [st[1][1]], st[1][2], None, coded_lf=True)
    assert got[offs[1]:offs[2]] == alone
    # is_last sits on the final tile only: the same tile as a middle one reads differently
    not_last = glue.frame_from_stages(md, False, False, [st[2][0]], [st[2][1]], st[2][2], None, coded_lf=True)
    assert got[offs[2]:] != not_last and got[offs[2]:] == want[2]


def test_single_group_frames_in_sequence_off_word_boundaries(lib, image):
    # 520 x 264 in 256 x 256 tiles: six frames, ragged edges, frames that start at any byte
    w, h = 520, 264
    img = image("photo", w, h)
    md = api.HYDImageMetadata(w, h, 0, 0, 0)
    st = _stages(img, 0, 0)
    assert len(st) == 6 and all(r.num_groups == 1 for _, r, _ in st)
    want = _host_frames(md, st)
    got, offs = _batched(lib, md, st)
    assert offs[-1] == sum(map(len, want))
    assert got == b"".join(want)


@pytest.mark.parametrize("picture,sx,sy", cc.TILED, ids=[f"{p[0]}-{p[1]}x{p[2]}-{p[3]}b-shift{sx}{sy}" for p, sx, sy in cc.TILED])
def test_the_content_corpus_in_tile_mode(lib, picture, sx, sy):
    """tests/content_corpus.py: neighbouring tiles that are entirely different frames (black, noise, primaries, photo:
    frames of 4 and of 115974 HF bytes side by side), frames of nothing but 4-byte sections at 16 bit, and the empty LF
    stream of a black 8 x 8 tile — every frame what frame.c writes for that tile"""
    img = cc.picture(*picture)
    h, w, _ = img.shape
    md = api.HYDImageMetadata(w, h, 0, sx, sy)
    st = _stages(img, sx, sy)
    want = _host_frames(md, st)
    got, offs = _batched(lib, md, st)
    assert offs == [sum(map(len, want[:k])) for k in range(len(want) + 1)]
    for k, frame in enumerate(want):
        assert got[offs[k]:offs[k + 1]] == frame, (k, st[k][0])
    assert got == b"".join(want)
    print(picture, (sx, sy), "frames of", [len(f) for f in want], "bytes")
