"""GPU: the four device-side file builders — device.MixedBatch, device.FrameBatch, device.TiledImage and
device.Assembler — on the content that moves their own data-dependent fields furthest (tests/content_corpus.py: HF
sections of 4 bytes beside ones above 100 KB, TOCs of the 10-bit class only and of the 10- and 22-bit classes, the empty
LF stream, token 28, log_alphabet_size 7 beside 5, files of 102 bytes beside files of 390 KB in one offsets table).
Every file and every table is compared whole with what the compiled reference writes; no tolerance anywhere.

And k_pieces_copy itself, which stores the bytes of all four: launched on crafted piece lists through the probe
flavour's hook (hydt_pieces_copy_device, csrc/hip/assemble.hip) and held, over the WHOLE buffer, to the bit-by-bit model
of tests/test_pieces.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import content_corpus as cc
import test_pieces as tp
from conftest import has_gpu, reference_expected
from hydrium_amd import api, build as hbuild
from test_gpu_assembler import _assemble_on_device, _blobs_on_device, _cuda, _host_assembly
from test_gpu_mixed_batch import _check_on_device

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

_cache = {}


def _tensor(p):
    """the picture on the device; made once"""
    import torch

    if ("t", p) not in _cache:
        _cache[("t", p)] = _cuda(cc.picture(*p))
        torch.cuda.synchronize()
    return _cache[("t", p)]


def _reference(p, sx=-1, sy=-1):
    """the compiled reference's file for that picture alone; made once per picture and never changed"""
    from oracle import refprobe

    assert reference_expected()
    key = ("ref", p, sx, sy)
    if key not in _cache:
        _cache[key] = api.encode_image(refprobe.reference_library(optimised=True), cc.picture(*p), out_buf_size=1 << 22, shift_x=sx,
                                       shift_y=sy)
    return _cache[key]


# ---- MixedBatch ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """ONE object for the batches of all three sample formats: the plan is rebuilt between them"""
    from hydrium_amd import device

    with device.MixedBatch(max(map(len, cc.MIXED.values()))) as mb:
        yield mb


@pytest.mark.parametrize("depth", sorted(cc.MIXED))
def test_mixed_batches_forward_and_reversed_on_one_object(mixed, depth):
    """(depth 32: 1614 of float_neg's 1683 LF ints are INT_MIN — the reference's cube root of a negative weighted sum is
    some 1e12, and its float -> int cast gives INT_MIN for what does not fit; the transform kernel converts float input
    the same way, and the LF coder treats the residual symbol 0xFFFFFFFF as the reference's run detector does)"""
    pictures = cc.MIXED[depth]
    imgs, wants = [_tensor(p) for p in pictures], [_reference(p) for p in pictures]
    assert len(set(wants)) == len(wants)
    for order in (slice(None), slice(None, None, -1)):
        mixed.encode(imgs[order])
        print(f"{depth}-bit: files of", [len(w) for w in wants[order]], "bytes; overflow reruns so far:", mixed.overflow_reruns())
        _check_on_device(mixed, wants[order])


@pytest.mark.parametrize("picture", cc.MIXED[32], ids=[p[0] for p in cc.MIXED[32]])
def test_each_float_picture_alone(picture):
    """the pictures of the float batch one by one, so that one that differs does not hide the others: float_neg (its
    LF stream starts with the symbol 0xFFFFFFFF), float_wide (a running alphabet maximum of 72, log_alphabet_size 7, 71 LF
    ints of INT_MIN), float_photo and black"""
    from hydrium_amd import device

    with device.MixedBatch(1) as mb:
        mb.encode([_tensor(picture)])
        _check_on_device(mb, [_reference(picture)])


# ---- FrameBatch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pictures", cc.BATCH, ids=[f"{b[0][0]}-{b[0][1]}x{b[0][2]}-{b[0][3]}b" for b in cc.BATCH])
def test_same_shape_batches_and_the_same_batch_rotated_by_one(pictures):
    """... rotated: a file of a few hundred bytes lands where one of hundreds of KB stood, on the same object"""
    from hydrium_amd import device

    _, w, h, _, _ = pictures[0]
    imgs, wants = [_tensor(p) for p in pictures], [_reference(p) for p in pictures]
    with device.FrameBatch(w, h, len(pictures)) as fb:
        fb.encode(imgs)
        _check_on_device(fb, wants)
        fb.encode(imgs[1:] + imgs[:1])
        _check_on_device(fb, wants[1:] + wants[:1])
        print((w, h), "files of", [len(x) for x in wants], "bytes; overflow reruns:", fb.overflow_reruns())


# ---- TiledImage ------------------------------------------------------------------------------------------------------------
TILED = [(p, sx, sy, 0) for p, sx, sy in cc.TILED] + [(cc.TILED[0][0], 0, 0, 2)]  # launch groups of two: the running offset
#                                                                                   crosses them between a black tile and a noise tile


@pytest.mark.parametrize("picture,sx,sy,per_launch", TILED, ids=[f"{p[0]}-{p[1]}x{p[2]}-{p[3]}b-shift{sx}{sy}-launch{n}" for p, sx, sy, n in TILED])
def test_tiled_files(picture, sx, sy, per_launch):
    from hydrium_amd import device

    _, w, h, _, _ = picture
    want = _reference(picture, sx, sy)
    with device.TiledImage(w, h, sx, sy, tiles_per_launch=per_launch) as ti:
        ti.encode(_tensor(picture))
        got = bytes(ti.read())
        print(picture, (sx, sy), len(want), "bytes; overflow reruns:", ti.overflow_reruns())
    assert len(got) == len(want) and got == want


# ---- Assembler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("picture", cc.ASSEMBLER, ids=[p[0] for p in cc.ASSEMBLER])
@pytest.mark.parametrize("parts", [[[0, 1]], [[0], [1]]], ids=["one-shard", "two-shards"])
def test_a_frame_of_a_noise_lf_group_and_a_black_one(picture, parts):
    """sections of 4 (with two presets: 5) bytes and of 100 KB in one TOC, an HF piece of a few dozen bytes beside one
    of a megabyte"""
    _, w, h, _, _ = picture
    img = cc.picture(*picture)
    blobs = _blobs_on_device(_tensor(picture), w, h, parts)
    md = api.HYDImageMetadata(w, h, 0, -1, -1)
    got = _assemble_on_device(md, blobs, parts)
    assert got == _host_assembly(md, blobs)
    assert got == api.encode_image(api.Library(), img, out_buf_size=1 << 22)
    assert got == _reference(picture)


# ---- k_pieces_copy against the bit model -----------------------------------------------------------------------------------
def _max_pieces():
    text = open(os.path.join(hbuild.CSRC, "hip", "hydk_asm_common.h")).read()
    return int(re.search(r"#define HYDK_COPY_MAX_PIECES (\d+)", text).group(1))


class _OnDevice:
    """What tests/test_pieces.py calls the host composer through, answered by the kernel: the same arguments, plus the
    lengths of the two buffers (test_pieces' own: its SRC, and _out_size of the range) and the range's error word."""

    def __init__(self, d, err_word=0):
        self.d, self.err_word = d, err_word

    def hydt_compose_pieces(self, dst, n, off, count, src, lo, nbytes, out):
        assert src == tp.SRC.ctypes.data
        return self.d.hydt_pieces_copy_device(dst, n, off, count, src, tp.SRC.nbytes, lo, nbytes, self.err_word, out, tp._out_size(lo, nbytes))


@pytest.fixture(scope="module")
def probe():
    from hydrium_amd import preload_hip_runtime

    preload_hip_runtime()
    d = C.CDLL(hbuild.PROBE_PATH)
    d.hydt_pieces_copy_device.restype = C.c_int
    d.hydt_pieces_copy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                          C.c_uint32, C.c_void_p, C.c_uint64]
    return d


def test_the_copy_kernel_on_the_crafted_lists_of_the_host_test(probe):
    """every list tests/test_pieces.py holds the composer to on the host, through the kernel: the full buffer, fill bytes
    included, equals the model"""
    dev = _OnDevice(probe)
    for end in (31, 32, 33):
        tp.test_piece_ends_around_a_word_boundary(dev, end)
    tp.test_three_pieces_inside_one_word(dev)
    tp.test_empty_pieces(dev)
    for off in (0, 1, 2, 3, 4093):
        tp.test_source_alignment(dev, off)
    tp.test_one_bit(dev)
    tp.test_gap_reads_as_zero(dev)
    tp.test_range_edges_leave_the_neighbours_alone(dev)
    tp.test_random_lists(dev)


def test_the_copy_kernel_where_a_thread_handles_more_than_one_word(probe, monkeypatch):
    """1024 blocks of 256 threads: a range longer than 262144 words goes round the grid-stride loop.  1.5 MB from three
    long pieces at odd bit positions, their sources at other byte alignments; the whole range, and one as long that
    starts and ends off word boundaries"""
    big = np.random.default_rng(23).integers(0, 256, 1_600_000, dtype=np.uint8)
    monkeypatch.setattr(tp, "SRC", big)
    monkeypatch.setattr(tp, "SRC_BITS", np.unpackbits(big, bitorder="little"))
    pieces = [(5, 4_000_003, 1), (5 + 4_000_003, 4_100_001, 500_002), (5 + 8_100_004 + 27, 4_200_000, 1_050_003)]
    end = (pieces[-1][0] + pieces[-1][1] + 7) // 8
    assert end > 4 * 1024 * 256 and max(off + (n + 7) // 8 for _, n, off in pieces) <= big.nbytes
    dev = _OnDevice(probe)
    tp._check(dev, pieces)
    tp._check(dev, pieces, lo=13, nbytes=end - 13 - 2)


def test_the_copy_kernel_on_the_longest_list_it_keeps_in_lds(probe):
    n = _max_pieces()
    assert n == 2040
    rng = np.random.default_rng(31)
    at, pieces = 3, []
    for _ in range(n):
        bits = int(rng.choice([0, 1, int(rng.integers(0, 40)), int(rng.integers(0, 300))]))
        pieces.append((at, bits, int(rng.integers(0, 4096 - 40))))
        at += bits + int(rng.choice([0, 0, int(rng.integers(0, 9))]))
    pieces[-1] = (pieces[-1][0], 77, 11)  # the list's last end matters: a piece that is not empty
    tp._check(_OnDevice(probe), pieces)
    tp._check(_OnDevice(probe), pieces, lo=pieces[n // 2][0] // 8 + 1)


def test_the_copy_kernel_at_every_alignment_of_the_range(probe):
    """b_lo and b_hi in all 16 combinations mod 4: hydk_store_word's byte-wise first and last words"""
    pieces = tp._chain([100, 0, 37, 200, 333], start=3 * 8 + 3)
    dev = _OnDevice(probe)
    seen = set()
    for lo in range(4, 8):
        for hi in range(60, 64):
            tp._check(dev, pieces, lo=lo, nbytes=hi - lo)
            seen.add((lo % 4, hi % 4))
    assert len(seen) == 16
    for lo in range(4, 8):  # ... and ranges that lie inside one word
        for hi in range(lo + 1, 9):
            tp._check(dev, pieces, lo=lo, nbytes=hi - lo)


def test_the_copy_kernel_leaves_the_buffer_alone_on_an_error_word_and_on_an_empty_range(probe):
    pieces = tp._chain([100, 0, 37, 200], start=5 * 8 + 3)
    for fill in (0xA5, 0x00):
        for err in (1, 0x40, 0x80000000):
            got = tp._compose(_OnDevice(probe, err), pieces, 5, 44, fill)
            assert (got == fill).all(), (err, np.flatnonzero(got != fill)[:8])
        for lo in (0, 5, 8):
            got = tp._compose(_OnDevice(probe), pieces, lo, 0, fill)
            assert (got == fill).all(), (lo, np.flatnonzero(got != fill)[:8])
    tp._check(_OnDevice(probe), pieces, lo=5, nbytes=44)  # ... and the same range without either


def test_the_hook_refuses_lists_that_leave_its_buffers(probe):
    """nothing is launched for a piece that reads past the source or a range that ends past the output"""
    out = np.full(64, 0xA5, np.uint8)
    one = np.array([0], np.uint64)

    def call(nbits, off, lo, nbytes, out_bytes=64):
        n, o = np.array([nbits], np.uint64), np.array([off], np.uint64)
        return probe.hydt_pieces_copy_device(one.ctypes.data, n.ctypes.data, o.ctypes.data, 1, tp.SRC.ctypes.data, tp.SRC.nbytes, lo, nbytes, 0,
                                             out.ctypes.data, out_bytes)

    assert call(8 * 4096 + 1, 0, 0, 16) == -14
    assert call(16, 4095, 0, 16) == -14
    assert call(16, 0, 60, 8) == -14
    assert call(16, 0, 0, 16, out_bytes=62) == -14
    assert (out == 0xA5).all()
    assert call(16, 0, 0, 16) == 0 and bytes(out[:2]) == bytes(tp.SRC[:2]) and not out[2:16].any() and (out[16:] == 0xA5).all()
