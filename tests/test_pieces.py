"""The shared piece composer (csrc/hip/hydk_pieces.h: what k_pieces_copy runs for both device-side assemblers) compiled
for the host and held to a bit-by-bit model on crafted piece lists.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from hydrium_amd import build as hbuild


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    d = C.CDLL(hbuild.HOSTTEST_PATH)
    d.hydt_compose_pieces.restype = C.c_int
    d.hydt_compose_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    return d


SRC = np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8)
SRC_BITS = np.unpackbits(SRC, bitorder="little")


def _out_size(lo, nbytes):
    """bytes of the buffer a range is composed into: whole words, and two more behind them that must stay as they were"""
    return (lo + nbytes + 3) // 4 * 4 + 8


def _model(pieces, lo, nbytes, fill):
    """pieces: (dst_bit, nbits, source byte offset).  The whole buffer: `fill` outside [lo, lo + nbytes), inside it the
    pieces' bits, LSB first, and zero where no piece lies."""
    size = _out_size(lo, nbytes)
    bits = np.zeros(max([size * 8] + [d + n for d, n, _ in pieces]) + 7 & ~7, np.uint8)
    for dst, n, off in pieces:
        bits[dst:dst + n] = SRC_BITS[off * 8:off * 8 + n]
    want = np.full(size, fill, np.uint8)
    want[lo:lo + nbytes] = np.packbits(bits, bitorder="little")[lo:lo + nbytes]
    return want


def _compose(lib, pieces, lo, nbytes, fill):
    a = np.array(pieces, np.uint64).reshape(-1, 3)
    dst, n, off = (np.ascontiguousarray(a[:, i]) for i in range(3))
    out = np.full(_out_size(lo, nbytes), fill, np.uint8)
    assert out.ctypes.data % 4 == 0
    assert lib.hydt_compose_pieces(dst.ctypes.data, n.ctypes.data, off.ctypes.data, len(a), SRC.ctypes.data, lo, nbytes, out.ctypes.data) == 0
    return out


def _check(lib, pieces, lo=None, nbytes=None, fill=0xA5):
    end = max((d + n for d, n, _ in pieces), default=0)
    lo = 0 if lo is None else lo
    nbytes = (end + 7) // 8 - lo if nbytes is None else nbytes
    got, want = _compose(lib, pieces, lo, nbytes, fill), _model(pieces, lo, nbytes, fill)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def _chain(lengths, start=0, off=0):
    """pieces back to back from bit `start`, sources one after another (each at the next byte)"""
    out, at = [], start
    for n in lengths:
        out.append((at, n, off))
        at += n
        off += (n + 7) // 8
    return out


@pytest.mark.parametrize("end", [31, 32, 33])
def test_piece_ends_around_a_word_boundary(lib, end):
    _check(lib, _chain([64 + end, 200]))
    _check(lib, [(0, end, 5), (end, 150, 40)])


def test_three_pieces_inside_one_word(lib):
    _check(lib, _chain([70, 5, 9, 11, 130], start=0))
    _check(lib, [(32, 3, 0), (40, 7, 9), (50, 13, 22), (64, 100, 31)])


def test_empty_pieces(lib):
    _check(lib, _chain([0, 100, 0, 77, 0]))
    _check(lib, _chain([0, 0, 100, 0, 0, 77, 0, 0]))
    _check(lib, [(0, 0, 0), (0, 0, 1)], lo=0, nbytes=8)  # nothing but empty pieces: zeros
    _check(lib, [], lo=0, nbytes=8)


@pytest.mark.parametrize("off", [0, 1, 2, 3, 4093])
def test_source_alignment(lib, off):
    _check(lib, [(0, 24 if off == 4093 else 300, off)])
    _check(lib, [(13, 24 if off == 4093 else 300, off)])


def test_one_bit(lib):
    for dst in (0, 31, 32, 63, 200):
        one = int(np.flatnonzero(SRC & 1)[0])  # a source byte whose first bit is set
        _check(lib, [(dst, 1, one)], lo=0, nbytes=32)


def test_gap_reads_as_zero(lib):
    _check(lib, [(0, 61, 0), (64, 93, 16), (160, 3, 64), (256, 100, 80)])  # byte padding, and whole words no piece covers


def test_range_edges_leave_the_neighbours_alone(lib):
    pieces = _chain([100, 0, 37, 200], start=5 * 8 + 3)
    for lo, nbytes in ((5, 44), (6, 41), (7, 1), (5, 2), (8, 40), (5, 0)):
        _check(lib, pieces, lo=lo, nbytes=nbytes)


def test_random_lists(lib):
    rng = np.random.default_rng(11)
    for _ in range(300):
        at, pieces = int(rng.integers(0, 70)), []
        for _ in range(int(rng.integers(0, 25))):
            n = int(rng.choice([0, 1, int(rng.integers(0, 40)), int(rng.integers(0, 300))]))
            pieces.append((at, n, int(rng.integers(0, 4096 - 40))))
            at += n + int(rng.choice([0, 0, int(rng.integers(0, 9)), int(rng.integers(0, 80))]))
        lo = int(rng.integers(0, at // 8 + 1))
        _check(lib, pieces, lo=lo, nbytes=int(rng.integers(0, (at + 7) // 8 - lo + 3)))
