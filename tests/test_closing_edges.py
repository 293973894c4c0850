"""CPU-only: the edge-word helper of csrc/hip/hydk_edges.h, compiled with the host compiler.

k_rans_emit's self-placing mode writes a section's first and last 32-bit word as byte stores of exactly the section's own
bytes, because nothing clears those words beforehand and up to four sections may meet in one of them.  Here the same text
writes sections of every (offset mod 4, length 1..12) into a buffer of 0xA5 bytes, word by word as the kernel does (every
word that holds a byte of the section, with the foreign bytes of the value set to garbage), and into a zeroed buffer as
neighbours in both orders: the section's bytes are right and no byte outside it changes."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "hydrium_amd", "csrc", "hip")

DRIVER = r"""
#include <stdint.h>
#include "hydk_edges.h"
/* one section, the way the emit kernel stores it: each word that holds one of its bytes once, whole words inside, the edge
 * words through the helper; `junk` fills the bytes of an edge word's value that are not the section's */
void write_section(uint8_t *buf, uint64_t lo, uint64_t len, const uint8_t *bytes, uint32_t junk, int downwards) {
    if (!len)
        return;
    const uint64_t hi = lo + len, w0 = lo >> 2, w1 = (hi - 1) >> 2;
    for (uint64_t k = 0; k <= w1 - w0; k++) {
        const uint64_t w = downwards ? w1 - k : w0 + k;
        uint32_t v = junk;
        for (uint32_t b = 0; b < 4; b++) {
            const uint64_t at = w * 4 + b;
            if (at >= lo && at < hi)
                v = (v & ~(0xFFu << (8 * b))) | ((uint32_t)bytes[at - lo] << (8 * b));
        }
        hydk_store_edge_word(buf, w, v, lo, hi);
    }
}
uint32_t byte_mask(uint64_t word, uint64_t lo, uint64_t hi) { return hydk_edge_byte_mask(word, lo, hi); }
"""


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    d = tmp_path_factory.mktemp("edges")
    src, lib = d / "edges.c", d / "libedges.so"
    src.write_text(DRIVER)
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-O1", "-Wall", "-Werror", "-fno-strict-aliasing", "-shared", "-fPIC",
                        f"-I{HEADER_DIR}", str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dll = C.CDLL(str(lib))
    dll.write_section.restype = None
    dll.write_section.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int]
    dll.byte_mask.restype = C.c_uint32
    dll.byte_mask.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    return dll


def _section(seed, n):
    return (np.random.default_rng(seed).integers(1, 256, n)).astype(np.uint8)  # never 0: a dropped byte shows in a zeroed buffer


def _write(dll, buf, lo, data, junk=0xFFFFFFFF, downwards=False):
    dll.write_section(buf.ctypes.data, lo, len(data), data.ctypes.data, junk, int(downwards))


def test_the_mask_names_the_words_own_bytes(edges):
    for word, lo, n in itertools.product(range(5), range(12), range(0, 13)):
        want = sum(1 << b for b in range(4) if lo <= word * 4 + b < lo + n)
        assert edges.byte_mask(word, lo, lo + n) == want, (word, lo, n)
    big = 1 << 33  # payload offsets are 64-bit
    assert edges.byte_mask(big // 4, big + 1, big + 3) == 0b0110


@pytest.mark.parametrize("downwards", [False, True])
def test_every_offset_and_length_alone(edges, downwards):
    for off, n in itertools.product(range(4), range(1, 13)):
        for base in (0, 8):
            lo = base + off
            data = _section(off * 16 + n, n)
            buf = np.full(32, 0xA5, np.uint8)
            _write(edges, buf, lo, data, junk=0x5A5A5A5A ^ n, downwards=downwards)
            assert bytes(buf[lo:lo + n]) == bytes(data), (off, n, base)
            assert (buf[:lo] == 0xA5).all() and (buf[lo + n:] == 0xA5).all(), f"offset {lo}, length {n}: a foreign byte changed"


def test_neighbours_in_both_orders_into_a_zeroed_buffer(edges):
    """Two and three sections back to back (so that up to four meet in one word), written in every order."""
    checked = 0
    for off, lens in itertools.product(range(4), itertools.product(range(1, 13), range(1, 4), range(1, 13))):
        los = [8 + off, 8 + off + lens[0], 8 + off + lens[0] + lens[1]]
        datas = [_section(100 * i + n, n) for i, n in enumerate(lens)]
        want = np.zeros(48, np.uint8)
        for lo, d in zip(los, datas):
            want[lo:lo + len(d)] = d
        for order in itertools.permutations(range(3)):
            buf = np.zeros(48, np.uint8)
            for i in order:
                _write(edges, buf, los[i], datas[i], junk=0xFFFFFFFF, downwards=bool(i & 1))
            assert bytes(buf) == bytes(want), (off, lens, order)
            checked += 1
    assert checked == 4 * 12 * 3 * 12 * 6


def test_three_sections_inside_one_word(edges):
    """One-byte sections (a group without symbols is only its preset bits) at bytes 1, 2, 3 of a word and 0 of the next."""
    datas = [_section(7 + i, 1) for i in range(4)]
    for order in itertools.permutations(range(4)):
        buf = np.zeros(16, np.uint8)
        for i in order:
            _write(edges, buf, 5 + i, datas[i])
        assert bytes(buf[5:9]) == b"".join(bytes(d) for d in datas)
        assert not buf[:5].any() and not buf[9:].any()
