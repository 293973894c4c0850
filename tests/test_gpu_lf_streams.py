"""GPU: the LF-group coder's kernels on the crafted residual streams of tests/lf_streams.py, against the serial host coder.

Pictures put run heads where their content happens to; these streams put them at the positions the kernels decide at
(window edges, the look-ahead's end, the backward scan's steps, chunk ends, plane boundaries inside a thread, the longest
bit string at every awkward bit of a word).  The LF ints reach the device through the probe flavour's hook
hydt_write_lf_ints, the mirror of hydamd_read_dc: an all-zero picture of the stream's shape is transformed, its LF planes
are overwritten, and the coder runs on one of three routes, each of which launches the kernels differently:

  early   hydamd_run_lf_coder in the main stream in front of the entropy stage (hyd_send_tile's schedule);
  side    the whole coder forked onto the side stream (the device API's default);
  riding  tokens in front of the chain kernel, the code construction inside its launch, offsets and pack behind it
          (what the batch, tiled and mixed objects run).

Everything is bit-exact; the assertion that counts is that the device's stream, spliced by the host, equals the section
the serial host coder writes from the same LF ints.  The contexts come from the probe library; the module global the rest
of the process uses is never rebound."""
import ctypes as C
import functools

import numpy as np
import pytest

from hydrium_amd import build as hbuild, device as dev
from tests import lf_model, lf_streams as ls

pytestmark = pytest.mark.gpu

ROUTES = ("riding", "early", "side")


class Probe:
    """the HYD_TEST_HOOKS flavour, bound beside the shipped library"""

    def __init__(self):
        import torch

        shipped = dev.dll()
        self.d = dev.dll(hbuild.PROBE_PATH)
        assert dev.dll() is shipped and self.d is not shipped
        self.d.hydt_write_lf_ints.restype = C.c_int
        self.d.hydt_write_lf_ints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t]
        self.zeros = torch.zeros(2048 * 2048 * 3, dtype=torch.uint8, device="cuda")  # a black picture of any shape

    def open(self, slots: int, route: str) -> "dev.DeviceContext":
        saved = dev._dll
        dev._dll = self.d
        try:
            c = dev.DeviceContext(0, slots)
        finally:
            dev._dll = saved
        assert c.d is self.d
        if route == "riding":
            c.set_lf_coder(2)
            c.set_rans_waves(5)
        else:
            assert c.d.hydamd_lf_coder(c.h) == 1
        return c

    def write_lf_ints(self, c, slot: int, dc: np.ndarray):
        dc = np.ascontiguousarray(dc, np.int32)
        c._ck(self.d.hydt_write_lf_ints(c.h, slot, dc.ctypes.data, dc.shape[2], dc.shape[1]))


@pytest.fixture(scope="module")
def probe():
    saved = dev.dll()
    yield Probe()
    assert dev._dll is saved, "the process is back on the shipped library"


@pytest.fixture(scope="module")
def contexts(probe):
    """one context per route for all single-slot cases, in the corpus' order: each also sees what the case before left"""
    ctxs = {r: probe.open(1, r) for r in ROUTES}
    yield ctxs
    for c in ctxs.values():
        c.close()


@functools.lru_cache(maxsize=None)
def reference(case):
    """(model's lengths, alphabet, run pairs, bits, bit count; the host coder's section) — computed once per case"""
    dc = case.lf_ints()
    _, lengths, alphabet, pairs, bits, nbits = lf_model.model(dc)
    return lengths, alphabet, pairs, bits, nbits, lf_model.host_lf_group(dc)


def run_frame(probe, c, route, cases):
    """one frame of len(cases) LF groups on `route`; -> per slot (lengths, alphabet, pairs, nbits, bits), records, payload"""
    n = len(cases)
    p = probe.zeros.data_ptr()
    c.begin_frame(n)
    for s, case in enumerate(cases):
        w, h = 8 * case.vbw, 8 * case.vbh
        c.encode_lf_group(s, [p, p + 1, p + 2], 3 * w, 3, 0, w, h, s)
        c.submit_lf_group(s)
    for s, case in enumerate(cases):
        probe.write_lf_ints(c, s, case.lf_ints())
    if route == "early":
        c.run_lf_coder(n, True)
        c.finish_frame(n)
        c.sync_lf()
    else:
        c.finish_frame(n)
        c.sync()
    got = []
    for s, case in enumerate(cases):
        lengths, alphabet, pairs, nbits = c.read_lf_stream(s)
        got.append((lengths, alphabet, pairs, nbits, c.read_lf_bits(s, nbits)))
    info, blob = c.read_lf_streams(n), c.read_lf_payload().copy()
    if route == "early":
        c.sync()
    for s, case in enumerate(cases):  # the coder ran on the planes written
        np.testing.assert_array_equal(c.read_dc(s, case.vbw, case.vbh), case.lf_ints())
    return got, info, blob


def first_difference(case, bits, m_bits, nbits):
    """where the device's bits leave the model's: bit, stream position, window"""
    a = np.unpackbits(bits, bitorder="little")[:nbits]
    b = np.unpackbits(m_bits, bitorder="little")[:nbits]
    bad = np.nonzero(a != b)[0]
    if not len(bad):
        return None
    i = ls.Info(case.stream())
    pos = int(np.searchsorted(i.off + i.ln, bad[0], side="right"))
    return f"first differing bit {int(bad[0])}: stream position {pos}, window {pos // ls.WINDOW}"


def check_slot(case, got):
    lengths, alphabet, pairs, nbits, bits = got
    m_len, m_alpha, m_pairs, m_bits, m_nbits, section = reference(case)
    assert (alphabet, pairs, nbits) == (m_alpha, m_pairs, m_nbits)
    np.testing.assert_array_equal(lengths, m_len)
    # bits past bit_count in the last byte are unspecified on the device side
    dev_bits, mod_bits = bits.copy(), m_bits[:(nbits + 7) // 8].copy()
    if nbits % 8:
        mask = (1 << (nbits % 8)) - 1
        dev_bits[-1] &= mask
        mod_bits[-1] &= mask
    assert np.array_equal(dev_bits, mod_bits), first_difference(case, dev_bits, mod_bits, nbits)
    # the one that counts: the serial host coder shares nothing with the kernels
    assert lf_model.coded_lf_group(case.vbw, case.vbh, lengths, alphabet, pairs, bits, nbits) == section


def check_payload(c, cases, got, info, blob):
    end = 0
    for s, (lengths, alphabet, pairs, nbits, bits) in enumerate(got):
        assert (int(info["bit_count"][s]), int(info["alphabet"][s]), int(info["run_pairs"][s])) == (nbits, alphabet, pairs)
        assert int(info["error"][s]) == 0
        np.testing.assert_array_equal(info["lengths"][s], lengths)
        off = int(info["offset"][s])
        assert off == end and off % 4 == 0
        np.testing.assert_array_equal(blob[off:off + (nbits + 7) // 8], bits)
        end = off + (nbits + 31) // 32 * 4
    assert end == len(blob)
    np.testing.assert_array_equal(c.lf_payload_tensor().cpu().numpy(), blob)


def _single():
    for route in ROUTES:
        for case in ls.CASES:
            if route != "side" or case.family in ls.FAMILIES_ON_SIDE:
                yield pytest.param(route, case, id=f"{route}-{case.name}")


@pytest.mark.parametrize("route,case", list(_single()))
def test_crafted_stream(probe, contexts, route, case):
    c = contexts[route]
    got, info, blob = run_frame(probe, c, route, [case])
    check_slot(case, got[0])
    check_payload(c, [case], got, info, blob)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("frame", ls.FRAMES, ids=[f.name for f in ls.FRAMES])
def test_several_slots_in_one_frame(probe, frame, route):
    c = probe.open(len(frame.slots), route)
    try:
        got, info, blob = run_frame(probe, c, route, frame.slots)
        for case, g in zip(frame.slots, got):
            check_slot(case, g)
        check_payload(c, frame.slots, got, info, blob)
        if frame.name == "g-zero-bits-in-the-middle":
            assert got[1][3] == 0 and int(info["offset"][1]) == int(info["offset"][2])
        if frame.name == "g-bits-multiple-of-32":
            assert got[0][3] % 32 == 0 and int(info["offset"][1]) * 8 == got[0][3]
    finally:
        c.close()


@pytest.mark.parametrize("route", ROUTES)
def test_a_context_used_twice(probe, route):
    """the longest stream, then the shortest in the same context and slot: nothing the first frame left in records, window
    histograms, offsets or bit words shows in the second"""
    c = probe.open(1, route)
    try:
        for case in ls.TWICE:
            got, info, blob = run_frame(probe, c, route, [case])
            check_slot(case, got[0])
            check_payload(c, [case], got, info, blob)
    finally:
        c.close()


def test_the_hook_checks_its_arguments(probe):
    c = probe.open(1, "side")
    try:
        dc = np.zeros((3, 1, 1), np.int32)
        assert probe.d.hydt_write_lf_ints(c.h, 1, dc.ctypes.data, 1, 1) != 0       # no such slot
        assert probe.d.hydt_write_lf_ints(c.h, 0, dc.ctypes.data, 257, 1) != 0     # larger than an LF group
        assert probe.d.hydt_write_lf_ints(c.h, 0, None, 1, 1) != 0
    finally:
        c.close()


def test_the_process_stays_on_the_shipped_library(probe):
    from hydrium_amd import api

    assert dev.dll() is not probe.d and dev.dll()._name == api.DEFAULT_LIB
    with dev.DeviceContext(0, 1) as c:
        assert c.d is dev.dll()
