"""The frame-batch API's surface without a GPU: the shipped library exports it, the Python binding agrees with the
header's prototypes, and creation refuses what it must before any device is touched.  And the batch's own plan with the
batched frame layout (csrc/hip/hydk_tiles.h compiled for the host: what k_batch_prepare_one runs) on the content corpus,
every file held to what frame.c writes for that picture alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import content_corpus as cc
import glue
from conftest import has_gpu
from hydrium_amd import api, build as hbuild, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["hydamd_batch_create", "hydamd_batch_destroy", "hydamd_batch_error", "hydamd_encode_batch", "hydamd_batch_result",
           "hydamd_batch_offsets", "hydamd_batch_device", "hydamd_batch_offsets_device", "hydamd_batch_read",
           "hydamd_batch_overflow_reruns"]
API_ERROR = -14


def test_the_shipped_library_exports_the_batch_api():
    lib = hbuild.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in SYMBOLS + ["hydamd_export_batch_owned"] if s not in exported]
    assert not [s for s in exported if s.startswith("hydk_")]  # the planners and the device half stay inside the library


_CTYPE = {"int": C.c_int, "size_t": C.c_size_t, "ptrdiff_t": C.c_ssize_t, "unsigned": C.c_uint}


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    m = re.search(r"HYDAMD_EXPORT\s+([^;]*?)\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return " ".join(m.group(1).split()), [" ".join(a.split()) for a in m.group(2).split(",")]


def _kind(decl):
    """what a C declarator is to ctypes: 'ptr' for any pointer or array, else the scalar type"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w not in ("const",)]
    return _CTYPE[words[0]]


def _ctypes_kind(t):
    if t is None:
        return None
    return "ptr" if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents") or hasattr(t, "_type_") and isinstance(t._type_, type) else t


@pytest.mark.parametrize("name", SYMBOLS)
def test_binding_and_header_agree(name):
    d = device.dll()
    ret, args = _prototype(name)
    fn = getattr(d, name)
    assert len(fn.argtypes) == len(args), (name, args)
    for decl, t in zip(args, fn.argtypes):
        assert _ctypes_kind(t) == _kind(decl), (name, decl, t)
    if ret.startswith("void") and "*" not in ret:
        assert fn.restype is None
    else:
        assert _ctypes_kind(fn.restype) == _kind(ret + " x"), (name, ret, fn.restype)


def _refused(md, max_frames):
    d = device.dll()
    st = C.c_int(0)
    h = d.hydamd_batch_create(0, C.byref(md) if md is not None else None, max_frames, None, 0, C.byref(st))
    assert not h
    return st.value, d.hydamd_batch_error(None)


def test_what_creation_refuses_needs_no_device():
    for sx, sy in [(0, 0), (-1, 0), (1, -1), (3, 3)]:  # a batch holds one-frame images
        st, msg = _refused(api.HYDImageMetadata(2100, 300, 0, sx, sy), 2)
        assert st == API_ERROR and b"tile_size_shift" in msg
    st, msg = _refused(api.HYDImageMetadata(2100, 300, 0, -1, -1), 0)
    assert st == API_ERROR and b"max_frames" in msg
    st, msg = _refused(api.HYDImageMetadata(2100, 300, 0, -1, -1), -3)
    assert st == API_ERROR and b"max_frames" in msg
    st, msg = _refused(api.HYDImageMetadata(2100, 300, 0, -1, -1), 128)  # 2 LF groups x 128 frames = 256 slots
    assert st == API_ERROR and b"255" in msg
    st, msg = _refused(api.HYDImageMetadata(700, 500, 0, -1, -1), 256)   # one LF group x 256 frames
    assert st == API_ERROR and b"255" in msg
    st, msg = _refused(api.HYDImageMetadata(262144, 8, 0, -1, -1), 1)    # 128 LF groups: no frame holds them
    assert st == API_ERROR and b"unsupported number of LF groups" in msg
    st, msg = _refused(api.HYDImageMetadata(2048 * 256, 8, 0, -1, -1), 1)  # 256
    assert st == API_ERROR and b"unsupported number of LF groups" in msg
    st, msg = _refused(None, 2)
    assert st == API_ERROR and b"null" in msg


def test_the_largest_admissible_batches_are_not_refused_for_their_size():
    """F x n = 255 passes the checks that need no device, and then fails for want of one (an index no machine has)."""
    for w, h, f in [(700, 500, 255), (2100, 300, 127), (2048 * 5, 2048 * 3, 17)]:
        with pytest.raises(device.DeviceError, match="no usable HIP device"):
            device.FrameBatch(w, h, f, device=0 if not has_gpu() else 1 << 20)


def test_creation_reports_a_missing_device():
    # no device at all on a CPU machine; an index no machine has anywhere else
    with pytest.raises(device.DeviceError, match="no usable HIP device"):
        device.FrameBatch(2100, 300, 2, device=0 if not has_gpu() else 1 << 20)


# ---- the batch plan and layout on the content corpus (tests/content_corpus.py) -------------------------------------------
MAXC, ALPHA, GPL = 9, 128, 64


@pytest.fixture(scope="module")
def hooks():
    hbuild.build()
    d = C.CDLL(hbuild.HOSTTEST_PATH)
    d.hydt_batch_from_streams.restype = C.c_int
    d.hydt_batch_from_streams.argtypes = [C.POINTER(api.HYDImageMetadata), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
    d.hydt_free.argtypes = [C.c_void_p]
    return d


def _batch_files(d, w, h, stages):
    """(bytes of all files, offsets table) of one same-shape batch through hydt_batch_from_streams; stages: cc.stage's"""
    n = len(stages)
    freq = np.zeros((n, MAXC, ALPHA), np.uint32)
    alpha = np.zeros((n, MAXC), np.uint32)
    bits = np.zeros((n, GPL), np.uint32)
    mxs = np.zeros(n, np.uint32)
    keep, arr = [], (glue.LfStream * n)()
    for s, (r, mx, lf, _) in enumerate(stages):
        ncl = r.cluster_to - r.cluster_from
        freq[s, :ncl] = r.freqs[r.cluster_from:r.cluster_to]
        alpha[s, :ncl] = r.alphabet_size[r.cluster_from:r.cluster_to]
        bits[s, :r.num_groups] = r.group_bits
        mxs[s] = mx
        _, lengths, alphabet, pairs, packed, nbits = lf
        lengths = np.ascontiguousarray(lengths, np.uint8)
        packed = np.ascontiguousarray(packed, np.uint8)
        keep.append((lengths, packed))
        arr[s] = glue.LfStream(lengths.ctypes.data, alphabet, pairs, packed.ctypes.data if nbits else None, nbits)
    payload = b"".join(r.stream for r, _, _, _ in stages)
    md = api.HYDImageMetadata(w, h, 0, -1, -1)
    offs = np.zeros(n + 1, np.uint64)
    out, out_len, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p(None)
    ret = d.hydt_batch_from_streams(C.byref(md), n, arr, freq.ctypes.data, alpha.ctypes.data, bits.ctypes.data, mxs.ctypes.data, payload,
                                    len(payload), offs.ctypes.data, C.byref(out), C.byref(out_len), C.byref(err))
    assert ret == 0, err.value
    data = bytes((C.c_uint8 * out_len.value).from_address(out.value))
    d.hydt_free(out)
    return data, [int(o) for o in offs]


ONE_GROUP_BATCHES = [b for b in cc.BATCH if b[0][1] <= cc.LF_GROUP]


@pytest.mark.parametrize("pictures", ONE_GROUP_BATCHES, ids=[f"{b[0][1]}x{b[0][2]}-{b[0][3]}b" for b in ONE_GROUP_BATCHES])
def test_the_content_corpus_in_same_shape_batches(hooks, pictures):
    """black, noise, primaries and photo in one batch (files of 203 bytes and of 250 KB behind one another); a float frame
    of log_alphabet_size 5 between two of 7 — a running alphabet that leaked from frame to frame would change its header;
    the empty LF stream of black 8 x 8 between two frames of noise.  Then the same batch rotated by one."""
    _, w, h, _, _ = pictures[0]
    assert all(p[1:3] == (w, h) for p in pictures)
    stages = [cc.stage(*p) for p in pictures]
    for order in (stages, stages[1:] + stages[:1]):
        wants = [want for _, _, _, want in order]
        got, offs = _batch_files(hooks, w, h, order)
        assert offs == [sum(map(len, wants[:k])) for k in range(len(wants) + 1)]
        for k, want in enumerate(wants):
            assert got[offs[k]:offs[k + 1]] == want, (k, pictures)
        assert got == b"".join(wants)
    print(pictures[0][1:4], "files of", [len(s[3]) for s in stages], "bytes; log_alphabet_size", [s[0].log_alphabet_size for s in stages])
    if pictures[0][3] == 32:
        assert [s[0].log_alphabet_size for s in stages] == [7, 5, 7]


def test_the_two_lf_group_batch_pictures_are_what_the_reference_makes_of_them(ref_lib):
    """Shapes of several LF groups go through csrc/hip/hydk_asm_writers.h, which runs on the GPU only
    (tests/test_gpu_builder_content.py).  Here: frame.c — what the host assembly of that test is — on the same pictures,
    from the oracle's stages, against the compiled reference; and the black LF group really is nothing but sections of a few bytes."""
    from oracle import binding as orc

    for p in [p for b in cc.BATCH if b[0][1] > cc.LF_GROUP for p in b] + cc.ASSEMBLER:
        img = cc.picture(*p)
        assert glue.encode_with_oracle_stages(img, coded_lf=True) == api.encode_image(ref_lib, img, out_buf_size=1 << 22), p
        black = 0 if p[0] == "black_noise" else 1
        r, _ = orc.encode_lf_group(img, black, 0)
        sizes = cc.hf_section_bytes(r)  # one size for every section of the black LF group, a few bytes
        assert len(set(sizes)) == 1 and sizes[0] < 8, p
