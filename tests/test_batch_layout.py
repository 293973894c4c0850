"""The frame-batch API's surface without a GPU: the shipped library exports it, the Python binding agrees with the
header's prototypes, and creation refuses what it must before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

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
