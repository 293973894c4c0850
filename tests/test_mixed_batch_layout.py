"""The mixed-size batch API's surface without a GPU: the shipped library exports it (and not its test hook), the Python
binding agrees with the header's prototypes, and creation refuses what it must before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import has_gpu
from hydrium_amd import build as hbuild, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["hydamd_mixed_create", "hydamd_mixed_destroy", "hydamd_mixed_error", "hydamd_encode_mixed", "hydamd_mixed_result",
           "hydamd_mixed_offsets", "hydamd_mixed_device", "hydamd_mixed_offsets_device", "hydamd_mixed_read",
           "hydamd_mixed_overflow_reruns"]
API_ERROR, INTERNAL_ERROR = -14, -15


def _exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_shipped_library_exports_the_mixed_api_and_not_its_hook():
    shipped = _exported(hbuild.build())
    assert not [s for s in SYMBOLS if s not in shipped]
    assert not [s for s in shipped if s.startswith("hydt_") or s.startswith("hydk_")]
    assert "hydt_mixed_from_streams" in _exported(hbuild.PROBE_PATH)  # the probe flavour is where the hook lives


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


def test_the_descriptor_is_the_header_s_struct():
    """field for field: three pointers, two strides in samples, width and height — 56 bytes on an LP64 machine"""
    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    m = re.search(r"typedef struct HydAmdImageDesc \{(.*?)\} HydAmdImageDesc;", text, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip(" *").split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == [f[0] for f in device.HydAmdImageDesc._fields_] == ["src", "row_stride", "pixel_stride", "width", "height"]
    assert C.sizeof(device.HydAmdImageDesc) == 3 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_ssize_t) + 2 * C.sizeof(C.c_size_t)


@pytest.mark.parametrize("max_frames", [-1, 256])
def test_what_creation_refuses_needs_no_device(max_frames):
    d = device.dll()
    st = C.c_int(0)
    assert not d.hydamd_mixed_create(0, max_frames, 0, C.byref(st))
    assert st.value == API_ERROR and b"max_frames" in d.hydamd_mixed_error(None)
    with pytest.raises(device.DeviceError, match="max_frames") as e:
        device.MixedBatch(max_frames)
    assert e.value.code == API_ERROR


@pytest.mark.parametrize("max_frames", [0, 1, 255])
def test_creation_reports_a_missing_device(max_frames):
    # no device at all on a CPU machine; an index no machine has anywhere else
    dev = 0 if not has_gpu() else 1 << 20
    d = device.dll()
    st = C.c_int(0)
    assert not d.hydamd_mixed_create(dev, max_frames, 0, C.byref(st))
    assert st.value == INTERNAL_ERROR and b"no usable HIP device" in d.hydamd_mixed_error(None)
    with pytest.raises(device.DeviceError, match="no usable HIP device"):
        device.MixedBatch(max_frames, device=dev)
