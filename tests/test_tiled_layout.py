"""The tiled device API's surface without a GPU: the shipped library exports it, the Python binding agrees with the
header's prototypes, and creation fails cleanly where there is no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import has_gpu
from hydrium_amd import api, build as hbuild, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["hydamd_tiled_create", "hydamd_tiled_destroy", "hydamd_tiled_error", "hydamd_encode_image_tiled",
           "hydamd_tiled_result", "hydamd_tiled_read", "hydamd_tiled_device"]


def test_the_shipped_library_exports_the_tiled_api():
    lib = hbuild.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in SYMBOLS + ["hydamd_export_batch_owned"] if s not in exported]
    assert "hydt_tiles_from_streams" not in exported  # the test hook lives in the probe flavour only


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


def test_rejected_metadata_needs_no_device():
    d = device.dll()
    st = C.c_int(0)
    for sx, sy in [(-1, 0), (0, -1), (4, 0)]:
        md = api.HYDImageMetadata(300, 280, 0, sx, sy)
        assert not d.hydamd_tiled_create(0, C.byref(md), 0, C.byref(st))
        assert st.value == -14 and b"tile_size_shift" in d.hydamd_tiled_error(None)
    md = api.HYDImageMetadata(300, 280, 0, 0, 0)
    assert not d.hydamd_tiled_create(0, C.byref(md), 256, C.byref(st)) and st.value == -14
    assert not d.hydamd_tiled_create(0, None, 0, C.byref(st)) and st.value == -14


def test_creation_reports_a_missing_device():
    # no device at all on a CPU machine; an index no machine has anywhere else
    with pytest.raises(device.DeviceError, match="no usable HIP device"):
        device.TiledImage(300, 280, 0, 0, device=0 if not has_gpu() else 1 << 20)
