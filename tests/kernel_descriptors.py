"""What the default build's kernels ask of a compute unit, read from the code object hipcc cross-compiles from kernels.hip
(a plain helper: no tests here).  The compile takes some twenty seconds, so it is made once per process and shared by every
module that asserts on a kernel's LDS, registers or scratch."""
import os
import re
import subprocess
import tempfile

import pytest

from hydrium_amd import build as hbuild

FIELDS = ("group_segment_fixed_size", "next_free_vgpr", "private_segment_fixed_size")
_cache = {}


def parse(text):
    """{mangled name: {field: value}} of every kernel descriptor in an assembly listing"""
    return {m.group(1): {k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", m.group(2)).group(1)) for k in FIELDS}
            for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}


def kernel_descriptors():
    """of every kernel of kernels.hip in the default build (build.HIP_FLAGS); skips the calling test where there is no hipcc"""
    if "kernels" not in _cache:
        if not os.path.exists(hbuild.HIPCC):
            pytest.skip("no hipcc")
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "k.s")
            subprocess.run([hbuild.HIPCC] + hbuild.HIP_FLAGS + ["--cuda-device-only", "-S", "-o", out, os.path.join(hbuild.CSRC, "hip", "kernels.hip")],
                           check=True, capture_output=True)
            with open(out) as fh:
                _cache["kernels"] = parse(fh.read())
    return _cache["kernels"]
