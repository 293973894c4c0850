"""The programs of tests/c/*_formats.cc as plain C++ under address and UB sanitizers — stand-alone executables, nothing of them
is loaded into Python — and what tests/c/sample_formats.cc prints of every number -8 ... 4100, made once per session."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import format_model as fm
from hydrium_amd import build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def sanitized_program(stem):
    """tests/c/<stem>.cc with g++ under address and UB sanitizers, no HIP header, no warning: run(mode, *arguments, data=None) -> its output bytes"""
    d = tempfile.mkdtemp(prefix=stem + "_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, stem)
    source = os.path.join(ROOT, "tests", "c", stem + ".cc")
    assert "hip_runtime" not in open(source).read()
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", hbuild.CSRC, source, "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert made.returncode == 0 and not made.stderr, made.stderr  # no warning either

    def run(mode, *args, data=None):
        """the mode's output file, whole; exit status 0 and an empty stderr"""
        out = os.path.join(d, mode + ".out")
        if data is not None:
            with open(os.path.join(d, mode + ".in"), "wb") as f:
                f.write(data)
            args = (os.path.join(d, mode + ".in"),)
        ran = subprocess.run([exe, mode, out, *map(str, args)], capture_output=True, text=True, timeout=300)
        assert (ran.returncode, ran.stderr) == (0, ""), (mode, ran.returncode, ran.stderr[-4000:])
        got = np.fromfile(out, np.uint8)
        os.remove(out)
        return got

    return run


@functools.lru_cache(maxsize=None)
def formats():
    """(rows, origins) of `sample_formats formats`: rows {fmt: (Fmt as hyd_fmt_describe gives it, (ok, the format encoded back,
    cls, storage, a job's matrix, variant) of csrc/hip/hydk_store.h)} for fm.LO ... fm.HI - 1, and the int64 (cases, 3) origins"""
    got = sanitized_program("sample_formats")("formats")
    n = (fm.HI - fm.LO) * 18 * 4
    table = got[:n].view(np.int32).reshape(fm.HI - fm.LO, 18).tolist()
    rows = {fmt: (fm.Fmt(*row[:12]), tuple(row[12:])) for fmt, row in zip(range(fm.LO, fm.HI), table)}
    return rows, got[n:].view(np.int64).reshape(-1, 3)


def described(fmt):
    """hyd_fmt_describe(fmt), as the sanitized program printed it"""
    return formats()[0][fmt][0]
