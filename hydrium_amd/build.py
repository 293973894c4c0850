"""In-tree build of libhydrium.so.0 (host C + HIP kernels for gfx950).

Everything is compiled with -ffp-contract=off: the reference's canonical bytes are the
non-contracted ones.  Objects go to hydrium_amd/build/, the library to hydrium_amd/lib/ (both
git-ignored; the built library travels to the GPU box with the gpurun snapshot).
"""
from __future__ import annotations

import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ_DIR = os.path.join(HERE, "build")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libhydrium.so.0")
# the same sources under -DHYD_TEST_HOOKS: the host glue's test entry points (CPU-only tests) and the measurement / fault
# injection switches of the device side (HYDAMD_DEBUG_*, HYDAMD_TEST_*), which the shipped library does not contain.
# Loaded explicitly (tests/glue.py, scripts/pipe_probe.py, HYDAMD_LIB=...): never what a user of libhydrium.so.0 gets.
PROBE_PATH = os.path.join(LIB_DIR, "libhydrium_probe.so")
HOSTTEST_PATH = PROBE_PATH
# HIP sources that read HYD_TEST_HOOKS (the others are compiled once and shared by both flavours)
HOOKED_HIP = ("device_api.hip", "assemble.hip")

ARCH = os.environ.get("HYDAMD_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CC = os.environ.get("CC", "gcc")

HIP_FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
             "-fno-slp-vectorize",  # packed-f32 chains need a wait state per dependent op on gfx950: slower than scalar
             "-Wall", "-Wno-unused-function", f"-I{os.path.join(ROOT, 'include')}"]
C_FLAGS = ["-std=c99", "-O2", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden", "-Wall", "-Wextra",
           "-Wno-unused-parameter", "-DHYDRIUM_INTERNAL_BUILD", f"-I{os.path.join(ROOT, 'include')}",
           f"-I{os.path.join(CSRC, 'host')}"]


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        raise RuntimeError(f"build step failed: {cmd[0]} ... {cmd[-1]}")
    return r


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJ_DIR, exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    headers = glob.glob(os.path.join(CSRC, "**", "*.h"), recursive=True) + \
        glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True)
    objs, test_objs = [], []
    for src in sorted(glob.glob(os.path.join(CSRC, "hip", "*.hip"))):
        obj = os.path.join(OBJ_DIR, os.path.basename(src) + ".o")
        if force or _newer(obj, [src] + headers):
            if verbose:
                print("hipcc", os.path.basename(src))
            _run([HIPCC] + HIP_FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)
        if os.path.basename(src) in HOOKED_HIP:
            tobj = os.path.join(OBJ_DIR, os.path.basename(src) + ".test.o")
            if force or _newer(tobj, [src] + headers):
                if verbose:
                    print("hipcc -DHYD_TEST_HOOKS", os.path.basename(src))
                _run([HIPCC] + HIP_FLAGS + ["-DHYD_TEST_HOOKS", "-c", src, "-o", tobj])
            test_objs.append(tobj)
        else:
            test_objs.append(obj)
    for src in sorted(glob.glob(os.path.join(CSRC, "host", "*.c"))):
        obj = os.path.join(OBJ_DIR, os.path.basename(src) + ".o")
        if force or _newer(obj, [src] + headers):
            if verbose:
                print("cc", os.path.basename(src))
            _run([CC] + C_FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)
        tobj = os.path.join(OBJ_DIR, os.path.basename(src) + ".test.o")
        if force or _newer(tobj, [src] + headers):
            _run([CC] + C_FLAGS + ["-DHYD_TEST_HOOKS", "-c", src, "-o", tobj])
        test_objs.append(tobj)
    if force or _newer(LIB_PATH, objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-Wl,-soname,libhydrium.so.0", "-o", LIB_PATH] + objs + ["-lpthread"])
    if force or _newer(PROBE_PATH, test_objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-Wl,-soname,libhydrium.so.0", "-o", PROBE_PATH] + test_objs + ["-lpthread"])
    stale = os.path.join(LIB_DIR, "libhydrium_hosttest.so")  # until round 5 the test flavour's name
    if os.path.exists(stale):
        os.remove(stale)
    return LIB_PATH


# ---- build-time variants: the shipped library with kernels.hip (and lf_coder.hip for HYDK_LF_* defines) recompiled ----
VARIANT_DIR = os.path.join(OBJ_DIR, "variants")


def _defines(defines) -> list:
    items = defines.items() if isinstance(defines, dict) else (d.partition("=")[::2] for d in defines)
    return [f"-D{k}={v}" if str(v) != "" else f"-D{k}" for k, v in sorted((str(k), v) for k, v in items)]


def _flavour_objects(probe: bool = False) -> list:
    """The objects build() links into libhydrium.so.0 (probe: into libhydrium_probe.so), in its order."""
    hip = [os.path.basename(s) for s in sorted(glob.glob(os.path.join(CSRC, "hip", "*.hip")))]
    host = [os.path.basename(s) for s in sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))]
    return [os.path.join(OBJ_DIR, f + (".test.o" if probe and f in HOOKED_HIP else ".o")) for f in hip] + \
        [os.path.join(OBJ_DIR, f + (".test.o" if probe else ".o")) for f in host]


def _variant_plan(name: str, defines, probe: bool = False):
    import hashlib

    flags = _defines(defines)
    srcs = ["kernels.hip"] + (["lf_coder.hip"] if any(f.startswith("-DHYDK_LF_") for f in flags) else [])
    # (paths relative to the tree: a copy of the tree elsewhere finds its variants current)
    h = hashlib.sha256("\0".join([ARCH, HIPCC, "probe" if probe else "shipped"] + HIP_FLAGS + flags).replace(ROOT, "").encode())
    files = sorted(glob.glob(os.path.join(CSRC, "**", "*.*"), recursive=True) + glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True))
    for f in files:  # a content stamp, not mtimes: the variant is current when no source it was linked from changed
        with open(f, "rb") as fh:
            h.update(os.path.relpath(f, ROOT).encode() + b"\0" + fh.read())
    out = os.path.join(VARIANT_DIR, name)
    return flags, srcs, h.hexdigest(), out, os.path.join(out, "libhydrium.so.0")


def variant_path(name: str) -> str:
    return os.path.join(VARIANT_DIR, name, "libhydrium.so.0")


def _variant_current(name: str, defines, probe: bool) -> bool:
    _, _, stamp, out, lib = _variant_plan(name, defines, probe)
    try:
        with open(os.path.join(out, "stamp")) as f:
            return os.path.exists(lib) and f.read() == stamp
    except OSError:
        return False


def build_variants(specs: dict, jobs: int = 0, probe: bool = False) -> dict:
    """{name: defines} -> {name: path of hydrium_amd/build/variants/<name>/libhydrium.so.0}.

    A variant is what the product would be if its defines were the defaults: kernels.hip (and lf_coder.hip when a HYDK_LF_*
    define is given) recompiled with them, linked with the SHIPPED flavour's other objects (not the HYD_TEST_HOOKS ones).
    Only stale variants are rebuilt (a content stamp of the sources and flags), with at most min(16, MAX_JOBS) compilers.
    probe=True links the HYD_TEST_HOOKS flavour's objects instead (measurement builds that use HYDAMD_DEBUG_*)."""
    from concurrent.futures import ThreadPoolExecutor

    todo = {n: d for n, d in specs.items() if not _variant_current(n, d, probe)}
    if todo:
        build()
        base = _flavour_objects(probe)
        jobs = jobs or int(os.environ.get("MAX_JOBS") or os.cpu_count() or 1)
        jobs = max(1, min(16, jobs))
        compiles = []
        for name, d in todo.items():
            flags, srcs, _, out, _ = _variant_plan(name, d, probe)
            os.makedirs(out, exist_ok=True)
            for s in srcs:
                compiles.append([HIPCC] + HIP_FLAGS + flags + ["-c", os.path.join(CSRC, "hip", s), "-o", os.path.join(out, s + ".o")])
        with ThreadPoolExecutor(jobs) as ex:
            list(ex.map(_run, compiles))
        for name, d in todo.items():
            flags, srcs, stamp, out, lib = _variant_plan(name, d, probe)
            objs = [os.path.join(out, os.path.basename(o)[:-2] + ".o") if os.path.basename(o)[:-2] in srcs else o for o in base]
            _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-Wl,-soname,libhydrium.so.0", "-o", lib] + objs + ["-lpthread"])
            with open(os.path.join(out, "stamp"), "w") as f:
                f.write(stamp)
    return {n: variant_path(n) for n in specs}


def build_variant(name: str, defines, probe: bool = False) -> str:
    """One variant (see build_variants); `defines` is {NAME: value} or ["NAME=value", ...]."""
    return build_variants({name: defines}, probe=probe)[name]


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
