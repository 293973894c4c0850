"""Record the calls the CPU tests make into the host glue's hooks (libhydrium_probe.so through ctypes) and replay them in a
stand-alone program built with the address and undefined-behaviour sanitizers (tests/c/host_replay.c).

TEST INFRASTRUCTURE ONLY.  A Recorder stands where a test module keeps its ctypes library: a call of a hook listed in SPECS
goes on to the real library and is kept as a record — scalars, every input buffer with the exact number of bytes the hook's
contract lets it read, every output buffer with its exact capacity and what it held before — together with what the call
gave.  The lengths come from the contract (SPECS below), not from the arrays a test happens to pass: the replay allocates
exactly that much, so a hook that reads or writes one byte more meets the allocator's redzone.

Nothing here loads sanitized code into Python: the sanitized build is a program of its own, started as a child process.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

from hydrium_amd import api, build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXC, ALPHA, GPL, LF_CODES, TILE_PIECES = 9, 128, 64, 384, 8
K_SCALAR, K_IN, K_OUT, K_OUTPTR, K_OUTLEN, K_ERR, K_LFARR, K_PTRARR = range(8)
F_NULL, F_STREAM = 1, 2
NONE = (1 << 64) - 1

SAN_FLAGS = ["-std=c99", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-DHYD_TEST_HOOKS", "-DHYDRIUM_INTERNAL_BUILD", f"-I{os.path.join(ROOT, 'include')}",
             f"-I{os.path.join(hbuild.CSRC, 'host')}"]
# the hooks that tiled.c defines without an export: other files call them, and the link counts those calls (host_replay.c)
WRAPPED = ("hydt_layout_from_streams", "hydt_layout_from_streams_skip")


# ---- what each argument of each hook is ------------------------------------------------------------------------------------
def sc():
    return ("scalar",)


def inp(length, stream=False):
    """an input buffer of length(v) bytes, v[i] = scalar argument i; stream: a byte stream by contract (any address)"""
    return ("in", length, stream)


def out(length):
    return ("out", length)


def obj_in():
    """byref(structure): its size"""
    return ("in", None, False)


def obj_out():
    return ("out", None)


def _dc_lengths(v, raw):
    """hydt_frame_from_stages' dc[s]: 3 planes of the LF group's varblocks, int32 (hydamd_read_dc)"""
    md = raw[0]._obj
    tw, th = api.tile_dims(md.width, md.height, md.tile_size_shift_x, md.tile_size_shift_y)
    xy = struct.unpack(f"<{2 * v[3]}I", C.string_at(_address(raw[4]), 8 * v[3]))
    lens = []
    for s in range(v[3]):
        w, h = min(tw, md.width - xy[2 * s] * tw), min(th, md.height - xy[2 * s + 1] * th)
        lens.append(3 * ((w + 7) // 8) * ((h + 7) // 8) * 4 if w > 0 and h > 0 else 0)
    return lens


def _frame(lf):
    return [obj_in(), sc(), sc(), sc(), inp(lambda v: 8 * v[3]), ("lfarr", lambda v: v[3]) if lf else ("ptrarr", _dc_lengths),
            inp(lambda v: v[3] * MAXC * ALPHA * 4), inp(lambda v: v[3] * MAXC * 4), inp(lambda v: v[3] * GPL * 4), sc(),
            inp(lambda v: v[11], True), sc(), inp(lambda v: v[13], True), sc(), ("outptr",), ("outlen",), ("err",)]


def _streams(n, first):
    """(lf, freq, alphabet, group_bits, max_alphabet, payload, payload_len) of n frames, from argument `first`"""
    return [("lfarr", lambda v: v[n]), inp(lambda v: v[n] * MAXC * ALPHA * 4), inp(lambda v: v[n] * MAXC * 4),
            inp(lambda v: v[n] * GPL * 4), inp(lambda v: v[n] * 4), inp(lambda v: v[first + 6], True), sc()]


def _head():
    return [inp(lambda v: LF_CODES), sc(), sc(), out(lambda v: v[4]), sc(), obj_out()]


def _piece_source(v, raw):
    """hydt_compose_pieces' src: the composer reads the source in aligned 32-bit words and "no word of the source that holds
    none of the string's bits" (hydk_pieces.h) — the last word a string touches, whole.  The source itself is 4-byte aligned
    here as in both device-side assemblers (HydkPiece.src), so it is no stream for the odd-address pass."""
    n = v[3]
    bits = struct.unpack(f"<{n}Q", C.string_at(_address(raw[1]), 8 * n)) if n else ()
    offs = struct.unpack(f"<{n}Q", C.string_at(_address(raw[2]), 8 * n)) if n else ()
    return max([(o + (b + 7) // 8 + 3) // 4 * 4 for o, b in zip(offs, bits) if b], default=0)


HOOKS = ["hydt_frame_from_stages", "hydamd_frame_from_streams", "hydt_lf_group", "hydt_lf_group_coded", "hydt_code_lengths",
         "hydt_small_code_lengths", "hydt_icc_mangled", "hydt_blob_class", "hydt_layout_from_streams", "hydt_layout_from_streams_skip",
         "hydt_mixed_from_streams", "hydt_mixed_from_streams_skip", "hydt_mixed_plan_counts", "hydt_mixed_plan_describe",
         "hydt_mixed_frame_plan_alone", "hydt_tiles_from_streams", "hydt_batch_from_streams", "hydt_compose_pieces",
         "hydt_ans_distribution_host", "hydt_ans_distribution_sections", "hydt_lf_head_host", "hydt_lf_head_sections", "hydt_lf_head_wave",
         "hydt_toc_entry_check", "hydt_shard_checks", "hydt_free", "hydt_blob_class:prefixes"]
PREFIXES = HOOKS.index("hydt_blob_class:prefixes")

SPECS = {
    "hydt_frame_from_stages": _frame(False),
    "hydamd_frame_from_streams": _frame(True),
    "hydt_lf_group": [inp(lambda v: 3 * v[1] * v[2] * 4), sc(), sc(), ("outptr",), ("outlen",)],
    "hydt_lf_group_coded": [sc(), sc(), inp(lambda v: LF_CODES), sc(), sc(), inp(lambda v: (v[6] + 7) // 8, True), sc(), ("outptr",),
                            ("outlen",)],
    "hydt_code_lengths": [inp(lambda v: 4 * v[2]), out(lambda v: 4 * v[2]), sc(), sc()],
    "hydt_small_code_lengths": [inp(lambda v: 4 * v[2]), out(lambda v: 4 * v[2]), sc(), sc()],
    "hydt_icc_mangled": [inp(lambda v: v[1], True), sc(), ("outptr",), ("outlen",)],
    "hydt_blob_class": [inp(lambda v: v[1], True), sc(), sc()],
    "hydt_mixed_from_streams": [sc(), inp(lambda v: 4 * v[0]), inp(lambda v: 4 * v[0])] + _streams(0, 3) +
                               [out(lambda v: 8 * (v[0] + 1)), ("outptr",), ("outlen",), ("err",)],
    "hydt_mixed_from_streams_skip": [sc(), inp(lambda v: 4 * v[0]), inp(lambda v: 4 * v[0])] + _streams(0, 3) +
                                    [inp(lambda v: 4 * v[0]), out(lambda v: 8 * (v[0] + 1)), out(lambda v: 4 * v[0]),
                                     out(lambda v: 16 * TILE_PIECES * v[0]), ("outptr",), ("outlen",), ("err",)],
    "hydt_mixed_plan_counts": [sc(), inp(lambda v: 4 * v[0]), inp(lambda v: 4 * v[0]), obj_out(), obj_out()],
    "hydt_mixed_plan_describe": [sc(), inp(lambda v: 4 * v[0]), inp(lambda v: 4 * v[0]), sc(), sc(), out(lambda v: 44 * v[0]),
                                 out(lambda v: 24), out(lambda v: 4 * 510), obj_out(), out(lambda v: 40), ("outptr",), ("outlen",),
                                 ("err",)],
    "hydt_mixed_frame_plan_alone": [sc(), sc(), ("outptr",), ("outlen",), ("err",)],
    "hydt_tiles_from_streams": [obj_in(), sc()] + _streams(1, 2) + [out(lambda v: 8 * (v[1] + 1)), ("outptr",), ("outlen",), ("err",)],
    "hydt_batch_from_streams": [obj_in(), sc()] + _streams(1, 2) + [out(lambda v: 8 * (v[1] + 1)), ("outptr",), ("outlen",), ("err",)],
    # out: "bytes [lo, lo + bytes) of `out` (4-byte aligned, whole words)"
    "hydt_compose_pieces": [inp(lambda v: 8 * v[3]), inp(lambda v: 8 * v[3]), inp(lambda v: 8 * v[3]), sc(), ("in", _piece_source, False),
                            sc(), sc(), out(lambda v: (v[5] + v[6] + 3) // 4 * 4)],
    "hydt_ans_distribution_host": [inp(lambda v: 4 * ALPHA), sc(), out(lambda v: v[3]), sc(), obj_out()],
    "hydt_ans_distribution_sections": [inp(lambda v: 4 * ALPHA), sc(), out(lambda v: v[3]), sc(), obj_out()],
    "hydt_lf_head_host": _head(),
    "hydt_lf_head_sections": _head(),
    "hydt_lf_head_wave": _head(),
    "hydt_toc_entry_check": [sc()],
    "hydt_shard_checks": [sc(), sc(), sc(), inp(lambda v: 4 * max(v[2], 0)), sc(), sc(), out(lambda v: 4 * max(v[2], 0)),
                          out(lambda v: 4 * max(v[2], 0))],
}


_V, _Z, _I, _U, _Q = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
_PV, _PZ, _PE, _MD = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_char_p), C.POINTER(api.HYDImageMetadata)
_FRAME = [_MD, _I, _I, _Z, _V, _V, _V, _V, _V, C.c_uint, _V, _Z, C.c_char_p, _Z, _PV, _PZ, _PE]
_BATCH = [_MD, _Z, _V, _V, _V, _V, _V, C.c_char_p, _Z, _V, _PV, _PZ, _PE]
_HEAD = [_V, _U, _U, _V, _Z, C.POINTER(_Q)]
# as the test modules declare them (glue.py, lf_model.py, test_sections.py, test_pieces.py, test_*_layout.py, test_*_sections.py)
ARGTYPES = {
    "hydt_frame_from_stages": _FRAME[:5] + [_PV] + _FRAME[6:],
    "hydamd_frame_from_streams": _FRAME,
    "hydt_lf_group": [_V, _Z, _Z, _PV, _PZ],
    "hydt_lf_group_coded": [_Z, _Z, _V, _U, _U, _V, _Q, _PV, _PZ],
    "hydt_code_lengths": [_V, _V, _U, _I],
    "hydt_small_code_lengths": [_V, _V, _U, _I],
    "hydt_icc_mangled": [C.c_char_p, _Z, _PV, _PZ],
    "hydt_blob_class": [C.c_char_p, _Z, _Z],
    "hydt_mixed_from_streams": [_Z, _V, _V, _V, _V, _V, _V, _V, C.c_char_p, _Z, _V, _PV, _PZ, _PE],
    "hydt_mixed_from_streams_skip": [_Z, _V, _V, _V, _V, _V, _V, _V, C.c_char_p, _Z, _V, _V, _V, _V, _PV, _PZ, _PE],
    "hydt_mixed_plan_counts": [_Z, _V, _V, C.POINTER(_U), _PZ],
    "hydt_mixed_plan_describe": [_Z, _V, _V, _I, _I, _V, _V, _V, C.POINTER(_Q), _V, _PV, _PZ, _PE],
    "hydt_mixed_frame_plan_alone": [_U, _U, _PV, _PZ, _PE],
    "hydt_tiles_from_streams": _BATCH,
    "hydt_batch_from_streams": _BATCH,
    "hydt_compose_pieces": [_V, _V, _V, _U, _V, _Q, _Q, _V],
    "hydt_ans_distribution_host": [_V, _U, _V, _Z, C.POINTER(_Q)],
    "hydt_ans_distribution_sections": [_V, _U, _V, _Z, C.POINTER(_Q)],
    "hydt_lf_head_host": _HEAD,
    "hydt_lf_head_sections": _HEAD,
    "hydt_lf_head_wave": _HEAD,
    "hydt_toc_entry_check": [_Q],
    "hydt_shard_checks": [_I, _I, _I, C.POINTER(_I), _I, _I, C.POINTER(_I), C.POINTER(_I)],
}


def _address(a):
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if hasattr(a, "_obj"):  # byref(x)
        return C.addressof(a._obj)
    if isinstance(a, (C.c_void_p, C.c_char_p)):
        return a.value or 0
    return C.addressof(a)  # an array or a structure


def _scalar(a):
    return int(a.value if hasattr(a, "value") else a)


def _length(spec, v, raw, a):
    fn = spec[1]
    if fn is None:
        return C.sizeof(a._obj)
    return int(fn(v, raw) if fn.__code__.co_argcount == 2 else fn(v))


class Record:
    __slots__ = ("hook", "blob", "ret", "err", "outs", "layout", "streams", "label")


class _Hook:
    def __init__(self, rec, name):
        self.__dict__.update(rec=rec, name=name, fn=getattr(rec.real, name))

    def __setattr__(self, key, value):  # restype, argtypes: the real function's
        setattr(self.fn, key, value)

    def __getattr__(self, key):
        return getattr(self.fn, key)

    def __call__(self, *raw):
        spec = SPECS[self.name]
        assert len(raw) == len(spec), (self.name, len(raw))
        v = [_scalar(a) if s[0] == "scalar" else None for s, a in zip(spec, raw)]
        parts, outs, streams = [], [], False
        for s, a in zip(spec, raw):
            kind = s[0]
            if kind == "scalar":
                parts.append(struct.pack("<IIQQ", K_SCALAR, 0, _scalar(a) & NONE, 0))
            elif kind in ("in", "out"):
                if isinstance(a, bytes):
                    n = _length(s, v, raw, a)
                    assert n <= len(a), (self.name, n, len(a))
                    data, null = a[:n], False
                else:
                    addr = _address(a)
                    null = addr == 0
                    n = 0 if null else _length(s, v, raw, a)
                    data = b"" if null else C.string_at(addr, n)
                flags = (F_NULL if null else 0) | (F_STREAM if kind == "in" and s[2] else 0)
                streams |= kind == "in" and s[2] and not null
                parts.append(struct.pack("<IIQQ", K_IN if kind == "in" else K_OUT, flags, n, 0) + data)
                if kind == "out" and not null:
                    outs.append(("out", _address(a), n))
            elif kind in ("outptr", "outlen", "err"):
                k = {"outptr": K_OUTPTR, "outlen": K_OUTLEN, "err": K_ERR}[kind]
                parts.append(struct.pack("<IIQQ", k, F_NULL if a is None else 0, 0, 0))
                if a is not None:
                    outs.append((kind, a._obj, 0))
            elif kind == "lfarr":
                addr, n = _address(a), s[1](v)
                body = []
                for i in range(0 if not addr else n):
                    lengths, alphabet, pairs, bits, count = struct.unpack("<QIIQQ", C.string_at(addr + 32 * i, 32))
                    body.append(struct.pack("<IIQ", alphabet, pairs, count))
                    body.append(struct.pack("<Q", LF_CODES) + C.string_at(lengths, LF_CODES) if lengths else struct.pack("<Q", NONE))
                    nb = (count + 7) // 8
                    body.append(struct.pack("<Q", nb) + C.string_at(bits, nb) if bits else struct.pack("<Q", NONE))
                streams |= bool(addr)
                parts.append(struct.pack("<IIQQ", K_LFARR, 0 if addr else F_NULL, n if addr else 0, 0) + b"".join(body))
            elif kind == "ptrarr":
                addr = _address(a)
                lens = s[1](v, raw) if addr else []
                ptrs = struct.unpack(f"<{len(lens)}Q", C.string_at(addr, 8 * len(lens))) if lens else ()
                body = [struct.pack("<Q", n) + C.string_at(p, n) if p else struct.pack("<Q", NONE) for p, n in zip(ptrs, lens)]
                parts.append(struct.pack("<IIQQ", K_PTRARR, 0 if addr else F_NULL, len(lens), 0) + b"".join(body))
        ret = self.fn(*raw)
        r = Record()
        r.hook, r.ret, r.err, r.outs, r.streams, r.label = HOOKS.index(self.name), int(ret), None, [], streams, self.name
        r.layout = [n if kind == "out" else "ptr" for kind, _, n in outs if kind in ("out", "outptr")]
        n_out = 0
        for kind, where, n in outs:
            if kind == "outlen":
                n_out = int(where.value)
        for kind, where, n in outs:
            if kind == "out":
                r.outs.append(C.string_at(where, n))
            elif kind == "outptr":
                r.outs.append(C.string_at(where.value, n_out) if ret == 0 and where.value else None)
            elif kind == "err":
                r.err = where.value
        r.blob = struct.pack("<II", r.hook, len(spec)) + b"".join(parts)
        self.rec.records.append(r)
        return ret


class Recorder:
    """Stands for the ctypes library of a test module: hooks of SPECS are recorded, everything else is the library's."""

    def __init__(self, real=None):
        hbuild.build()
        self.real = real if real is not None else C.CDLL(hbuild.HOSTTEST_PATH)
        self.records = []
        self._hooks = {}
        for name, types in ARGTYPES.items():
            getattr(self.real, name).restype, getattr(self.real, name).argtypes = C.c_int, types
        for name in ("hydt_free", "hydamd_free"):
            getattr(self.real, name).restype, getattr(self.real, name).argtypes = None, [_V]

    def __getattr__(self, name):
        if name in SPECS:
            if name not in self._hooks:
                self._hooks[name] = _Hook(self, name)
            return self._hooks[name]
        return getattr(self.real, name)

    def blob_prefixes(self, blob: bytes, expected: int):
        """every truncation of `blob` through hydt_blob_class: the classes through ctypes, and one record that has the replay
        program do the same, each prefix in an allocation of exactly its length"""
        fn = self.real.hydt_blob_class
        fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.c_size_t, C.c_size_t]
        classes = bytes(fn(blob[:k], k, expected) & 255 for k in range(len(blob) + 1))
        r = Record()
        r.hook, r.ret, r.err, r.outs, r.streams, r.label = PREFIXES, 0, None, [classes], True, "hydt_blob_class:prefixes"
        r.layout = [len(blob) + 1]
        r.blob = struct.pack("<II", PREFIXES, 3) + struct.pack("<IIQQ", K_IN, F_STREAM, len(blob), 0) + blob + \
            struct.pack("<IIQQ", K_SCALAR, 0, expected, 0) + struct.pack("<IIQQ", K_OUT, 0, len(blob) + 1, 0) + bytes(len(blob) + 1)
        self.records.append(r)
        return classes


# ---- the sanitized program -------------------------------------------------------------------------------------------------
def _run(cmd, timeout=600):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout + r.stderr


def build_program(workdir: str, extra_flags=()):
    """All of csrc/host/*.c and tests/c/host_replay.c with the sanitizers, at most 16 compilers at a time; the device functions
    the host files call (they live in csrc/hip/*.hip) become stubs that end the program.  -> (program, compiler output)"""
    os.makedirs(workdir, exist_ok=True)
    sources = sorted(glob.glob(os.path.join(hbuild.CSRC, "host", "*.c"))) + [os.path.join(ROOT, "tests", "c", "host_replay.c")]
    objects = [os.path.join(workdir, os.path.basename(s) + ".o") for s in sources]
    jobs = max(1, min(16, int(os.environ.get("MAX_JOBS") or os.cpu_count() or 1)))
    with ThreadPoolExecutor(jobs) as ex:
        done = list(ex.map(lambda so: _run([hbuild.CC] + SAN_FLAGS + list(extra_flags) + ["-c", so[0], "-o", so[1]]), zip(sources, objects)))
    log = "".join(text for _, text in done)
    if any(code for code, _ in done):
        raise RuntimeError("the sanitizer build failed:\n" + log)
    defined, wanted = set(), set()
    for o in objects:
        code, text = _run(["nm", "-g", o])
        assert code == 0, text
        for line in text.splitlines():
            f = line.split()
            (wanted if f[0] == "U" else defined).add(f[-1])
    missing = sorted(s for s in wanted - defined if s.startswith(("hydamd_", "hydk_", "hyd_")))
    stubs = os.path.join(workdir, "device_stubs.c")
    with open(stubs, "w") as f:
        f.write("/* written by tests/host_replay.py: a device function of csrc/hip, reached from the host, ends the program */\n"
                "void hydt_replay_device_call(const char *name);\n")
        for s in missing:
            f.write(f'void {s}(void) {{ hydt_replay_device_call("{s}"); }}\n')
        f.write(f"void hydt_replay_first_stub(void) {{ {missing[0]}(); }}\n")
    exe = os.path.join(workdir, "host_replay")
    code, text = _run([hbuild.CC] + SAN_FLAGS + list(extra_flags) + [stubs] + objects + [f"-Wl,--wrap={w}" for w in WRAPPED] +
                      ["-o", exe, "-lpthread", "-lm"])
    log += text
    if code:
        raise RuntimeError("the sanitizer link failed:\n" + log)
    return exe, log, missing


def replay(exe: str, records, workdir: str, tag: str, timeout=900):
    """-> (exit status, stderr, [(record, pass, ret, err, outs)], {hook: calls})"""
    rec_path, res_path, rep_path = (os.path.join(workdir, f"{tag}.{ext}") for ext in ("records", "results", "report"))
    with open(rec_path, "wb") as f:
        f.write(b"HYDRPLY1" + struct.pack("<I", len(records)))
        for r in records:
            f.write(r.blob)
    ran = subprocess.run([exe, rec_path, res_path, rep_path], capture_output=True, text=True, timeout=timeout)
    results, calls = [], {}
    if ran.returncode == 0:
        data = open(res_path, "rb").read()
        at = 0
        while at < len(data):
            idx, pas, ret, elen = struct.unpack_from("<IIiI", data, at)
            at += 16
            err = None
            if elen != 0xFFFFFFFF:
                err = data[at:at + elen]
                at += elen
            outs = []
            for want in records[idx].layout:
                if want == "ptr":
                    n, = struct.unpack_from("<Q", data, at)
                    at += 8
                    if n == NONE:
                        outs.append(None)
                    else:
                        outs.append(data[at:at + n])
                        at += n
                else:
                    outs.append(data[at:at + want])
                    at += want
            results.append((idx, pas, ret, err, outs))
        for line in open(rep_path):
            name, n = line.split()
            calls[name] = int(n)
    return ran.returncode, ran.stderr, results, calls
