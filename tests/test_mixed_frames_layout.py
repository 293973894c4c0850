"""Mixed-size batches whose images hold several LF groups, without a GPU: the shipped library exports the two new calls and
the binding agrees with the header, creation refuses what it must before any device is touched, and the product's planner
(csrc/host/mixed.c, build_frames_plan, through the hosttest flavour's hook) lays a list of sizes out as the device follows
it — slots, pieces, the workgroup table, every frame's share of the assembler's scratch — with every frame of several LF
groups carrying exactly the frame plan a uniform batch of its shape gets."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hydrium_amd import build as hbuild, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["hydamd_mixed_create_slots", "hydamd_begin_batch_frames"]
API_ERROR = -14
SIZES = [(2049, 8), (200, 120), (8, 4097), (256, 256), (2049, 2049), (520, 264), (2049, 8)]
MAX_FRAMES, MAX_SLOTS = 7, 14

_CTYPE = {"int": C.c_int, "size_t": C.c_size_t, "ptrdiff_t": C.c_ssize_t, "unsigned": C.c_uint}


def test_the_shipped_library_exports_the_new_calls_and_no_hook():
    lib = hbuild.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in exported if s.startswith(("hydk_", "hydt_"))]


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    m = re.search(r"HYDAMD_EXPORT\s+([^;]*?)\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return " ".join(m.group(1).split()), [" ".join(a.split()) for a in m.group(2).split(",")]


def _kind(decl):
    if "*" in decl or "[" in decl:
        return "ptr"
    return _CTYPE[[w for w in decl.split() if w != "const"][0]]


def _ctypes_kind(t):
    return "ptr" if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents") or hasattr(t, "_type_") and isinstance(t._type_, type) else t


@pytest.mark.parametrize("name", SYMBOLS)
def test_binding_and_header_agree(name):
    fn = getattr(device.dll(), name)
    ret, args = _prototype(name)
    assert len(fn.argtypes) == len(args), (name, args)
    for decl, t in zip(args, fn.argtypes):
        assert _ctypes_kind(t) == _kind(decl), (name, decl, t)
    assert _ctypes_kind(fn.restype) == _kind(ret + " x"), (name, ret, fn.restype)


@pytest.mark.parametrize("max_frames,max_lf_groups,word", [(4, 256, b"max_lf_groups"), (8, 7, b"max_lf_groups"), (0, 31, b"max_lf_groups"),
                                                           (4, -1, b"max_lf_groups"), (256, 255, b"max_frames"), (-1, 8, b"max_frames")])
def test_what_creation_refuses_needs_no_device(max_frames, max_lf_groups, word):
    d = device.dll()
    st = C.c_int(0)
    assert not d.hydamd_mixed_create_slots(0, max_frames, max_lf_groups, 0, C.byref(st))
    assert st.value == API_ERROR and word in d.hydamd_mixed_error(None)
    with pytest.raises(device.DeviceError, match=word.decode()):
        device.MixedBatch(max_frames, max_lf_groups=max_lf_groups)


# ---- the planner ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooks():
    hbuild.build()
    d = C.CDLL(hbuild.HOSTTEST_PATH)
    d.hydt_mixed_plan_describe.restype = C.c_int
    d.hydt_mixed_plan_describe.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_char_p)]
    d.hydt_mixed_frame_plan_alone.restype = C.c_int
    d.hydt_mixed_frame_plan_alone.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
    d.hydt_free.argtypes = [C.c_void_p]
    return d


def _describe(d, sizes, max_frames=MAX_FRAMES, max_slots=MAX_SLOTS):
    w = np.array([s[0] for s in sizes], np.uint32)
    h = np.array([s[1] for s in sizes], np.uint32)
    per = np.zeros((len(sizes), 11), np.uint32)
    counts, parts, caps = np.zeros(6, np.uint32), np.zeros(510, np.uint32), np.zeros(5, np.uint64)
    fixed, plan, plan_len, err = C.c_uint64(0), C.c_void_p(0), C.c_size_t(0), C.c_char_p()
    st = d.hydt_mixed_plan_describe(len(sizes), w.ctypes.data, h.ctypes.data, max_frames, max_slots, per.ctypes.data, counts.ctypes.data,
                                    parts.ctypes.data, C.byref(fixed), caps.ctypes.data, C.byref(plan), C.byref(plan_len), C.byref(err))
    if st:
        return st, err.value
    raw = C.string_at(plan.value, plan_len.value)
    d.hydt_free(plan)
    return dict(frames=per, nplans=int(counts[0]), nshapes=int(counts[1]), parts=parts[: int(counts[2])], npieces=int(counts[3]),
                slots=int(counts[4]), plan=raw, fixed=int(fixed.value), caps=[int(c) for c in caps])


KIND, FIRST, N, PLAN_OFF, PIECE, HFG_OFF, HFG_N, TOC_OFF, TOC_N, SIZES_OFF, SIZES_N = range(11)


@pytest.fixture(scope="module")
def plan(hooks):
    p = _describe(hooks, SIZES)
    assert isinstance(p, dict), p
    return p


def test_slots_pieces_and_kinds(plan):
    f = plan["frames"]
    assert f[:, N].tolist() == [2, 1, 3, 1, 4, 1, 2]
    assert f[:, FIRST].tolist() == [0, 2, 3, 6, 7, 11, 12] and plan["slots"] == 14
    assert f[:, KIND].tolist() == [1, 0, 1, 0, 1, 0, 1]
    assert f[:, PIECE].tolist() == np.concatenate([[0], np.cumsum(3 * f[:, N] + 5)[:-1]]).tolist()
    assert plan["npieces"] == int(np.sum(3 * f[:, N] + 5))


def test_images_of_one_size_share_a_plan(plan):
    f = plan["frames"]
    assert plan["nplans"] == 3 and plan["nshapes"] == 3
    assert f[0, PLAN_OFF] == f[6, PLAN_OFF] != 0
    assert len({int(f[k, PLAN_OFF]) for k in (0, 2, 4)}) == 3
    assert all(f[k, PLAN_OFF] == 0 for k in (1, 3, 5))
    assert all(int(off) % 16 == 0 for off in f[:, PLAN_OFF])


def test_the_workgroup_table_deals_the_frames_of_several_lf_groups_in_order(plan):
    f = plan["frames"]
    want = [(k << 8) | part for k in (0, 2, 4, 6) for part in range(int(f[k, N]) + 1)]
    assert plan["parts"].tolist() == want and len(want) == (2 + 1) + (3 + 1) + (4 + 1) + (2 + 1)


def test_scratch_shares_are_disjoint_and_inside_what_creation_allocates(plan):
    f = plan["frames"].astype(np.int64)
    head, hfg, toc, sizes, pieces = plan["caps"]
    assert head >= 704 * MAX_SLOTS  # a slot's head holds either layout's: 704 (one LF group) >= 640 words
    for off, n, cap in [(HFG_OFF, HFG_N, hfg), (TOC_OFF, TOC_N, toc), (SIZES_OFF, SIZES_N, sizes)]:
        end = 0
        for k in range(len(SIZES)):
            assert f[k, off] >= end, (k, off)  # batch order, no overlap
            end = f[k, off] + f[k, n]
        assert end <= cap
    assert plan["npieces"] <= pieces
    for k in range(len(SIZES)):
        if f[k, KIND]:  # what hydk_batch_create gives a uniform batch of the shape: TOC entries + 2 words, a size per entry
            groups = sum(((min(2048, SIZES[k][0] - x) + 255) // 256) * ((min(2048, SIZES[k][1] - y) + 255) // 256)
                         for y in range(0, SIZES[k][1], 2048) for x in range(0, SIZES[k][0], 2048))
            assert f[k, SIZES_N] == 2 + f[k, N] + groups and f[k, TOC_N] == f[k, SIZES_N] + 2
            assert f[k, HFG_N] >= 73 * 9 * f[k, N] + 2
        else:
            assert f[k, HFG_N] == 3072 and f[k, TOC_N] == 80 and f[k, SIZES_N] == 0
    assert plan["fixed"] > 0


def test_the_2x2_image_has_groups_of_64_8_8_and_1(plan, hooks):
    """the list's 2049 x 2049 image: four LF groups of 64, 8, 8 and 1 groups — 81 sections behind LFGlobal, the LF groups and HFGlobal"""
    assert plan["frames"][4, SIZES_N] == 2 + 4 + 64 + 8 + 8 + 1


@pytest.mark.parametrize("k", [0, 2, 4, 6])
def test_a_frame_of_several_lf_groups_carries_the_plan_of_that_image_alone(plan, hooks, k):
    p, n, err = C.c_void_p(0), C.c_size_t(0), C.c_char_p()
    assert hooks.hydt_mixed_frame_plan_alone(SIZES[k][0], SIZES[k][1], C.byref(p), C.byref(n), C.byref(err)) == 0, err.value
    alone = C.string_at(p.value, n.value)
    hooks.hydt_free(p)
    off = int(plan["frames"][k, PLAN_OFF])
    assert len(alone) >= 64 and plan["plan"][off: off + len(alone)] == alone


def test_the_same_list_plans_the_same_bytes(hooks, plan):
    assert _describe(hooks, SIZES)["plan"] == plan["plan"]


def test_what_the_planner_refuses(hooks):
    st, msg = _describe(hooks, [(2048 * 28 + 1, 8)], 1, 255)
    assert st == API_ERROR and b"28 LF groups" in msg
    st, msg = _describe(hooks, [(2048 * 5 + 1, 2048 * 5 + 1)], 1, 255)  # 6 x 6
    assert st == API_ERROR and b"28 LF groups" in msg
    for size in [(0, 8), (8, 0)]:
        st, msg = _describe(hooks, [(64, 64), size], 2, 8)
        assert st == API_ERROR
    st, msg = _describe(hooks, SIZES, MAX_FRAMES, MAX_SLOTS - 1)
    assert st == API_ERROR and b"more LF groups than the object has slots" in msg
    assert isinstance(_describe(hooks, [(2048 * 27 + 1, 8)], 1, 28), dict)  # the cap itself


def test_the_largest_batches_fit_the_scratch_creation_allocates(hooks):
    """255 slots in frames of 28 LF groups (the longest cluster maps and TOCs) and in frames of one"""
    p = _describe(hooks, [(2048 * 28, 2048)] * 9 + [(2048 * 3, 8)], 10, 255)
    assert isinstance(p, dict) and p["slots"] == 255 and p["npieces"] <= 2040
    p = _describe(hooks, [(2048 * 4, 2048 * 7)] * 9 + [(2048 * 3, 2048)], 10, 255)
    assert isinstance(p, dict), p
    p = _describe(hooks, [(64 + k, 64) for k in range(255)], 255, 255)
    assert isinstance(p, dict) and p["npieces"] == 2040 and len(p["parts"]) == 0
