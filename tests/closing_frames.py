"""Frames for tests/test_gpu_closing_launch.py, what the CPU oracle says about their HF sections, and the child process of
the payload-capacity test (python tests/closing_frames.py REPORT: HYDAMD_PAYLOAD_CAP is read when a context is created).

In a frame whose slots all leave their bits to k_rans_emit, the emit launch finds every section's byte offset itself and
writes a word that two sections share as byte stores.  What can go wrong depends on the sections' byte lengths and on where
they start inside a word, so the frames are chosen, with the oracle alone, to hold lengths of every residue mod 4 and shared
words split 1 | 3, 2 | 2 and 3 | 1.

Three sections in one word cannot be had from a picture: a populated group always codes a non-zero count per block and
channel, so its section holds the 32-bit final state and is at least four bytes long, and a group with g >= ngroups has no
section at all.  At most two sections meet in a word; the split of a word among up to four writers is held to account on the
CPU (tests/test_closing_edges.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hydrium_amd import synth  # noqa: E402
from oracle import binding as orc  # noqa: E402

GROUPS_PER_LFG = 64


def _ramp():
    """2304 x 520: slot 0 has 24 groups, slot 1 three — forty empty places (g >= ngroups) lie between the two slots' sections"""
    img = np.zeros((520, 2304, 3), np.uint8)
    img[:] = (np.arange(2304) // 9)[None, :, None]
    return img


FRAMES = {
    "flat_512": lambda: np.full((512, 512, 3), 128, np.uint8),          # four groups of four bytes each
    "photo_520x264": lambda: synth.make_image("photo", 520, 264, 8),    # ragged groups
    "ramp_2304x520": _ramp,
}
BATCH = [lambda: synth.make_image("photo", 256, 256, 8), lambda: synth.make_image("photo", 256, 256, 8, seed=99)]


def oracle_frame(img):
    """(payload bytes, bits[slots * 64], offsets[slots * 64]) of a one-frame image, slot by slot in send order."""
    h, w, _ = img.shape
    lfx, lfy = -(-w // 2048), -(-h // 2048)
    payload, bits, offs, mx = b"", [], [], 0
    for ty in range(lfy):
        for tx in range(lfx):
            res, mx = orc.encode_lf_group(np.ascontiguousarray(img), tx, ty, max_alphabet_size=mx)
            b = np.zeros(GROUPS_PER_LFG, np.int64)
            b[:res.num_groups] = res.group_bits
            nbytes = (b + 7) >> 3
            o = len(payload) + np.concatenate(([0], np.cumsum(nbytes)[:-1]))
            assert np.array_equal(o[:res.num_groups] - len(payload), res.group_offset)
            bits.append(b)
            offs.append(o)
            payload += res.stream
    return payload, np.concatenate(bits), np.concatenate(offs)


def section_facts(bits):
    """(byte lengths mod 4 that occur, splits a|b of words shared by two sections, most sections in one word)"""
    nbytes = (np.asarray(bits, np.int64) + 7) >> 3
    mods, splits, per_word, at = set(), set(), {}, 0
    for n in nbytes:
        n = int(n)
        if n:
            mods.add(n % 4)
            for wd in range(at // 4, (at + n - 1) // 4 + 1):
                per_word[wd] = per_word.get(wd, 0) + 1
            if at % 4 and at:
                splits.add((at % 4, 4 - at % 4))
        at += n
    return mods, splits, max(per_word.values())


def torch_image(img):
    import torch

    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def child(report_path):
    """The ragged photo frame with the payload sized to exactly its section bytes, and one byte short, through the device
    API and through the drop-in API; writes what came back."""
    import hashlib
    import json

    from hydrium_amd import api, device

    img = FRAMES["photo_520x264"]()
    want, bits, offs = oracle_frame(img)
    t = torch_image(img)
    report = {"B": len(want), "want_md5": hashlib.md5(want).hexdigest(), "runs": {}}
    lib = api.Library()
    for name, cap in (("exact", len(want)), ("short", len(want) - 1)):
        print(f"CASE {name}: HYDAMD_PAYLOAD_CAP {cap}", flush=True)
        os.environ["HYDAMD_PAYLOAD_CAP"] = str(cap)
        with device.DeviceContext(0, 1, 0) as ctx:
            ctx.encode_image_tensor(t)
            ctx.sync()
            got = ctx.read_payload()
            gbits, goffs = ctx.read_sections(0)
            run = {"payload_ok": got == want, "payload_md5": hashlib.md5(got).hexdigest(), "reruns": ctx.overflow_reruns(),
                   "bits_ok": bool(np.array_equal(gbits, bits)), "offsets_ok": bool(np.array_equal(goffs, offs))}
        lib.dll.hydamd_trim_cache()   # parked contexts keep the caps they were created with
        run["file_md5"] = hashlib.md5(bytes(api.encode_image(lib, img.copy(), out_buf_size=1 << 22))).hexdigest()
        report["runs"][name] = run
        with open(report_path, "w") as f:
            json.dump(report, f)
    lib.dll.hydamd_trim_cache()
    report["done"] = True
    with open(report_path, "w") as f:
        json.dump(report, f)
    return 0


if __name__ == "__main__":
    sys.exit(child(sys.argv[1]))
