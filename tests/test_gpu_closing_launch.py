"""GPU: the closing stage of a frame whose emit launch places its own sections, against the CPU oracle and the reference.

A frame whose slots all leave their bits to k_rans_emit runs no scan kernel: every wavefront of the emit launch sums the
byte sizes of the groups before its own, writes offsets[G] (for the empty places g >= ngroups too), and stores the words
its section shares with a neighbour as byte stores of its own bytes; the wavefront of group 0 writes the total and the
payload overflow status.  tests/closing_frames.py picks frames, with the oracle alone, whose sections have byte lengths of
every residue mod 4 and share words at every split; here their payload, offsets[], total and whole file are compared, the
payload is sized to exact fit and one byte short, and a batch that mixes an integer and a float picture (which keeps the
scan kernel and the ORing emit) is held to each picture coded alone.

The frame's packed LF area: the window offsets come from the wavefront that builds a slot's code and the pack workgroups
replace exactly their own bits of a word two windows share.  A three-slot frame (bit counts that are no multiples of 32, one
slot a flat plane) must give the slots' streams of tests/lf_model.py back to back at 4-byte alignment with zero bytes
between them, the same from the in-stream coder, the side stream and three growing hydamd_run_lf_coder calls, and again
on a second visit of the same context; read_lf_bits asked for more than a slot's stream gives zero beyond its end, also
where an earlier, longer stream lay in the slot's words."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu, reference_expected

import closing_frames as cf

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120
BEYOND = 64   # bytes asked of read_lf_bits beyond a slot's stream


@pytest.fixture(scope="module")
def oracle_frames():
    """name -> (image, payload, bits, offsets), computed once; checked to hold what the tests below are about"""
    out = {name: (img,) + cf.oracle_frame(img) for name, img in ((n, f()) for n, f in cf.FRAMES.items())}
    for k, f in enumerate(cf.BATCH):
        img = f()
        out[f"batch_{k}"] = (img,) + cf.oracle_frame(img)
    mods, splits, most = set(), set(), 0
    for name, (_, _, bits, _) in out.items():
        m, s, p = cf.section_facts(bits)
        print(f"  {name}: byte lengths mod 4 {sorted(m)}, shared-word splits {sorted(s)}, at most {p} sections in a word")
        mods |= m
        splits |= s
        most = max(most, p)
    assert {1, 2, 3} <= mods, f"no section of every byte length mod 4 in the chosen frames: {sorted(mods)}"
    assert {(1, 3), (2, 2), (3, 1)} <= splits, f"shared words of every split are not all there: {sorted(splits)}"
    assert most == 2   # never more from a picture (closing_frames.py says why); up to four writers per word: test_closing_edges.py
    bits = out["ramp_2304x520"][2]
    assert bits[:24].all() and not bits[24:64].any() and bits[64:67].all(), "empty places between populated slots"
    assert list((out["flat_512"][2][:4] + 7) >> 3) == [4, 4, 4, 4]
    return out


def _sections(ctx, slots):
    pairs = [ctx.read_sections(s) for s in range(slots)]
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


@pytest.mark.parametrize("form", [5, 4])  # lane form: the self-placing emit; wave form: scan kernel in front, as before
@pytest.mark.parametrize("name", list(cf.FRAMES))
def test_sections_that_share_words(oracle_frames, ref_lib, name, form):
    from hydrium_amd import api, device

    img, want, bits, offs = oracle_frames[name]
    slots = len(bits) // cf.GROUPS_PER_LFG
    t = cf.torch_image(img)
    with device.DeviceContext(0, slots, 0) as ctx:
        ctx.set_rans_waves(form)
        for visit in range(2):   # the second visit meets the first one's bytes in every shared word
            ctx.encode_image_tensor(t)
            ctx.sync()
            assert ctx.payload_size() == len(want), f"total, visit {visit}"
            got_bits, got_offs = _sections(ctx, slots)
            assert np.array_equal(got_bits, bits), f"section bits, visit {visit}"
            assert np.array_equal(got_offs, offs), f"offsets[], empty places included, visit {visit}"
            assert ctx.read_payload() == want, f"payload, visit {visit}"
        assert ctx.overflow_reruns() == 0
    assert reference_expected()
    assert bytes(api.encode_image(api.Library(), img.copy())) == bytes(api.encode_image(ref_lib, img.copy())), "whole file"


def test_two_frame_batch(oracle_frames, ref_lib):
    from hydrium_amd import api, device

    frames = [oracle_frames[f"batch_{k}"] for k in range(len(cf.BATCH))]
    tensors = [cf.torch_image(f[0]) for f in frames]
    want = b"".join(f[1] for f in frames)
    with device.DeviceContext(0, len(frames), 0) as ctx:
        ctx.encode_image_batch(tensors)
        ctx.sync()
        assert ctx.payload_size() == len(want)
        got_bits, got_offs = _sections(ctx, len(frames))
        base = 0
        for k, (_, payload, bits, offs) in enumerate(frames):
            sl = slice(k * cf.GROUPS_PER_LFG, (k + 1) * cf.GROUPS_PER_LFG)
            assert np.array_equal(got_bits[sl], bits), f"frame {k}: section bits"
            assert np.array_equal(got_offs[sl], offs + base), f"frame {k}: offsets[]"
            base += len(payload)
        assert ctx.read_payload() == want
    assert reference_expected()
    with device.FrameBatch(256, 256, len(frames)) as fb:
        fb.encode(tensors)
        files = fb.read()
    for k, f in enumerate(frames):
        assert bytes(files[k]) == bytes(api.encode_image(ref_lib, f[0].copy())), f"frame {k}: whole file"


def test_payload_at_exact_fit_and_one_byte_short(oracle_frames, ref_lib, tmp_path):
    from hydrium_amd import api

    img, want, _, _ = oracle_frames["photo_520x264"]
    report = str(tmp_path / "report.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("HYDAMD_")}
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "closing_frames.py"), report], capture_output=True, text=True,
                       env=env, timeout=CHILD_TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, f"child ended with {r.returncode} after {r.stdout.splitlines()[-1:]}\n{r.stderr[-3000:]}"
    with open(report) as f:
        rep = json.load(f)
    assert rep.get("done") and rep["B"] == len(want) and rep["want_md5"] == hashlib.md5(want).hexdigest()
    assert reference_expected()
    file_md5 = hashlib.md5(bytes(api.encode_image(ref_lib, img.copy(), out_buf_size=1 << 22))).hexdigest()
    for name, reruns in (("exact", 0), ("short", 1)):
        run = rep["runs"][name]
        print(f"  {name}: {run}")
        assert run["payload_ok"] and run["payload_md5"] == rep["want_md5"], f"{name}: sections"
        assert run["bits_ok"] and run["offsets_ok"], f"{name}: section bits and offsets"
        assert run["reruns"] == reruns, f"{name}: {run['reruns']} reruns"
        assert run["file_md5"] == file_md5, f"{name}: whole file"


def test_an_integer_and_a_float_picture_in_one_batch(oracle_frames):
    """The float picture's 8-byte records keep the whole launch group on the wave form: scan kernel, ORing emit or pack."""
    import torch

    from hydrium_amd import device, synth

    a = cf.torch_image(oracle_frames["photo_520x264"][0])
    b = torch.from_numpy(synth.make_image_f32("photo", 264, 200)).cuda()
    with device.MixedBatch(2) as mb:
        alone = []
        for t in (a, b):
            mb.encode([t])
            alone.append(bytes(mb.read(0)))
        mb.encode([a, b], sample_fmts="each")
        both = [bytes(f) for f in mb.read()]
        mb.encode([b, a], sample_fmts="each")
        swapped = [bytes(f) for f in mb.read()]
    assert both == alone and swapped == alone[::-1]


# ---- the frame's packed LF area ----------------------------------------------------------------------------------------
def _lf_frame():
    """4200 x 72 RGB8, three LF groups in a row: photo content, a flat plane (its stream is runs of one value), a narrow rest"""
    from hydrium_amd import synth

    img = synth.make_image("photo", 4200, 72, 8).copy()
    img[:, 2048:4096] = 77
    return img


@pytest.fixture(scope="module")
def lf_frame():
    """(image, per slot: (bits as bytes, bit count) of tests/lf_model.py from the oracle's LF ints)"""
    from tests import lf_model

    img = _lf_frame()
    slots, mx = [], 0
    for tx in range(3):
        res, mx = cf.orc.encode_lf_group(img, tx, 0, max_alphabet_size=mx)
        _, _, _, _, bits, nbits = lf_model.model(res.dc)
        slots.append((np.asarray(bits[:(nbits + 7) // 8], np.uint8), int(nbits)))
    assert all(n % 32 for _, n in slots), f"bit counts that are multiples of 32: {[n for _, n in slots]}"
    assert slots[1][1] < slots[0][1] // 8, "the flat plane's stream is not the short one"
    return img, slots


def _check_lf_area(ctx, slots, where):
    info, blob = ctx.read_lf_streams(len(slots)), ctx.read_lf_payload().copy()
    end = 0
    for s, (bits, nbits) in enumerate(slots):
        assert int(info["error"][s]) == 0 and int(info["bit_count"][s]) == nbits, f"{where}: slot {s} bit count"
        off, nbytes = int(info["offset"][s]), (nbits + 7) // 8
        assert off == end, f"{where}: slot {s} starts at {off}, the slots before it end at {end}"
        got = blob[off:off + nbytes].copy()
        want = bits.copy()
        if nbits % 8:   # the model leaves the last byte's spare bits zero; so does the device
            assert got[-1] >> (nbits % 8) == 0, f"{where}: slot {s}: bits behind the stream's end in its last byte"
        assert np.array_equal(got, want), f"{where}: slot {s} differs from the model"
        end = off + (nbits + 31) // 32 * 4
        assert not blob[off + nbytes:end].any(), f"{where}: slot {s}: bytes between the stream's end and the next slot"
        assert np.array_equal(ctx.read_lf_bits(s, nbits), got), f"{where}: read_lf_bits({s}) is not the slot's slice"
        more = ctx.read_lf_bits(s, nbits + 8 * BEYOND)   # a capacity beyond the stream's end: the slice, then zero
        assert len(more) == nbytes + BEYOND and np.array_equal(more[:nbytes], got), f"{where}: read_lf_bits({s}), larger capacity"
        assert not more[nbytes:].any(), f"{where}: read_lf_bits({s}): bytes beyond the stream's end are not zero"
    assert end == len(blob), f"{where}: the LF payload is {len(blob)} bytes, the slots end at {end}"
    return blob.tobytes()


def test_lf_area_is_the_slots_streams_at_four_byte_alignment(lf_frame):
    from hydrium_amd import device, synth

    img, slots = lf_frame
    t = cf.torch_image(img)
    blobs = {}
    for name, coder in (("in the stream", 2), ("side stream", 1)):
        with device.DeviceContext(0, 3, 0) as ctx:
            ctx.set_lf_coder(coder)
            # the same picture without its flat plane first: slot 1's words then hold photo content's stream, far longer than the
            # flat plane's, which is what lies behind that stream's end when it is read with a larger capacity
            ctx.encode_image_tensor(cf.torch_image(synth.make_image("photo", 4200, 72, 8)))
            ctx.sync()
            for visit in range(2):   # the second visit meets the first one's bits in every shared word
                ctx.encode_image_tensor(t)
                ctx.sync()
                blobs[name] = _check_lf_area(ctx, slots, f"{name}, visit {visit}")
    # the slots coded by three growing calls in front of the entropy stage
    with device.DeviceContext(0, 3, 0) as ctx:
        base, w = t.data_ptr(), img.shape[1]
        for visit in range(2):
            ctx.begin_frame(3)
            for s in range(3):
                p = base + s * 2048 * 3
                ctx.encode_lf_group(s, [p, p + 1, p + 2], 3 * w, 3, 0, min(2048, w - s * 2048), img.shape[0], s)
                ctx.submit_lf_group(s)
            for n in (1, 2, 3):
                ctx.run_lf_coder(n, n == 3)
            ctx.finish_frame(3)
            ctx.sync_lf()
            blobs["growing"] = _check_lf_area(ctx, slots, f"three growing calls, visit {visit}")
            ctx.sync()
    assert blobs["in the stream"] == blobs["side stream"] == blobs["growing"]
