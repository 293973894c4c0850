"""Frames for tests/test_gpu_fused_launches.py, what the CPU oracle and the LF model say about them, the checks a coded frame
has to pass, and the child process of the tests that need an environment setting read once per process
(python tests/fused_frames.py MODE CASE EXPECTATION.npz REPORT.json).

The frame loop's token workgroups ride in the table kernel's launch and its pack workgroups in the emit kernel's, where they
write the packed LF area at once.  What the role arithmetic can get wrong depends on how many windows of 896 values each
slot of a launch has (the riders of a launch are counted ceil(220 / HYDK_LF_WPB) per slot whatever the slot holds), on the
slots' bit counts (a slot's place is the sum of the words of those in front) and on what an earlier frame left in the
area: the cases hold one window, two windows with the second holding one value, 220 windows, slots of different window
counts in one launch, and six slots of two frames."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hydrium_amd import synth  # noqa: E402

import closing_frames as cf  # noqa: E402

BEYOND = 64   # bytes asked of read_lf_bits beyond a slot's stream
WINDOW = 896  # values a token / pack workgroup decides (lf_huffman.h kEmitSpan)


def lf_frame(seed=1234, flat=77):
    """4200 x 72 RGB8, three LF groups in a row: photo content, a flat plane (its stream is runs of one value), a narrow rest"""
    img = synth.make_image("photo", 4200, 72, 8, seed).copy()
    img[:, 2048:4096] = flat
    return img


# name -> the pictures of one launch group (one: a frame; two: a batch of two frames of one shape)
CASES = {
    "8x8": lambda: [synth.make_image("photo", 8, 8, 8)],                 # 3 values: one window
    "104x184": lambda: [synth.make_image("photo", 104, 184, 8)],         # 13 x 23 blocks, 897 values: the second window holds one
    "4200x72": lambda: [lf_frame()],                                     # three slots: 6 912, 6 912 and 351 values
    "2048x2048": lambda: [synth.make_image("photo", 2048, 2048, 8)],     # 196 608 values: all 220 windows
    "batch_4200x72": lambda: [lf_frame(), lf_frame(seed=99, flat=200)],  # six slots, offsets running across the frame boundary
}
# what is coded between two visits of a case on one context: slot 1 (and every other) then holds photo content's stream, far
# longer than the flat plane's and than the small frames', so stale words lie behind the short ones
LONG = lambda n: [synth.make_image("photo", 4200, 72, 8, seed=7 + k) for k in range(n)]  # noqa: E731


def windows_of(img):
    h, w, _ = img.shape
    return [-(-(3 * -(-min(2048, w - x) // 8) * -(-min(2048, h - y) // 8)) // WINDOW) for y in range(0, h, 2048) for x in range(0, w, 2048)]


def expectation(images):
    """What the oracle (closing_frames.oracle_frame) and the LF model (lf_model.model on the oracle's LF ints) say about a
    launch group: payload, section bits, offsets[] (running across the frames), and per slot the LF stream and its bit count."""
    from tests import lf_model

    payload, bits, offs, lf = b"", [], [], []
    for img in images:
        p, b, o = cf.oracle_frame(img)
        bits.append(b)
        offs.append(o + len(payload))
        payload += p
        h, w, _ = img.shape
        mx = 0
        for ty in range(-(-h // 2048)):
            for tx in range(-(-w // 2048)):
                res, mx = cf.orc.encode_lf_group(np.ascontiguousarray(img), tx, ty, max_alphabet_size=mx)
                _, _, _, _, sbits, nbits = lf_model.model(res.dc)
                lf.append((np.asarray(sbits[:(nbits + 7) // 8], np.uint8), int(nbits)))
    return {"payload": payload, "bits": np.concatenate(bits), "offs": np.concatenate(offs), "lf": lf}


def save_expectation(path, exp):
    arrays = {"payload": np.frombuffer(exp["payload"], np.uint8), "bits": exp["bits"], "offs": exp["offs"],
              "lf_nbits": np.array([n for _, n in exp["lf"]], np.int64)}
    for s, (b, _) in enumerate(exp["lf"]):
        arrays[f"lf_{s}"] = b
    np.savez(path, **arrays)


def load_expectation(path):
    z = np.load(path)
    return {"payload": z["payload"].tobytes(), "bits": z["bits"], "offs": z["offs"],
            "lf": [(z[f"lf_{s}"], int(n)) for s, n in enumerate(z["lf_nbits"])]}


def enqueue(ctx, tensors):
    if len(tensors) == 1:
        ctx.encode_image_tensor(tensors[0])
    else:
        ctx.encode_image_batch(tensors)


def check_sections(ctx, exp, where):
    slots = len(exp["lf"])
    assert ctx.payload_size() == len(exp["payload"]), f"{where}: total"
    pairs = [ctx.read_sections(s) for s in range(slots)]
    assert np.array_equal(np.concatenate([p[0] for p in pairs]), exp["bits"]), f"{where}: section bits"
    assert np.array_equal(np.concatenate([p[1] for p in pairs]), exp["offs"]), f"{where}: offsets[]"
    assert ctx.read_payload() == exp["payload"], f"{where}: payload"


def check_lf_area(ctx, exp, where):
    """The packed LF area is the slots' streams of the model back to back at 4-byte alignment, zero between a stream's end
    and the next slot; read_lf_bits gives a slot's slice and zero beyond it.  Returns the area's bytes."""
    slots = exp["lf"]
    info, blob = ctx.read_lf_streams(len(slots)), ctx.read_lf_payload().copy()
    end = 0
    for s, (bits, nbits) in enumerate(slots):
        assert int(info["error"][s]) == 0 and int(info["bit_count"][s]) == nbits, f"{where}: slot {s} bit count"
        off, nbytes = int(info["offset"][s]), (nbits + 7) // 8
        assert off == end and off % 4 == 0, f"{where}: slot {s} starts at {off}, the slots before it end at {end}"
        got = blob[off:off + nbytes].copy()
        if nbits % 8:   # the model leaves the last byte's spare bits zero; so does the device
            assert got[-1] >> (nbits % 8) == 0, f"{where}: slot {s}: bits behind the stream's end in its last byte"
        assert np.array_equal(got, bits), f"{where}: slot {s} differs from the model"
        end = off + (nbits + 31) // 32 * 4
        assert not blob[off + nbytes:end].any(), f"{where}: slot {s}: bytes between the stream's end and the next slot"
        assert np.array_equal(ctx.read_lf_bits(s, nbits), got), f"{where}: read_lf_bits({s}) is not the slot's slice"
        more = ctx.read_lf_bits(s, nbits + 8 * BEYOND)   # a capacity beyond the stream's end: the slice, then zero
        assert len(more) == nbytes + BEYOND and np.array_equal(more[:nbytes], got), f"{where}: read_lf_bits({s}), larger capacity"
        assert not more[nbytes:].any(), f"{where}: read_lf_bits({s}): bytes beyond the stream's end are not zero"
    assert end == len(blob) == ctx.lf_payload_size(), f"{where}: the LF payload is {len(blob)} bytes, the slots end at {end}"
    return blob.tobytes()


def visit_twice(ctx, images, exp, where):
    """The launch group coded, a launch group of longer LF streams in every slot, the launch group again; checked both times."""
    tensors = [cf.torch_image(i) for i in images]
    long_ones = [cf.torch_image(i) for i in LONG(len(images))]
    blob = None
    for visit in range(2):
        enqueue(ctx, tensors)
        ctx.sync()
        check_sections(ctx, exp, f"{where}, visit {visit}")
        again = check_lf_area(ctx, exp, f"{where}, visit {visit}")
        assert blob in (None, again)
        blob = again
        if visit == 0:
            enqueue(ctx, long_ones)
            ctx.sync()
    return blob


def child(mode, case, exp_path, report_path):
    """mode "visit": the case visited twice on an in-stream context under whatever HYDAMD_* settings the parent gave this
    process.  mode "payload": the case with the payload sized to exactly its section bytes, and one byte short (one rerun)."""
    from hydrium_amd import device

    images, exp = CASES[case](), load_expectation(exp_path)
    report = {"runs": {}}

    def leave():
        with open(report_path, "w") as f:
            json.dump(report, f)

    try:
        if mode == "visit":
            with device.DeviceContext(0, max(3, len(exp["lf"])), 0) as ctx:
                ctx.set_lf_coder(2)
                blob = visit_twice(ctx, images, exp, case)
                report["runs"]["visit"] = {"lf_md5": hashlib.md5(blob).hexdigest(), "reruns": ctx.overflow_reruns()}
        else:
            tensors = [cf.torch_image(i) for i in images]
            for name, cap in (("exact", len(exp["payload"])), ("short", len(exp["payload"]) - 1)):
                print(f"CASE {name}: HYDAMD_PAYLOAD_CAP {cap}", flush=True)
                os.environ["HYDAMD_PAYLOAD_CAP"] = str(cap)
                with device.DeviceContext(0, len(exp["lf"]), 0) as ctx:
                    ctx.set_lf_coder(2)
                    enqueue(ctx, tensors)
                    ctx.sync()
                    check_sections(ctx, exp, name)
                    blob = check_lf_area(ctx, exp, name)
                    report["runs"][name] = {"lf_md5": hashlib.md5(blob).hexdigest(), "reruns": ctx.overflow_reruns()}
                leave()
    except AssertionError as e:
        report["error"] = str(e)
        leave()
        return 1
    report["done"] = True
    leave()
    return 0


if __name__ == "__main__":
    sys.exit(child(*sys.argv[1:5]))
