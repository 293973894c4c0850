"""The process tests/test_gpu_stream_classes.py starts once per environment (the runtime reads GPU_MAX_HW_QUEUES, the library
HYDAMD_STREAM_HIGH, once per process).  usage: stream_class_client.py classes N | rounds N K | reuse
Prints `classes <c0> <c1> ...` and, where it compared bytes, `same <what>` lines; any difference is an assertion."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hydrium_amd import api, device, synth

W, H, FPL = 520, 264, 2  # one LF group of 3 x 2 groups, ragged on the right and below; two frames = one launch group


def make(n, slots=FPL):
    ctxs = [device.DeviceContext(0, slots, 0) for _ in range(n)]
    for c in ctxs:
        c.set_rans_waves(5)  # the lane form with the LF coder in the context's own stream: the loop's six launches
        c.set_lf_coder(2)
    return ctxs


def results(c):
    return (c.read_payload(), [c.read_sections(s)[0].tobytes() for s in range(FPL)], c.read_lf_streams(FPL).tobytes(),
            c.read_lf_payload().tobytes())


def expected_file(img):
    from test_gpu_api_parity import _expected

    return _expected(img)[0]


def context_file(ctx, img):
    """the file of the one-LF-group picture a context codes (as tests/test_gpu_chroma_filters.py builds it)"""
    h, w, _ = img.shape
    ctx.encode_image_tensor(torch.from_numpy(img).cuda())
    full = torch.zeros(ctx.blob_bound(1), dtype=torch.uint8, device="cuda")
    ctx.export_frame(1, full)
    ctx.sync()
    head = device.blob_header(full[:64].cpu().numpy().tobytes())
    return device.frame_from_blobs(api.HYDImageMetadata(w, h, 0, -1, -1), [full[: int(head["total_bytes"])].cpu().numpy().tobytes()])


def rounds(n, checked):
    ctxs = make(n)
    print("classes", *[c.stream_class() for c in ctxs], flush=True)
    dev = torch.device("cuda", 0)
    pics = {k: [synth.make_image("photo", W, H, 16, seed=100 + FPL * k + f, device=dev) for f in range(FPL)] for k in range(n)}
    torch.cuda.synchronize()
    want = {}
    for k in checked:  # the same two pictures alone on context 0
        ctxs[0].encode_image_batch(pics[k])
        ctxs[0].sync()
        want[k] = results(ctxs[0])
    assert len({w[0] for w in want.values()}) == len(want)  # pictures of their own
    for _ in range(3):
        for k, c in enumerate(ctxs):
            c.encode_image_batch(pics[k])
    for c in ctxs:
        c.sync()
    for k in checked:
        got = results(ctxs[k])
        for name, a, b in zip(("payload", "section sizes", "LF stream records", "LF streams"), got, want[k]):
            assert a == b, f"context {k} (class {ctxs[k].stream_class()}): {name} differ from the same pictures coded alone"
    print("same sections", len(checked), flush=True)
    img = synth.make_image("photo", W, H, 16, seed=100)
    assert api.encode_image(api.Library(), img) == expected_file(img), "drop-in API file differs from the reference's"
    print("same file", flush=True)
    for c in ctxs:
        c.close()


def reuse():
    ctxs = make(6, 1)
    before = [c.stream_class() for c in ctxs]
    ctxs[4].close()
    ctxs[4] = make(1, 1)[0]
    print("classes", *before, ctxs[4].stream_class(), flush=True)
    c = ctxs[4]
    c.set_rans_waves(4)  # wave form, LF coder on the side stream: created on first use, in its context's pool
    c.set_lf_coder(1)
    img = synth.make_image("photo", 264, 200, 8, seed=77)
    assert context_file(c, img) == expected_file(img), "file of a context with an LF side stream differs from the reference's"
    print("same file", flush=True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "classes":
        ctxs = make(int(sys.argv[2]))
        print("classes", *[c.stream_class() for c in ctxs], flush=True)
        for c in ctxs:
            c.close()
    elif mode == "rounds":
        n, k = int(sys.argv[2]), int(sys.argv[3])
        rounds(n, list(range(n)) if k >= n else [0, n - 1][:k])
    else:
        reuse()
