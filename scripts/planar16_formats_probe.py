#!/usr/bin/env python3
"""One 3840 x 2160 picture resident in HBM as planar YCbCr of 10-bit codes in 16-bit words (what a software decoder leaves for
10-bit video: yuv420p10le ...) through FrameBatch to finished files in HBM, nine ways: files per second of each.

  i010, i010c, i010l   the three I010 planes read by the transform kernel: nearest, centre-sited, left-sited chroma
  i210, i210c          the picture as I210: nearest, centre-sited
  i410                 the picture as I410
  p010                 i010's picture as P010: the codes shifted left by 6, U and V interleaved (HYDAMD_P010_BT709): i010's file
  rgb16                i010's picture as RGB16 already in HBM (the conversion's own output, made once outside the timing)
  prepass              the I010 planes converted to that RGB16 by a torch pre-pass for every frame, then as rgb16: the only
                       route a caller had before the formats.  The pre-pass is the definition (csrc/hip/hydk_yuvp16.h) in
                       torch int64 arithmetic, into an RGB16 buffer per frame in flight; it runs on torch's stream, and the
                       host waits for a batch's conversions before it hands the batch over.

Same process, same card; the p010, rgb16 and prepass legs code i010's file (checked).  Wall clock around the whole queue, fill
and drain included; `--repeats` timed repeats of each leg after one untimed pass.

    python scripts/planar16_formats_probe.py [--legs i010,rgb16,prepass] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/planar16_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["i010", "i010c", "i010l", "i210", "i210c", "i410", "p010", "rgb16", "prepass"]
PLANAR = {"i010": ("420", None), "i010c": ("420", "centre"), "i010l": ("420", "left"), "i210": ("422", None), "i210c": ("422", "centre"),
          "i410": ("444", None)}
SAME_FILE = ("i010", "p010", "rgb16", "prepass")


def to_rgb16(table, y, u, v, out):
    """the definition (I010, BT.709, limited range, nearest 4:2:0 chroma) as torch elementwise kernels: y (H, W), u and v
    (H / 2, W / 2) of int16 bits -> out (H, W, 3) int16 bits"""
    import torch

    yo, cy, crv, cgu, cgv, cbu = table
    h, w = y.shape
    sample = lambda p: ((p.to(torch.int64) & 0xFFFF) << 6) & 0xFFFF
    luma = (sample(y) - yo) * cy + (1 << 19)
    d, e = (sample(p).repeat_interleave(2, 0).repeat_interleave(2, 1)[:h, :w] - 32768 for p in (u, v))
    for ch, total in enumerate((luma + crv * e, luma - cgu * d - cgv * e, luma + cbu * d)):
        val = (total >> 20).clamp_(0, 65535)
        out[..., ch] = val - ((val >> 15) << 16)  # the uint16 sample's bits in the int16 buffer
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--per-batch", type=int, default=8)
    ap.add_argument("--objects", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import p016_model as pm
    import planar16_model as m16
    import planar_model as plm
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    legs = args.legs.split(",")
    photo = synth.make_image("photo", w, h, 16, 1234)
    pics, host420 = {}, None
    for sub_name, sub in (("420", plm.S420), ("422", plm.S422), ("444", plm.S444)):
        host = m16.planes_of_rgb(photo, 1, 0, sub)
        if sub == plm.S420:
            host420 = host
        planes = [torch.from_numpy(p.view(np.int16)).cuda() for p in host]  # three allocations, pitch = the plane's width
        for leg, (s, chroma) in PLANAR.items():
            if s == sub_name:
                pics[leg] = device.PlanarYuv16(*planes, device.NV12_BT709, s, chroma, 10)
    y, u, v = pics["i010"].y, pics["i010"].u, pics["i010"].v
    ys, us, vs = (m16.samples(1, p) for p in host420)
    surface = torch.from_numpy(np.concatenate([ys.reshape(-1), m16.interleave(us, vs).reshape(-1)]).view(np.int16)).cuda()
    p010 = device.P016.from_surface(surface, w, h, 2 * w, 2 * w * h, device.NV12_BT709, depth=10)
    rgb = torch.from_numpy(m16.expected_rgb(host420, device.I010_BT709).view(np.int16)).cuda()
    ring = []
    if "prepass" in legs:
        assert torch.equal(to_rgb16(pm.TABLE[1, 0], y, u, v, torch.empty_like(rgb)), rgb), "the torch pre-pass is not the model's conversion"
        ring = [torch.empty_like(rgb) for _ in range(G * S)]  # the pre-pass's RGB16 buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' as planar YCbCr of 10-bit codes (BT.709, limited range) resident in "
          f"HBM -> files in HBM; {G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed "
          f"repeats; {torch.cuda.get_device_name(0)}")

    digests = {}
    for leg in legs:
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]

        def batch_of(k, n):
            if leg in pics:
                return [pics[leg]] * n
            if leg == "p010":
                return [p010] * n
            if leg == "rgb16":
                return [rgb] * n
            bufs = ring[k * G: k * G + n]  # (the object's previous batch has been waited for: its buffers are free)
            for b in bufs:
                to_rgb16(pm.TABLE[1, 0], y, u, v, b)
            torch.cuda.current_stream().synchronize()
            return bufs

        def once():
            busy = [False] * S
            for i, grp in enumerate(groups):
                fb = fbs[i % S]
                if busy[i % S]:
                    fb.result()
                fb.encode(batch_of(i % S, len(grp)))
                busy[i % S] = True
            for k in range(S):
                if busy[k]:
                    fbs[k].result()

        once()
        rates = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            rates.append(N / (time.perf_counter() - t0))
        files = fbs[0].read()
        digest = hashlib.md5(bytes(files[0])).hexdigest()[:12]
        same = all(bytes(f) == bytes(files[0]) for f in files)
        if leg in SAME_FILE:
            assert digests.setdefault("i010", digest) == digest, "a p010, rgb16 or pre-pass leg codes another file than i010"
        print(f"{leg:8s} files/s  " + "  ".join(f"{r:7.1f}" for r in rates) +
              f"   median {sorted(rates)[len(rates) // 2]:7.1f}  spread {min(rates):7.1f} .. {max(rates):7.1f}"
              f"   file {len(files[0])} B md5 {digest} all alike {same}  reruns {[fb.overflow_reruns() for fb in fbs]}", flush=True)
        for fb in fbs:
            fb.close()


if __name__ == "__main__":
    main()
