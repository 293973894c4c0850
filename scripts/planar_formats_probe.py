#!/usr/bin/env python3
"""One 3840 x 2160 picture resident in HBM as planar YCbCr (what rocJPEG's planar output or a software decoder leaves) through
FrameBatch to finished files in HBM, nine ways: files per second of each.

  i420, i420c, i420l   the three I420 planes read by the transform kernel: nearest, centre-sited, left-sited chroma
  i422, i422c          the picture as I422: nearest, centre-sited
  i444                 the picture as I444
  nv12                 i420's picture with U and V interleaved (HYDAMD_NV12_BT709): the same file as i420
  rgb8                 i420's picture as RGB8 already in HBM (the conversion's own output, made once outside the timing)
  prepass              the I420 planes converted to RGB8 by a torch pre-pass for every frame, then as rgb8: the only route a
                       caller had before the planar formats.  The pre-pass is the same fixed-point formula in torch int32
                       arithmetic, into an RGB buffer per frame in flight; it runs on torch's stream, and the host waits for a
                       batch's conversions before it hands the batch over (FrameBatch has no stream hand-over).

Same process, same card.  Wall clock around the whole queue, fill and drain included; `--repeats` timed repeats of each leg
after one untimed pass.

    python scripts/planar_formats_probe.py [--legs i420,rgb8,prepass] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/planar_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["i420", "i420c", "i420l", "i422", "i422c", "i444", "nv12", "rgb8", "prepass"]
PLANAR = {"i420": ("420", None), "i420c": ("420", "centre"), "i420l": ("420", "left"), "i422": ("422", None), "i422c": ("422", "centre"),
          "i444": ("444", None)}
BT709 = (16, 19077, 29372, 3494, 8731, 34610)  # yo, cy, crv, cgu, cgv, cbu (csrc/hip/hydk_yuv.h)


def to_rgb8(y, u, v, out):
    """the conversion (BT.709, limited range, nearest 4:2:0 chroma) as torch elementwise kernels: y (H, W), u and v (H/2, W/2) -> out (H, W, 3)"""
    import torch

    yo, cy, crv, cgu, cgv, cbu = BT709
    h, w = y.shape
    c = (y.to(torch.int32) - yo) * cy + 8192
    d, e = (p.repeat_interleave(2, 0).repeat_interleave(2, 1)[:h, :w].to(torch.int32) - 128 for p in (u, v))
    out[..., 0] = ((c + crv * e) >> 14).clamp_(0, 255)
    out[..., 1] = ((c - cgu * d - cgv * e) >> 14).clamp_(0, 255)
    out[..., 2] = ((c + cbu * d) >> 14).clamp_(0, 255)
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

    import planar_model as plm
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    photo = synth.make_image("photo", w, h, 8, 1234)
    pics = {}
    for sub_name, sub in (("420", plm.S420), ("422", plm.S422), ("444", plm.S444)):
        planes = [torch.from_numpy(p).cuda() for p in plm.planes_of_rgb(photo, 0, sub)]  # three allocations, pitch = the plane's width
        for leg, (s, chroma) in PLANAR.items():
            if s == sub_name:
                pics[leg] = device.PlanarYuv(*planes, device.NV12_BT709, s, chroma)
    y, u, v = pics["i420"].y, pics["i420"].u, pics["i420"].v
    nv12 = device.Nv12(y, torch.stack([u, v], -1).contiguous(), device.NV12_BT709)
    rgb = torch.from_numpy(plm.expected_rgb([p.cpu().numpy() for p in (y, u, v)], 0, plm.S420, 0)).cuda()
    assert torch.equal(to_rgb8(y, u, v, torch.empty_like(rgb)), rgb), "the torch pre-pass is not the model's conversion"
    ring = [torch.empty_like(rgb) for _ in range(G * S)]  # the pre-pass's RGB buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' as planar YCbCr (BT.709, limited range) resident in HBM -> files in HBM; "
          f"{G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    for leg in args.legs.split(","):
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]

        def batch_of(k, n):
            if leg in pics:
                return [pics[leg]] * n
            if leg == "nv12":
                return [nv12] * n
            if leg == "rgb8":
                return [rgb] * n
            bufs = ring[k * G: k * G + n]  # (the object's previous batch has been waited for: its buffers are free)
            for b in bufs:
                to_rgb8(y, u, v, b)
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
        print(f"{leg:8s} files/s  " + "  ".join(f"{r:7.1f}" for r in rates) +
              f"   median {sorted(rates)[len(rates) // 2]:7.1f}  spread {min(rates):7.1f} .. {max(rates):7.1f}"
              f"   file {len(files[0])} B md5 {digest} all alike {same}  reruns {[fb.overflow_reruns() for fb in fbs]}", flush=True)
        for fb in fbs:
            fb.close()


if __name__ == "__main__":
    main()
