#!/usr/bin/env python3
"""One 3840 x 2160 picture resident in HBM with one dword of three 10-bit fields a pixel (RGB10A2: a Vulkan or DRM render target;
Y410: what a VA-API or D3D decoder leaves for 4:4:4 10-bit HEVC) through FrameBatch to finished files in HBM, seven ways: files per
second of each.

  rgb10, bgr10   the surface read by the transform kernel under HYDAMD_RGB10A2 and, the fields in the other order, HYDAMD_BGR10A2:
                 the same picture, so the same file
  rgb16          rgb10's picture as RGB16 already in HBM (the widening's own output, made once outside the timing) — the yardstick: 6
                 bytes a pixel instead of 4
  prepass        the RGB10A2 surface unpacked to RGB16 by a torch pre-pass for every frame, then as rgb16: the route a caller had
                 before these formats.  The pre-pass is the same integer formula in torch int64 arithmetic, into an RGB buffer per
                 frame in flight; it runs on torch's stream, and the host waits for a batch's conversions before it hands the batch
                 over (FrameBatch has no stream hand-over).
  y410           a Y410 surface (BT.709, limited range) read by the transform kernel
  i410           the same samples as three I410 planes — the yardstick: 6 bytes a pixel from three streams, and the same file as y410
  y410rgb16      y410's picture as RGB16 already in HBM

Same process, same card.  Wall clock around the whole queue, fill and drain included; `--repeats` timed repeats of each leg
after one untimed pass.

    python scripts/dword_formats_probe.py [--legs rgb10,rgb16] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/dword_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["rgb10", "bgr10", "rgb16", "prepass", "y410", "i410", "y410rgb16"]


def to_rgb16(surface, out):
    """the widening of an RGB10A2 surface (H, W) of int32 bits as torch elementwise kernels -> out (H, W, 3) int16 bits"""
    import torch

    d = surface.to(torch.int64) & 0xFFFFFFFF
    for c in range(3):
        out[..., c] = (((d >> (10 * c)) & 1023) * 65535 + 511) // 1023
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

    import dword_model as dm
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    photo = synth.make_image("photo", w, h, 16, 1234)
    photo = photo.cpu().numpy() if hasattr(photo, "cpu") else np.asarray(photo)
    photo = photo.view(np.uint16)
    host = {"rgb10": dm.surface_of_rgb(photo, dm.RGB10A2), "bgr10": dm.surface_of_rgb(photo, dm.BGR10A2), "y410": dm.surface_of_rgb(photo, dm.Y410[0])}
    surfaces = {k: torch.from_numpy(v.view(np.int32)).cuda() for k, v in host.items()}  # pitch = the row
    pics = {"rgb10": device.Rgb10(surfaces["rgb10"], w, "rgb"), "bgr10": device.Rgb10(surfaces["bgr10"], w, "bgr"),
            "y410": device.Y410(surfaces["y410"], w, device.NV12_BT709)}
    dev_planes = [torch.from_numpy(p.view(np.int16)).cuda() for p in dm.y410_planes(host["y410"])]  # three allocations, chroma pitch = the width
    pics["i410"] = device.PlanarYuv16(*dev_planes, device.NV12_BT709, "444", None, 10)
    rgb = torch.from_numpy(dm.expected_rgb(host["rgb10"], dm.RGB10A2).view(np.int16)).cuda()
    assert np.array_equal(dm.expected_rgb(host["rgb10"], dm.RGB10A2), dm.expected_rgb(host["bgr10"], dm.BGR10A2))
    assert torch.equal(to_rgb16(surfaces["rgb10"], torch.empty_like(rgb)), rgb), "the torch pre-pass is not the model's widening"
    tensors = {"rgb16": rgb, "y410rgb16": torch.from_numpy(dm.expected_rgb(host["y410"], dm.Y410[0]).view(np.int16)).cuda()}
    ring = [torch.empty_like(rgb) for _ in range(G * S)]  # the pre-pass's RGB buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' with one dword of three 10-bit fields a pixel (RGB10A2 / BGR10A2 / Y410, BT.709 "
          f"limited range) resident in HBM -> files in HBM; {G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + "
          f"{args.repeats} timed repeats; {torch.cuda.get_device_name(0)}")

    for leg in args.legs.split(","):
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]

        def batch_of(k, n):
            if leg in pics:
                return [pics[leg]] * n
            if leg in tensors:
                return [tensors[leg]] * n
            bufs = ring[k * G: k * G + n]  # (the object's previous batch has been waited for: its buffers are free)
            for b in bufs:
                to_rgb16(surfaces["rgb10"], b)
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
        print(f"{leg:9s} files/s  " + "  ".join(f"{r:7.1f}" for r in rates) +
              f"   median {sorted(rates)[len(rates) // 2]:7.1f}  spread {min(rates):7.1f} .. {max(rates):7.1f}"
              f"   file {len(files[0])} B md5 {digest} all alike {same}  reruns {[fb.overflow_reruns() for fb in fbs]}", flush=True)
        for fb in fbs:
            fb.close()


if __name__ == "__main__":
    main()
