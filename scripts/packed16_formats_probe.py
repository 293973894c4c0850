#!/usr/bin/env python3
"""One 3840 x 2160 picture resident in HBM as packed 4:2:2 YCbCr of 16-bit words (Y210: what a VA-API or D3D decoder leaves for
4:2:2 10-bit HEVC, ffmpeg's y210le) through FrameBatch to finished files in HBM, eight ways: files per second of each.

  y210, y210c, y210l   the Y210 surface read by the transform kernel: nearest, centre-sited, left-sited chroma
  y216                 the same words under HYDAMD_Y216_BT709, nearest: limited range, so the same file as y210
  i210, i210c          the same samples as three I210 planes (the words >> 6): nearest, centre-sited — the yardstick: the same 4
                       bytes a pixel from three streams instead of one, and the same files as y210 and y210c
  rgb16                y210's picture as RGB16 already in HBM (the conversion's own output, made once outside the timing)
  prepass              the Y210 surface de-interleaved and converted to RGB16 by a torch pre-pass for every frame, then as rgb16:
                       the route a caller had before the packed formats.  The pre-pass is the same fixed-point formula in torch
                       int64 arithmetic, into an RGB buffer per frame in flight; it runs on torch's stream, and the host waits
                       for a batch's conversions before it hands the batch over (FrameBatch has no stream hand-over).

Same process, same card.  Wall clock around the whole queue, fill and drain included; `--repeats` timed repeats of each leg
after one untimed pass.

    python scripts/packed16_formats_probe.py [--legs y210,i210,rgb16] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/packed16_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["y210", "y210c", "y210l", "y216", "i210", "i210c", "rgb16", "prepass"]
PACKED = {"y210": (None, 10), "y210c": ("centre", 10), "y210l": ("left", 10), "y216": (None, 16)}
PLANAR = {"i210": None, "i210c": "centre"}
BT709 = (4096, 1225714, 1887168, 224481, 560979, 2223666)  # yo, cy, crv, cgu, cgv, cbu at 2^20 (csrc/hip/hydk_yuv16.h, limited range)


def to_rgb16(surface, w, out):
    """the conversion (BT.709, limited range, nearest chroma) of a Y210 surface (H, 2 W) of int16 bits as torch elementwise kernels
    -> out (H, W, 3) int16 bits"""
    import torch

    yo, cy, crv, cgu, cgv, cbu = BT709
    word = lambda t: (t.to(torch.int32) & 0xFFFF).to(torch.int64)
    c = (word(surface[:, 0::2][:, :w]) - yo) * cy + (1 << 19)
    d, e = (word(surface[:, k::4]).repeat_interleave(2, 1)[:, :w] - 32768 for k in (1, 3))
    out[..., 0] = ((c + crv * e) >> 20).clamp_(0, 65535)
    out[..., 1] = ((c - cgu * d - cgv * e) >> 20).clamp_(0, 65535)
    out[..., 2] = ((c + cbu * d) >> 20).clamp_(0, 65535)
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

    import packed16_model as p6
    import planar16_model as m16
    import planar_model as plm
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    photo = synth.make_image("photo", w, h, 16, 1234)
    photo = photo.cpu().numpy() if hasattr(photo, "cpu") else np.asarray(photo)
    planes = m16.planes_of_rgb(photo.view(np.uint16), 1, 0, plm.S422)  # valid 10-bit codes, LSB-aligned: I210
    rows = p6.interleave(tuple(p << 6 for p in planes), "yuyv", w)  # MSB-aligned: Y210, pitch = the row
    surface = torch.from_numpy(rows.view(np.int16)).cuda()
    pics = {leg: device.PackedYuv16(surface, w, device.NV12_BT709, "yuyv", chroma, depth) for leg, (chroma, depth) in PACKED.items()}
    dev_planes = [torch.from_numpy(p.view(np.int16)).cuda() for p in planes]  # three allocations, pitch = the plane's width
    for leg, chroma in PLANAR.items():
        pics[leg] = device.PlanarYuv16(*dev_planes, device.NV12_BT709, "422", chroma, 10)
    rgb = torch.from_numpy(p6.expected_rgb(rows, "yuyv", w, p6.sample_fmt(0, 0, 1)).view(np.int16)).cuda()
    assert torch.equal(to_rgb16(surface, w, torch.empty_like(rgb)), rgb), "the torch pre-pass is not the model's conversion"
    ring = [torch.empty_like(rgb) for _ in range(G * S)]  # the pre-pass's RGB buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' as packed 4:2:2 YCbCr of 16-bit words (Y210, BT.709, limited range) resident in HBM "
          f"-> files in HBM; {G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    for leg in args.legs.split(","):
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]

        def batch_of(k, n):
            if leg in pics:
                return [pics[leg]] * n
            if leg == "rgb16":
                return [rgb] * n
            bufs = ring[k * G: k * G + n]  # (the object's previous batch has been waited for: its buffers are free)
            for b in bufs:
                to_rgb16(surface, w, b)
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
