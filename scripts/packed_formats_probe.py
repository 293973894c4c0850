#!/usr/bin/env python3
"""One 3840 x 2160 picture resident in HBM as packed 4:2:2 YCbCr (what rocJPEG's native output is for a 4:2:2 JPEG, or a capture
card's frame) through FrameBatch to finished files in HBM, eight ways: files per second of each.

  yuy2, yuy2c, yuy2l   the YUYV surface read by the transform kernel: nearest, centre-sited, left-sited chroma
  uyvy                 the same planes as UYVY, nearest: the same file as yuy2
  i422, i422c          the same planes as three I422 planes: nearest, centre-sited — the yardstick: the same 2 bytes a pixel
                       from three streams instead of one, and the same files as yuy2 and yuy2c
  rgb8                 yuy2's picture as RGB8 already in HBM (the conversion's own output, made once outside the timing)
  prepass              the YUYV surface de-interleaved and converted to RGB8 by a torch pre-pass for every frame, then as rgb8:
                       the only route a caller had before the packed formats, short of asking the decoder for another output.
                       The pre-pass is the same fixed-point formula in torch int32 arithmetic, into an RGB buffer per frame in
                       flight; it runs on torch's stream, and the host waits for a batch's conversions before it hands the batch
                       over (FrameBatch has no stream hand-over).

Same process, same card.  Wall clock around the whole queue, fill and drain included; `--repeats` timed repeats of each leg
after one untimed pass.

    python scripts/packed_formats_probe.py [--legs yuy2,i422,rgb8] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/packed_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["yuy2", "yuy2c", "yuy2l", "uyvy", "i422", "i422c", "rgb8", "prepass"]
PACKED = {"yuy2": ("yuyv", None), "yuy2c": ("yuyv", "centre"), "yuy2l": ("yuyv", "left"), "uyvy": ("uyvy", None)}
PLANAR = {"i422": None, "i422c": "centre"}
BT709 = (16, 19077, 29372, 3494, 8731, 34610)  # yo, cy, crv, cgu, cgv, cbu (csrc/hip/hydk_yuv.h)


def to_rgb8(surface, w, out):
    """the conversion (BT.709, limited range, nearest chroma) of a YUYV surface (H, 2 W) as torch elementwise kernels -> out (H, W, 3)"""
    import torch

    yo, cy, crv, cgu, cgv, cbu = BT709
    c = (surface[:, 0::2][:, :w].to(torch.int32) - yo) * cy + 8192
    d, e = (surface[:, k::4].repeat_interleave(2, 1)[:, :w].to(torch.int32) - 128 for k in (1, 3))
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

    import torch

    import packed_model as pkm
    import planar_model as plm
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    photo = synth.make_image("photo", w, h, 8, 1234)
    planes = plm.planes_of_rgb(photo, 0, plm.S422)
    surfaces = {order: torch.from_numpy(pkm.interleave(planes, order, w)).cuda() for order in ("yuyv", "uyvy")}  # pitch = the row
    pics = {leg: device.PackedYuv(surfaces[order], w, device.NV12_BT709, order, chroma) for leg, (order, chroma) in PACKED.items()}
    dev_planes = [torch.from_numpy(p).cuda() for p in planes]  # three allocations, pitch = the plane's width
    for leg, chroma in PLANAR.items():
        pics[leg] = device.PlanarYuv(*dev_planes, device.NV12_BT709, "422", chroma)
    rgb = torch.from_numpy(pkm.expected_rgb(pkm.interleave(planes, "yuyv", w), "yuyv", w, 0, 0)).cuda()
    assert torch.equal(to_rgb8(surfaces["yuyv"], w, torch.empty_like(rgb)), rgb), "the torch pre-pass is not the model's conversion"
    ring = [torch.empty_like(rgb) for _ in range(G * S)]  # the pre-pass's RGB buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' as packed 4:2:2 YCbCr (BT.709, limited range) resident in HBM -> files in HBM; "
          f"{G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    for leg in args.legs.split(","):
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]

        def batch_of(k, n):
            if leg in pics:
                return [pics[leg]] * n
            if leg == "rgb8":
                return [rgb] * n
            bufs = ring[k * G: k * G + n]  # (the object's previous batch has been waited for: its buffers are free)
            for b in bufs:
                to_rgb8(surfaces["yuyv"], w, b)
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
