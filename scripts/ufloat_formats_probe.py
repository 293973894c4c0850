#!/usr/bin/env python3
"""One 3840 x 2160 picture resident in HBM as a float render target of one dword a pixel (R11G11B10F: the HDR scene buffer of a
real-time renderer; RGB9E5: shared-exponent HDR textures) through FrameBatch to finished files in HBM, five ways: files per second of
each.

  r11        the surface read by the transform kernel under HYDAMD_R11G11B10F
  e5         the same float32 picture packed as RGB9E5, read under HYDAMD_RGB9E5 (another rounding, so another file)
  f32        r11's widened picture as float32 RGB already in HBM (made once outside the timing) — the yardstick: 12 bytes a pixel
             instead of 4
  f16        r11's widened picture as float16 RGB in HBM (every R11G11B10F value below 65 520 is a float16 value: the same samples,
             6 bytes a pixel)
  prepass    the R11G11B10F surface unpacked to float32 by a torch pre-pass for every frame, then as f32: the route a caller had
             before these formats.  The pre-pass is the header's three rules in torch arithmetic (exact: powers of two by ldexp),
             into a float32 buffer per frame in flight; it runs on torch's stream, and the host waits for a batch's conversions
             before it hands the batch over (FrameBatch has no stream hand-over).

Same process, same card.  Wall clock around the whole queue, fill and drain included; `--repeats` timed repeats of each leg
after one untimed pass.

    python scripts/ufloat_formats_probe.py [--legs r11,f32] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/ufloat_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["r11", "e5", "f32", "f16", "prepass"]


def to_f32(surface, out):
    """the widening of an R11G11B10F surface (H, W) of int32 bits as torch elementwise kernels -> out (H, W, 3) float32; finite
    fields only"""
    import torch

    d = surface.to(torch.int64) & 0xFFFFFFFF
    for c, (shift, mbits) in enumerate(((0, 6), (11, 6), (22, 5))):
        v = (d >> shift) & ((1 << (5 + mbits)) - 1)
        e, m = (v >> mbits).to(torch.int32), (v & ((1 << mbits) - 1)).to(torch.float32)
        normal = torch.ldexp(1.0 + m / float(1 << mbits), e - 15)
        out[..., c] = torch.where(e == 0, m * 2.0 ** (-14 - mbits), normal)
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

    import ufloat_model as um
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    photo = synth.make_image_f32("photo", w, h, 1234)
    host = {"r11": um.pack(photo, um.R11G11B10F), "e5": um.pack(photo, um.RGB9E5)}
    surfaces = {k: torch.from_numpy(v.view(np.int32)).cuda() for k, v in host.items()}  # pitch = the row
    pics = {"r11": device.R11g11b10f(surfaces["r11"], w), "e5": device.Rgb9e5(surfaces["e5"], w)}
    wide = um.expected_f32(host["r11"], um.R11G11B10F)
    f32 = torch.from_numpy(wide).cuda()
    f16 = f32.to(torch.float16)
    assert torch.equal(f16.to(torch.float32), f32), "an R11G11B10F value that is no float16 value"
    assert torch.equal(to_f32(surfaces["r11"], torch.empty_like(f32)), f32), "the torch pre-pass is not the model's widening"
    tensors = {"f32": f32, "f16": f16}
    ring = [torch.empty_like(f32) for _ in range(G * S)]  # the pre-pass's float32 buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' as a float render target of one dword a pixel (R11G11B10F / RGB9E5) "
          f"resident in HBM -> files in HBM; {G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + "
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
                to_f32(surfaces["r11"], b)
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
