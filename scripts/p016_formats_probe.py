#!/usr/bin/env python3
"""One 3840 x 2160 P010 picture resident in HBM (what a hardware decoder leaves for 10-bit video) through FrameBatch to
finished files in HBM, read by the transform kernel as it is, and by the routes a caller had before the formats existed:
files per second of each.

  nearest          HYDAMD_P010_BT709: every 2 x 2 block shares its chroma pair
  centre           HYDAMD_P010C_BT709: centre-sited chroma interpolated by the transform kernel
  left             HYDAMD_P010L_BT709: left-sited chroma interpolated by the transform kernel
  rgb16            the nearest leg's picture already converted to RGB16 in HBM (6 bytes a pixel instead of 3): what the
                   conversion costs the kernel
  prepass-nearest  the planes converted to RGB16 by a torch pre-pass for every frame, then coded as RGB16: the same integers
  prepass-left     (csrc/hip/hydk_yuv16.h, hydk_chroma.h) as torch int64 kernels into an RGB16 buffer per frame in flight;
                   torch's stream, and the host waits for a batch's conversions before it hands the batch over

Same process, same card; the rgb16 and prepass legs code the file their format's leg codes (checked).  Wall clock around the
whole queue, fill and drain included; `--repeats` timed repeats of each leg after one untimed pass.

    python scripts/p016_formats_probe.py [--legs nearest,centre,left,rgb16,prepass-nearest,prepass-left] [--frames 256]
                                         [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/p016_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["nearest", "centre", "left", "rgb16", "prepass-nearest", "prepass-left"]
FILTER = {"nearest": 0, "centre": 1, "left": 2}


class Prepass:
    """the formats' definition (P010, BT.709, limited range) as torch kernels: y (H, W), uv (ch, cw, 2) int16 bits -> out (H, W, 3)"""

    def __init__(self, filt, w, h, dev, table):
        import torch

        ch, cw = (h + 1) // 2, (w + 1) // 2
        y, x = torch.arange(h, device=dev), torch.arange(w, device=dev)
        self.filt, self.odd, self.table = filt, (x & 1).bool()[None, :, None], table
        self.cy, self.cx = y >> 1, x >> 1
        self.vy = (self.cy + torch.where((y & 1) == 1, 1, -1)).clamp_(0, ch - 1)
        self.hx = (self.cx + torch.where((x & 1) == 1, 1, -1 if filt == 1 else 0)).clamp_(0, cw - 1)

    def __call__(self, y, uv, out):
        import torch

        yo, cy, crv, cgu, cgv, cbu = self.table
        c = uv.to(torch.int64) & 0xFFFF
        if self.filt == 0:
            up = c.index_select(0, self.cy).index_select(1, self.cx)
        else:
            vmix = 3 * c.index_select(0, self.cy) + c.index_select(0, self.vy)  # (H, cw, 2)
            v0, v1 = vmix.index_select(1, self.cx), vmix.index_select(1, self.hx)
            if self.filt == 1:
                up = (3 * v0 + v1 + 8) >> 4
            else:
                up = torch.where(self.odd, (v0 + v1 + 4) >> 3, (v0 + 2) >> 2)
        d, e = up[..., 0] - 32768, up[..., 1] - 32768
        luma = ((y.to(torch.int64) & 0xFFFF) - yo) * cy + (1 << 19)
        for ch, total in enumerate((luma + crv * e, luma - cgu * d - cgv * e, luma + cbu * d)):
            v = (total >> 20).clamp_(0, 65535)
            out[..., ch] = v - ((v >> 15) << 16)  # the uint16 sample's bits in the int16 buffer
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
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    y, uv = pm.p016_of_rgb(synth.make_image("photo", w, h, 16, 1234), 1, 0)
    words = np.concatenate([y.reshape(-1), uv.reshape(-1)]).view(np.int16)
    surface = torch.from_numpy(words).cuda()  # pitch 3840 words: one allocation, as a decoder's
    pics = {name: device.P016.from_surface(surface, w, h, 2 * w, 2 * w * h, device.NV12_BT709, chroma=name, depth=10) for name in FILTER}
    legs = args.legs.split(",")
    prepass, models = {}, {}
    for name in sorted({leg.rpartition("-")[2] for leg in legs if leg.startswith("prepass")} | ({"nearest"} if "rgb16" in legs else set())):
        models[name] = torch.from_numpy(pm.expected_rgb((y, uv), pics[name].sample_fmt).view(np.int16)).cuda()
        prepass[name] = Prepass(FILTER[name], w, h, surface.device, pm.TABLE[1, 0])
        assert torch.equal(prepass[name](pics[name].y, pics[name].uv, torch.empty_like(models[name])), models[name]), "the torch pre-pass is not the model"
    ring = []
    if any(leg.startswith("prepass") for leg in legs):
        ring = [torch.empty((h, w, 3), dtype=torch.int16, device=surface.device) for _ in range(G * S)]  # an RGB16 buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' as P010 (BT.709, limited range) resident in HBM -> files in HBM; "
          f"{G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    digests = {}
    for leg in legs:
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]
        name = "nearest" if leg == "rgb16" else leg.rpartition("-")[2]

        def batch_of(k, n):
            if leg == "rgb16":
                return [models["nearest"]] * n
            if not leg.startswith("prepass"):
                return [pics[leg]] * n
            bufs = ring[k * G: k * G + n]  # (the object's previous batch has been waited for: its buffers are free)
            for b in bufs:
                prepass[name](pics[name].y, pics[name].uv, b)
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
        assert digests.setdefault(name, digest) == digest, "an rgb16 or pre-pass leg codes another file than its format's leg"
        print(f"{leg:15s} files/s  " + "  ".join(f"{r:7.1f}" for r in rates) +
              f"   median {sorted(rates)[len(rates) // 2]:7.1f}  spread {min(rates):7.1f} .. {max(rates):7.1f}"
              f"   file {len(files[0])} B md5 {digest} all alike {same}  reruns {[fb.overflow_reruns() for fb in fbs]}")
        for fb in fbs:
            fb.close()


if __name__ == "__main__":
    main()
