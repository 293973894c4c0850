#!/usr/bin/env python3
"""One 3840 x 2160 NV12 picture resident in HBM (what a hardware decoder leaves) through FrameBatch to finished files in HBM
under each chroma filter, and by the route a caller had before the interpolating formats: files per second of each.

  nearest          HYDAMD_NV12_BT709: every 2 x 2 block shares its chroma pair
  centre           HYDAMD_NV12C_BT709: centre-sited chroma interpolated by the transform kernel
  left             HYDAMD_NV12L_BT709: left-sited chroma interpolated by the transform kernel
  prepass-centre   the planes interpolated and converted to RGB8 by a torch pre-pass for every frame, then coded as RGB8: the
  prepass-left     same integers (csrc/hip/hydk_chroma.h, hydk_yuv.h) as torch int32 kernels into an RGB buffer per frame in
                   flight; torch's stream, and the host waits for a batch's conversions before it hands the batch over

Same process, same card; a prepass leg codes the file its filter's leg codes (checked).  Wall clock around the whole queue,
fill and drain included; `--repeats` timed repeats of each leg after one untimed pass.

    python scripts/chroma_filter_probe.py [--legs nearest,centre,left,prepass-centre,prepass-left] [--frames 256]
                                          [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/chroma_filters.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["nearest", "centre", "left", "prepass-centre", "prepass-left"]
FILTER = {"nearest": 0, "centre": 1, "left": 2}
BT709 = (16, 19077, 29372, 3494, 8731, 34610)  # yo, cy, crv, cgu, cgv, cbu (csrc/hip/hydk_yuv.h)


class Prepass:
    """the interpolating formats' definition (BT.709, limited range) as torch kernels: y (H, W), uv (ch, cw, 2) -> out (H, W, 3)"""

    def __init__(self, filt, w, h, dev):
        import torch

        ch, cw = (h + 1) // 2, (w + 1) // 2
        y, x = torch.arange(h, device=dev), torch.arange(w, device=dev)
        self.filt, self.odd = filt, (x & 1).bool()[None, :, None]
        self.cy, self.cx = y >> 1, x >> 1
        self.vy = (self.cy + torch.where((y & 1) == 1, 1, -1)).clamp_(0, ch - 1)
        self.hx = (self.cx + torch.where((x & 1) == 1, 1, -1 if filt == 1 else 0)).clamp_(0, cw - 1)

    def __call__(self, y, uv, out):
        import torch

        yo, cy, crv, cgu, cgv, cbu = BT709
        c = uv.to(torch.int32)
        vmix = 3 * c.index_select(0, self.cy) + c.index_select(0, self.vy)  # (H, cw, 2)
        v0, v1 = vmix.index_select(1, self.cx), vmix.index_select(1, self.hx)
        if self.filt == 1:
            up = (3 * v0 + v1 + 8) >> 4
        else:
            up = torch.where(self.odd, (v0 + v1 + 4) >> 3, (v0 + 2) >> 2)
        d, e = up[..., 0] - 128, up[..., 1] - 128
        luma = (y.to(torch.int32) - yo) * cy + 8192
        out[..., 0] = ((luma + crv * e) >> 14).clamp_(0, 255)
        out[..., 1] = ((luma - cgu * d - cgv * e) >> 14).clamp_(0, 255)
        out[..., 2] = ((luma + cbu * d) >> 14).clamp_(0, 255)
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

    import chroma_model as cm
    import yuv_model as ym
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    y, uv = ym.nv12_of_rgb(synth.make_image("photo", w, h, 8, 1234), 0)
    surface = torch.from_numpy(np.concatenate([y.reshape(-1), uv.reshape(-1)])).cuda()  # pitch 3840: one allocation, as a decoder's
    pics = {name: device.Nv12.from_surface(surface, w, h, w, w * h, device.NV12_BT709, chroma=name) for name in FILTER}
    prepass = {}
    for name in ("centre", "left"):
        prepass[name] = Prepass(FILTER[name], w, h, surface.device)
        model = torch.from_numpy(cm.expected_rgb((y, uv), 0, FILTER[name])).cuda()
        assert torch.equal(prepass[name](pics[name].y, pics[name].uv, torch.empty_like(model)), model), "the torch pre-pass is not the model"
    ring = [torch.empty((h, w, 3), dtype=torch.uint8, device=surface.device) for _ in range(G * S)]  # an RGB buffer per frame in flight
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' as NV12 (BT.709, limited range) resident in HBM -> files in HBM; "
          f"{G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    digests = {}
    for leg in args.legs.split(","):
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]
        name = leg.rpartition("-")[2]

        def batch_of(k, n):
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
        assert digests.setdefault(name, digest) == digest, "a pre-pass leg codes another file than its filter's leg"
        print(f"{leg:15s} files/s  " + "  ".join(f"{r:7.1f}" for r in rates) +
              f"   median {sorted(rates)[len(rates) // 2]:7.1f}  spread {min(rates):7.1f} .. {max(rates):7.1f}"
              f"   file {len(files[0])} B md5 {digest} all alike {same}  reruns {[fb.overflow_reruns() for fb in fbs]}")
        for fb in fbs:
            fb.close()


if __name__ == "__main__":
    main()
