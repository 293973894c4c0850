#!/usr/bin/env python3
"""One 3840 x 2160 picture resident in HBM with one group of four samples a pixel (AYUV: what a decoder leaves for 4:4:4 8-bit video;
Y412 / Y416: the same in 12 and 16 bits, XV36 / XV48) through FrameBatch to finished files in HBM, nine ways: files per second of each.

  ayuv           the AYUV surface (BT.709, limited range) read by the transform kernel
  i444           the same samples as three I444 planes — the yardstick: 3 bytes a pixel from three streams, and the same file as ayuv
  rgb8           ayuv's picture as RGB8 already in HBM
  ayuvprepass    the AYUV surface de-interleaved and converted to RGB8 by a torch pre-pass for every frame, then as rgb8: the route a
                 caller had before these formats.  The pre-pass is the conversion's integer formula in torch int64 arithmetic, into
                 an RGB buffer per frame in flight; it runs on torch's stream, and the host waits for a batch's conversions before it
                 hands the batch over (FrameBatch has no stream hand-over).
  y416           a Y416 surface read by the transform kernel
  y412           the same picture's 12-bit codes as a Y412 surface (low four bits zero)
  i416           y416's samples as three I416 planes — the yardstick: 6 bytes a pixel from three streams, and the same file as y416
  rgb16          y416's picture as RGB16 already in HBM
  y416prepass    the Y416 surface through the same kind of torch pre-pass to RGB16, then as rgb16

Same process, same card.  Wall clock around the whole queue, fill and drain included; `--repeats` timed repeats of each leg
after one untimed pass.

    python scripts/quad_formats_probe.py [--legs ayuv,i444] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

Results: profiles/quad_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LEGS = ["ayuv", "i444", "rgb8", "ayuvprepass", "y416", "y412", "i416", "rgb16", "y416prepass"]


def to_rgb(samples, table, out):
    """the conversion of a (H, W, 4) surface of samples — bytes V, U, Y, A or words U, Y, V, A — as torch elementwise kernels -> out
    (H, W, 3) of the class's samples.  table: (yo, cy, crv, cgu, cgv, cbu) of the models; bytes: scale 2^14, words: scale 2^20"""
    import torch

    wide = samples.element_size() == 2
    mask, mid, shift, top = (0xFFFF, 32768, 20, 65535) if wide else (0xFF, 128, 14, 255)
    s = samples.to(torch.int64) & mask
    y, u, v = (s[..., 1], s[..., 0], s[..., 2]) if wide else (s[..., 2], s[..., 1], s[..., 0])
    yo, cy, crv, cgu, cgv, cbu = table
    c, d, e = y - yo, u - mid, v - mid
    half = 1 << (shift - 1)
    out[..., 0] = torch.clamp((cy * c + crv * e + half) >> shift, 0, top)
    out[..., 1] = torch.clamp((cy * c - cgu * d - cgv * e + half) >> shift, 0, top)
    out[..., 2] = torch.clamp((cy * c + cbu * d + half) >> shift, 0, top)
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

    import p016_model as p16
    import quad_model as qm
    import yuv_model as ym
    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    AYUV, Y412, Y416 = qm.AYUV[0], qm.Y412[0], qm.Y416[0]

    def photo(bits):
        p = synth.make_image("photo", w, h, bits, 1234)
        p = p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)
        return p.view(np.uint16 if bits == 16 else np.uint8)

    host = {"ayuv": qm.surface_of_rgb(photo(8), AYUV, 255), "y416": qm.surface_of_rgb(photo(16), Y416, 65535), "y412": qm.surface_of_rgb(photo(16), Y412, 65535)}
    surfaces = {k: torch.from_numpy(v.view(np.int64 if v.itemsize == 8 else np.int32)).cuda() for k, v in host.items()}  # pitch = the row
    pics = {"ayuv": device.Ayuv(surfaces["ayuv"], w, device.NV12_BT709), "y416": device.Y416(surfaces["y416"], w, device.NV12_BT709, 16),
            "y412": device.Y416(surfaces["y412"], w, device.NV12_BT709, 12)}
    planes8 = [torch.from_numpy(p).cuda() for p in qm.samples(host["ayuv"], AYUV)[:3]]  # three allocations, chroma pitch = the width
    pics["i444"] = device.PlanarYuv(*planes8, device.NV12_BT709, "444", None)
    planes16 = [torch.from_numpy(p.view(np.int16)).cuda() for p in qm.samples(host["y416"], Y416)[:3]]
    pics["i416"] = device.PlanarYuv16(*planes16, device.NV12_BT709, "444", None, 16)
    rgb8 = torch.from_numpy(qm.expected_rgb(host["ayuv"], AYUV)).cuda()
    rgb16 = torch.from_numpy(qm.expected_rgb(host["y416"], Y416).view(np.int16)).cuda()
    tensors = {"rgb8": rgb8, "rgb16": rgb16}
    samples = {"ayuvprepass": surfaces["ayuv"].view(torch.uint8).view(h, w, 4), "y416prepass": surfaces["y416"].view(torch.int16).view(h, w, 4)}
    tables = {"ayuvprepass": ym.TABLE[0], "y416prepass": p16.TABLE[3, 0]}
    assert torch.equal(to_rgb(samples["ayuvprepass"], tables["ayuvprepass"], torch.empty_like(rgb8)), rgb8), "the torch pre-pass is not the model's conversion"
    assert torch.equal(to_rgb(samples["y416prepass"], tables["y416prepass"], torch.empty_like(rgb16)), rgb16), "the torch pre-pass is not the model's conversion"
    rings = {"ayuvprepass": [torch.empty_like(rgb8) for _ in range(G * S)], "y416prepass": [torch.empty_like(rgb16) for _ in range(G * S)]}
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' with one group of four samples a pixel (AYUV / Y412 / Y416, BT.709 limited "
          f"range) resident in HBM -> files in HBM; {G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + "
          f"{args.repeats} timed repeats; {torch.cuda.get_device_name(0)}")

    for leg in args.legs.split(","):
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]

        def batch_of(k, n):
            if leg in pics:
                return [pics[leg]] * n
            if leg in tensors:
                return [tensors[leg]] * n
            bufs = rings[leg][k * G: k * G + n]  # (the object's previous batch has been waited for: its buffers are free)
            for b in bufs:
                to_rgb(samples[leg], tables[leg], b)
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
        print(f"{leg:11s} files/s  " + "  ".join(f"{r:7.1f}" for r in rates) +
              f"   median {sorted(rates)[len(rates) // 2]:7.1f}  spread {min(rates):7.1f} .. {max(rates):7.1f}"
              f"   file {len(files[0])} B md5 {digest} all alike {same}  reruns {[fb.overflow_reruns() for fb in fbs]}", flush=True)
        for fb in fbs:
            fb.close()


if __name__ == "__main__":
    main()
