#!/usr/bin/env python3
"""One 3840 x 2160 picture's values resident in HBM as float32, float16 and bfloat16, interleaved (H, W, 3) and planar
(three (H, W) planes: an NCHW network output), through FrameBatch to finished files in HBM: files per second of each form.
Same process, same card, the same values (the photo picture rounded to bfloat16, which float16 and float32 hold exactly,
so that every form codes the same file); wall clock around the whole queue, fill and drain included; `--repeats` timed
repeats of each form after one untimed pass.

    python scripts/half_formats_probe.py [--forms float32,float16,...] [--frames 256] [--per-batch 8] [--objects 4] [--repeats 3]

HYDAMD_LIB=hydrium_amd/lib/libhydrium_probe.so HYDAMD_DEBUG_HALF_PER_SAMPLE=3 sends the half forms through the per-sample
loader (the probe flavour's switch; without the variable the probe flavour runs what the shipped library runs).  A tree
without the half formats runs `--forms float32`.
Results: profiles/half_formats.txt.
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = ["float32", "float16", "float16-planar", "bfloat16", "bfloat16-planar"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--per-batch", type=int, default=8)
    ap.add_argument("--objects", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import torch

    from hydrium_amd import device, synth

    w, h = 3840, 2160
    G, S, N = args.per_batch, args.objects, args.frames
    values = torch.from_numpy(synth.make_image_f32("photo", w, h, 1234)).to(torch.bfloat16).cuda()
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {args.label or 'this tree'}: {N} frames of {w} x {h} 'photo' (bfloat16-exact values) resident in HBM -> files in HBM; "
          f"{G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed repeats; "
          f"library {os.environ.get('HYDAMD_LIB', 'as built')}; {torch.cuda.get_device_name(0)}")

    for form in args.forms.split(","):
        dtype = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[form.partition("-")[0]]
        if form.endswith("-planar"):
            nchw = values.to(dtype).permute(2, 0, 1).contiguous()
            frame = [nchw[c] for c in range(3)]
        else:
            frame = values.to(dtype).contiguous()
        torch.cuda.synchronize()
        fbs = [device.FrameBatch(w, h, G) for _ in range(S)]

        def once():
            busy = [False] * S
            for i, grp in enumerate(groups):
                fb = fbs[i % S]
                if busy[i % S]:
                    fb.result()
                fb.encode([frame] * len(grp))
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
        print(f"{form:18s} files/s  " + "  ".join(f"{r:7.1f}" for r in rates) +
              f"   median {sorted(rates)[len(rates) // 2]:7.1f}  spread {min(rates):7.1f} .. {max(rates):7.1f}"
              f"   file {len(files[0])} B md5 {digest} all alike {same}  reruns {[fb.overflow_reruns() for fb in fbs]}")
        for fb in fbs:
            fb.close()


if __name__ == "__main__":
    main()
