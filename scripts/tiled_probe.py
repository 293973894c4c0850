#!/usr/bin/env python3
"""Tile mode, 4096 x 4096 RGB8 photo, per image: device-resident pixels through TiledImage (frames built on the GPU, file
left in HBM; the read-back timed separately) against hyd_send_tile from host pixels with eight frames in flight
(hydamd_set_tile_pipeline(e, 8)), the best tile-mode path before TiledImage.  Same process, same card, shifts 0/0 .. 3/3.

    python scripts/tiled_probe.py [--images 20] [--warmup 3] [--size 4096] > profiles/tiled_mode.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ms):
    ms = sorted(ms)
    return f"median {statistics.median(ms):8.2f} ms   min {ms[0]:8.2f}   p90 {ms[int(0.9 * (len(ms) - 1))]:8.2f}   max {ms[-1]:8.2f}   n {len(ms)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    from hydrium_amd import api, device, synth

    n = args.size
    t = synth.make_image("photo", n, n, 8, device="cuda")
    torch.cuda.synchronize()
    host = np.ascontiguousarray(t.cpu().numpy())
    lib = api.Library()
    print(f"# tile mode, {n} x {n} RGB8 photo, per image; {args.warmup} warm-up + {args.images} timed images; {torch.cuda.get_device_name(0)}")
    for shift in (0, 1, 2, 3):
        with device.TiledImage(n, n, shift, shift) as ti:
            enc, rd = [], []
            out = np.empty(n * n * 2, np.uint8)
            for i in range(args.warmup + args.images):
                t0 = time.perf_counter()
                ti.encode(t)
                size = ti.result()
                t1 = time.perf_counter()
                ti.read(out)
                t2 = time.perf_counter()
                if i >= args.warmup:
                    enc.append((t1 - t0) * 1e3)
                    rd.append((t2 - t1) * 1e3)
            held = ti.device_bytes()
        buf = (C.c_uint8 * (n * n * 2))()
        base = []
        for i in range(args.warmup + args.images):
            t0 = time.perf_counter()
            ref = api.encode_image(lib, host, shift_x=shift, shift_y=shift, out_buf=buf, tile_pipeline=8)
            if i >= args.warmup:
                base.append((time.perf_counter() - t0) * 1e3)
        tiles = (-(-n // (256 << shift))) ** 2
        print(f"shift {shift}/{shift}  {tiles:4d} tiles  file {size} bytes  equal to hyd_send_tile's: {bytes(out[:size]) == bytes(ref)}")
        print(f"    TiledImage encode+result (file in HBM)   {stats(enc)}")
        print(f"    TiledImage read-back                     {stats(rd)}")
        print(f"    hyd_send_tile, 8 frames in flight        {stats(base)}")
        print(f"    device memory held by the TiledImage     {held / 2**20:.0f} MiB")


if __name__ == "__main__":
    main()
