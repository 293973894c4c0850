#!/usr/bin/env python3
"""A queue of 3840 x 2160 RGB8 photo frames resident in HBM, every one to a finished file in HBM: files per second of
  (a) FrameBatch (hydamd_batch_*): `--per-batch` frames per call, `--objects` objects in flight;
  (b) one context per frame — hydamd_encode_image + hydamd_export_frame_owned + hydamd_context_assembler, the only
      route to files for such frames without FrameBatch — with the same number of FRAMES in flight as (a);
  (c) the sections-only batch loop of bench.py's batch_device_leg (hydamd_encode_image_batch, no files): the ceiling.
Same process, same card, same pictures; wall clock around the whole queue, fill and drain included; `--repeats` timed
repeats of each loop after one untimed pass that touches every buffer.

    python scripts/batch_files_probe.py [--frames 512] [--per-batch 8] [--objects 4] [--repeats 3] > profiles/batch_files.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--per-batch", type=int, default=8)
    ap.add_argument("--objects", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    from hydrium_amd import api, device, synth

    w, h, distinct = 3840, 2160, 8
    G, S, N = args.per_batch, args.objects, args.frames
    n = 4  # LF groups of a 3840 x 2160 frame
    imgs = [synth.make_image("photo", w, h, 8, seed=1234 + k, device="cuda") for k in range(distinct)]
    torch.cuda.synchronize()
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {N} frames of {w} x {h} RGB8 'photo' ({distinct} distinct pictures) resident in HBM -> files in HBM; "
          f"{G} frames per batch, {S} objects in flight (= {G * S} frames in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    def timed(name, once):
        once()  # every buffer touched, every plan made
        rates = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            rates.append(N / (time.perf_counter() - t0))
        print(f"{name:68s} files/s  " + "  ".join(f"{r:8.1f}" for r in rates) + f"   median {sorted(rates)[len(rates) // 2]:8.1f}")
        return rates

    # ---- (a) FrameBatch ----
    fbs = [device.FrameBatch(w, h, G) for _ in range(S)]
    sizes = {}

    def loop_a():
        busy = [False] * S
        for i, grp in enumerate(groups):
            fb = fbs[i % S]
            if busy[i % S]:
                fb.result()
            fb.encode([imgs[f % distinct] for f in grp])
            busy[i % S] = True
        for k in range(S):
            if busy[k]:
                sizes[k] = fbs[k].result()

    timed("(a) FrameBatch: finished files, one call and one buffer per batch", loop_a)
    # what the last batch of object 0 left, against the drop-in encoder's file for the same picture
    last = [grp for i, grp in enumerate(groups) if i % S == 0][-1]
    lib = api.Library()
    ok = all(bytes(f) == api.encode_image(lib, np.ascontiguousarray(imgs[k % distinct].cpu().numpy()), out_buf_size=1 << 25)
             for f, k in zip(fbs[0].read(), last))
    print(f"    files of the last batch equal to hyd_send_tile's for the same pictures: {ok}; reruns {[fb.overflow_reruns() for fb in fbs]}")
    for fb in fbs:
        fb.close()

    # ---- (b) one context and one assembler per frame, G x S frames in flight ----
    d = device.dll()
    ctxs = [device.DeviceContext(0, n, 0) for _ in range(G * S)]
    for c in ctxs:
        c.set_rans_waves(5)
        c.set_lf_coder(2)
    md = api.HYDImageMetadata(w, h, 0, -1, -1)
    slots = (C.c_uint32 * 1)(n)
    ids = (C.c_uint32 * n)(*range(n))

    def ck(c, asm, st):
        if st:
            raise RuntimeError((d.hydamd_assembler_error(asm) or d.hydamd_error(c.h) or b"").decode())

    def collect(c):
        c.sync()
        size = C.c_size_t(0)
        asm = d.hydamd_context_assembler(c.h)
        ck(c, asm, d.hydamd_assembler_result(asm, C.byref(size)))
        return size.value

    def loop_b():
        busy = [False] * len(ctxs)
        for f in range(N):
            k = f % len(ctxs)
            c = ctxs[k]
            if busy[k]:
                collect(c)
            c.encode_image_tensor(imgs[f % distinct])
            blob, cap = c.export_frame_owned(n)
            asm = d.hydamd_context_assembler(c.h)
            ck(c, asm, d.hydamd_assembler_plan(asm, C.byref(md), 1, 1, 1, slots, ids, None, 0))
            ptr, caps = (C.c_void_p * 1)(blob), (C.c_size_t * 1)(cap)
            ck(c, asm, d.hydamd_assembler_run(asm, ptr, caps, c.get_stream(), None, c.blob_bound(n)))
            busy[k] = True
        for k, c in enumerate(ctxs):
            if busy[k]:
                collect(c)

    timed("(b) a context and an assembler per frame: finished files, one by one", loop_b)
    for c in ctxs:
        c.close()

    # ---- (c) sections only: the batch loop of bench.py's batch_device_leg ----
    ctxs = [device.DeviceContext(0, n * G, 0) for _ in range(S)]
    for c in ctxs:
        c.set_rans_waves(5)
        c.set_lf_coder(2)

    def loop_c():
        for i, grp in enumerate(groups):
            if len(grp) == G:
                ctxs[i % S].encode_image_batch([imgs[f % distinct] for f in grp])
            else:
                for f in grp:
                    ctxs[i % S].encode_image_tensor(imgs[f % distinct])
        for c in ctxs:
            c.sync()

    timed("(c) sections only (hydamd_encode_image_batch, no files): the ceiling", loop_c)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
