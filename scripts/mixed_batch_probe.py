#!/usr/bin/env python3
"""A queue of RGB8 photo pictures OF MANY SIZES resident in HBM, every one to a finished file in HBM: files per second of
  (a) MixedBatch (hydamd_mixed_*): `--per-batch` pictures per call, `--objects` objects in flight;
  (b) one context per picture — hydamd_encode_image + hydamd_export_frame_owned + hydamd_context_assembler with a plan
      per picture (pictures of one 256 x 256 group, which that assembler refuses: the staged blob and
      hydamd_frame_from_blobs on the host), the only route to files for such a corpus without MixedBatch — with the
      same number of PICTURES in flight as (a);
  (c) the same corpus PADDED into shape classes (each side up to the next of 256, 512, 1024, 2048) through one
      FrameBatch per class, `--per-batch` frames per call: what a caller who may alter the pictures could reach.  Its
      files are not the pictures' files (they hold the padding); an upper reference, not an alternative.
The corpus is fixed and seeded: `--pictures` windows of a few 2048 x 2048 'photo' pictures, each a contiguous tensor of
its own, both sides drawn log-uniformly from 64 ... 2048 (small pictures are the workload; uniform sides would make the
corpus mostly megapixels).  Same process, same card, same pictures; wall clock around the whole queue, fill and drain
included; `--repeats` timed repeats of each loop after one untimed pass that touches every buffer and every shape.

    python scripts/mixed_batch_probe.py [--pictures 384] [--per-batch 16] [--objects 4] [--repeats 3] > profiles/mixed_batch.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus_sizes(n, seed=20240607):
    import numpy as np

    rng = np.random.default_rng(seed)
    sides = np.exp(rng.uniform(np.log(64.0), np.log(2048.0), size=(n, 2)))
    return [(int(min(2048, max(64, round(w)))), int(min(2048, max(64, round(h))))) for w, h in sides]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=384)
    ap.add_argument("--per-batch", type=int, default=16)
    ap.add_argument("--objects", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    from hydrium_amd import api, device, synth

    G, S, N = args.per_batch, args.objects, args.pictures
    sizes = corpus_sizes(N)
    rng = np.random.default_rng(7)
    sources = [synth.make_image("photo", 2048, 2048, 8, seed=1234 + k, device="cuda") for k in range(4)]
    imgs = []
    for k, (w, h) in enumerate(sizes):
        x0, y0 = int(rng.integers(0, 2048 - w + 1)), int(rng.integers(0, 2048 - h + 1))
        imgs.append(sources[k % len(sources)][y0:y0 + h, x0:x0 + w, :].contiguous())
    del sources
    torch.cuda.synchronize()
    pixels = sum(w * h for w, h in sizes)
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    print(f"# {N} RGB8 'photo' pictures, sides log-uniform in 64 ... 2048 (seeded; {len(set(sizes))} distinct sizes, "
          f"{pixels / 1e6:.1f} Mpixel in all, median {sorted(w * h for w, h in sizes)[N // 2] / 1e6:.2f} Mpixel) resident in HBM -> files in HBM; "
          f"{G} pictures per batch, {S} objects in flight (= {G * S} pictures in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    def timed(name, once):
        once()  # every buffer touched, every shape seen
        rates = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            rates.append(N / (time.perf_counter() - t0))
        print(f"{name:76s} files/s  " + "  ".join(f"{r:8.1f}" for r in rates) + f"   median {sorted(rates)[len(rates) // 2]:8.1f}", flush=True)
        return rates

    # ---- (a) MixedBatch ----
    mbs = [device.MixedBatch(G) for _ in range(S)]
    totals = {}

    def loop_a():
        busy = [False] * S
        for i, grp in enumerate(groups):
            mb = mbs[i % S]
            if busy[i % S]:
                mb.result()
            mb.encode([imgs[f] for f in grp])
            busy[i % S] = True
        for k in range(S):
            if busy[k]:
                totals[k] = mbs[k].result()

    timed("(a) MixedBatch: finished files, one call and one buffer per batch of sizes", loop_a)
    # what the last batch of object 0 left, against the drop-in encoder's file for the same picture
    last = [grp for i, grp in enumerate(groups) if i % S == 0][-1]
    lib = api.Library()
    ok = all(bytes(f) == api.encode_image(lib, np.ascontiguousarray(imgs[k].cpu().numpy()), shift_x=-1, shift_y=-1, out_buf_size=1 << 25)
             for f, k in zip(mbs[0].read(), last))
    print(f"    files of the last batch equal to hyd_send_tile's for the same pictures: {ok}; reruns {[mb.overflow_reruns() for mb in mbs]}",
          flush=True)
    for mb in mbs:
        mb.close()

    # ---- (b) one context and one assembler per picture, G x S pictures in flight ----
    d = device.dll()
    ctxs = [device.DeviceContext(0, 1, 0) for _ in range(G * S)]
    for c in ctxs:
        c.set_rans_waves(5)
        c.set_lf_coder(2)
    mds = [api.HYDImageMetadata(w, h, 0, -1, -1) for w, h in sizes]
    slots = (C.c_uint32 * 1)(1)
    ids = (C.c_uint32 * 1)(0)

    def ck(c, asm, st):
        if st:
            raise RuntimeError((d.hydamd_assembler_error(asm) or d.hydamd_error(c.h) or b"").decode())

    # the device-side frame assembler refuses a frame of ONE 256 x 256 group (a single bit-contiguous section: "assemble it
    # on the host"), so such a picture takes the route hyd_send_tile takes for it: the staged blob, one copy to the host,
    # hydamd_frame_from_blobs — its file ends in HOST memory
    d.hydamd_stage_frame_blob.argtypes = [C.c_void_p, C.c_int]
    d.hydamd_read_frame_blob.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    one_group = [w <= 256 and h <= 256 for w, h in sizes]
    pending = [None] * len(ctxs)

    def collect(k):
        c, f = ctxs[k], pending[k]
        c.sync()
        if one_group[f]:
            blob, size = C.c_void_p(0), C.c_size_t(0)
            c._ck(d.hydamd_read_frame_blob(c.h, 1, C.byref(blob), C.byref(size)))
            if not size.value:
                raise RuntimeError("a staged frame was rerun")
            return len(device.frame_from_blobs(mds[f], [(C.c_uint8 * size.value).from_address(blob.value)]))
        size = C.c_size_t(0)
        asm = d.hydamd_context_assembler(c.h)
        ck(c, asm, d.hydamd_assembler_result(asm, C.byref(size)))
        return size.value

    def loop_b():
        for f in range(N):
            k = f % len(ctxs)
            c = ctxs[k]
            if pending[k] is not None:
                collect(k)
            c.encode_image_tensor(imgs[f])
            pending[k] = f
            if one_group[f]:
                c._ck(d.hydamd_stage_frame_blob(c.h, 1))
                continue
            blob, cap = c.export_frame_owned(1)
            asm = d.hydamd_context_assembler(c.h)
            ck(c, asm, d.hydamd_assembler_plan(asm, C.byref(mds[f]), 1, 1, 1, slots, ids, None, 0))
            ptr, caps = (C.c_void_p * 1)(blob), (C.c_size_t * 1)(cap)
            ck(c, asm, d.hydamd_assembler_run(asm, ptr, caps, c.get_stream(), None, c.blob_bound(1)))
        for k in range(len(ctxs)):
            if pending[k] is not None:
                collect(k)
                pending[k] = None

    print(f"    (b): {sum(one_group)} of the {N} pictures are one 256 x 256 group, which the device-side frame assembler refuses: "
          f"those are assembled on the host from the staged blob, as hyd_send_tile does", flush=True)
    timed("(b) a context and an assembler per picture: finished files, one by one", loop_b)
    for c in ctxs:
        c.close()

    # ---- (c) padded into shape classes, one FrameBatch per class ----
    def up(v):
        return next(s for s in (256, 512, 1024, 2048) if v <= s)

    classes = {}
    for f, (w, h) in enumerate(sizes):
        classes.setdefault((up(w), up(h)), []).append(f)
    padded = {}
    for (cw, ch), members in classes.items():
        for f in members:
            w, h = sizes[f]
            p = torch.zeros((ch, cw, 3), dtype=torch.uint8, device="cuda")
            p[:h, :w, :] = imgs[f]
            padded[f] = p
    torch.cuda.synchronize()
    fbs = {cls: device.FrameBatch(cls[0], cls[1], G) for cls in classes}
    work = [(cls, members[i:i + G]) for cls, members in classes.items() for i in range(0, len(members), G)]
    work.sort(key=lambda cm: cm[1][0])  # in the order the queue delivers each batch's first picture
    padded_pixels = sum(cw * ch * len(m) for (cw, ch), m in classes.items())

    def loop_c():
        busy = dict.fromkeys(fbs, False)
        for cls, members in work:
            fb = fbs[cls]
            if busy[cls]:
                fb.result()
            fb.encode([padded[f] for f in members])
            busy[cls] = True
        for cls, fb in fbs.items():
            if busy[cls]:
                fb.result()

    timed(f"(c) padded into {len(classes)} shape classes, one FrameBatch per class ({padded_pixels / pixels:.2f} x the pixels)", loop_c)
    for fb in fbs.values():
        fb.close()


if __name__ == "__main__":
    main()
