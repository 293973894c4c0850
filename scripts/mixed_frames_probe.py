#!/usr/bin/env python3
"""A queue of RGB8 photo pictures OF MANY SIZES AND LF-GROUP COUNTS resident in HBM, every one to a finished file in HBM:
files per second and Mpixel/s of
  (a) MixedBatch(max_lf_groups=...) (hydamd_mixed_create_slots): `--per-batch` pictures per call, `--objects` objects in
      flight, every object with as many LF-group slots as the corpus's fullest batch needs;
  (b) one context per picture — hydamd_encode_image + hydamd_export_frame_owned + hydamd_context_assembler with a plan
      per picture (pictures of one 256 x 256 group, which that assembler refuses: the staged blob and
      hydamd_frame_from_blobs on the host), the only route to files such a corpus had before — with the same number of
      PICTURES in flight as (a), every context with nine slots.
The corpus is fixed and seeded: `--pictures` windows of a few 6144 x 6144 'photo' pictures, each a contiguous tensor of
its own, both sides drawn log-uniformly from 64 ... 6144: up to nine LF groups.  Same process, same card, same pictures;
wall clock around the whole queue, fill and drain included; `--repeats` timed repeats of each loop after one untimed pass
that touches every buffer and every shape.  Device memory held: what torch.cuda.mem_get_info loses while a route's objects
exist (after the untimed pass).

    python scripts/mixed_frames_probe.py [--pictures 384] [--per-batch 16] [--objects 4] [--repeats 3] > profiles/mixed_frames.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIDE = 6144


def lf_groups(w, h):
    return -(-w // 2048) * -(-h // 2048)


def corpus_sizes(n, seed=20240607):
    import numpy as np

    rng = np.random.default_rng(seed)
    sides = np.exp(rng.uniform(np.log(64.0), np.log(float(SIDE)), size=(n, 2)))
    return [(int(min(SIDE, max(64, round(w)))), int(min(SIDE, max(64, round(h))))) for w, h in sides]


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
    sources = [synth.make_image("photo", SIDE, SIDE, 8, seed=1234 + k, device="cuda") for k in range(4)]
    imgs = []
    for k, (w, h) in enumerate(sizes):
        x0, y0 = int(rng.integers(0, SIDE - w + 1)), int(rng.integers(0, SIDE - h + 1))
        imgs.append(sources[k % len(sources)][y0:y0 + h, x0:x0 + w, :].contiguous())
    del sources
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    pixels = sum(w * h for w, h in sizes)
    counts = [lf_groups(w, h) for w, h in sizes]
    groups = [list(range(i, min(i + G, N))) for i in range(0, N, G)]
    slots = max(sum(counts[f] for f in grp) for grp in groups)
    print(f"# {N} RGB8 'photo' pictures, sides log-uniform in 64 ... {SIDE} (seeded; {len(set(sizes))} distinct sizes, "
          f"{pixels / 1e6:.1f} Mpixel in all, median {sorted(w * h for w, h in sizes)[N // 2] / 1e6:.2f} Mpixel; LF groups per picture: "
          + ", ".join(f"{n}: {counts.count(n)}" for n in sorted(set(counts))) + f") resident in HBM -> files in HBM; "
          f"{G} pictures per batch, {S} objects in flight (= {G * S} pictures in flight); 1 untimed + {args.repeats} timed repeats; "
          f"{torch.cuda.get_device_name(0)}")

    def held():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def timed(name, once, free_before):
        once()  # every buffer touched, every shape seen
        mem = (free_before - held()) / 2.0 ** 30
        rates = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            rates.append(N / (time.perf_counter() - t0))
        med = sorted(rates)[len(rates) // 2]
        print(f"{name:76s} files/s  " + "  ".join(f"{r:8.1f}" for r in rates) + f"   median {med:8.1f}  = {med * pixels / N / 1e6:8.1f} Mpixel/s"
              f"   device memory held {mem:6.1f} GiB", flush=True)
        return rates

    # ---- (a) MixedBatch with LF-group slots ----
    free0 = held()
    mbs = [device.MixedBatch(G, max_lf_groups=slots) for _ in range(S)]
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

    timed(f"(a) MixedBatch(max_lf_groups={slots}): finished files, one call and one buffer per batch", loop_a, free0)
    # what the last batch of object 0 left, against the drop-in encoder's file for the same picture
    last = [grp for i, grp in enumerate(groups) if i % S == 0][-1]
    lib = api.Library()
    ok = all(bytes(f) == api.encode_image(lib, np.ascontiguousarray(imgs[k].cpu().numpy()), shift_x=-1, shift_y=-1, out_buf_size=1 << 27)
             for f, k in zip(mbs[0].read(), last))
    print(f"    files of the last batch equal to hyd_send_tile's for the same pictures: {ok}; reruns {[mb.overflow_reruns() for mb in mbs]}",
          flush=True)
    for mb in mbs:
        mb.close()

    # ---- (b) one context and one assembler per picture, G x S pictures in flight ----
    d = device.dll()
    free0 = held()
    ctxs = [device.DeviceContext(0, max(counts), 0) for _ in range(G * S)]
    for c in ctxs:
        c.set_rans_waves(5)
        c.set_lf_coder(2)
    mds = [api.HYDImageMetadata(w, h, 0, -1, -1) for w, h in sizes]
    ids = (C.c_uint32 * max(counts))(*range(max(counts)))

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
            n = counts[f]
            blob, cap = c.export_frame_owned(n)
            asm = d.hydamd_context_assembler(c.h)
            ck(c, asm, d.hydamd_assembler_plan(asm, C.byref(mds[f]), 1, 1, 1, (C.c_uint32 * 1)(n), ids, None, 0))
            ptr, caps = (C.c_void_p * 1)(blob), (C.c_size_t * 1)(cap)
            ck(c, asm, d.hydamd_assembler_run(asm, ptr, caps, c.get_stream(), None, c.blob_bound(n)))
        for k in range(len(ctxs)):
            if pending[k] is not None:
                collect(k)
                pending[k] = None

    print(f"    (b): {sum(one_group)} of the {N} pictures are one 256 x 256 group, which the device-side frame assembler refuses: "
          f"those are assembled on the host from the staged blob, as hyd_send_tile does", flush=True)
    timed(f"(b) a context ({max(counts)} slots) and an assembler per picture: finished files, one by one", loop_b, free0)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
