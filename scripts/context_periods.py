"""Every context's own period in bench.py's frame loop, beside the queue pool of its stream (hydamd_stream_class): the loop of
bench.py's timed_run — 16 contexts, two 8192x8192 RGB16 'photo' frames per launch group, a picture of its own per frame, contexts
in turn, one HIP event behind every launch group, 10 priming groups per context — and what timed_run computes from the events:
ms per frame of each context's stream (a context completes one launch group per S group periods).
usage: python scripts/context_periods.py [groups_per_context=8]   (HYDAMD_LIB names another build of the library)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hydrium_amd import device, synth

S, FPL, W, H = 16, 2, 8192, 8192
groups = int(sys.argv[1]) if len(sys.argv) > 1 else 8
dev = torch.device("cuda", 0)
ctxs = [device.DeviceContext(0, 16 * FPL, 0) for _ in range(S)]
pictures = [[synth.make_image("photo", W, H, 16, x0=0, y0=(1 + k * FPL + f) * H, device=dev) for f in range(FPL)] for k in range(S)]
torch.cuda.synchronize()
for c in ctxs:
    c.set_rans_waves(5)
    c.set_lf_coder(2)
ext = [torch.cuda.ExternalStream(c.get_stream()) for c in ctxs]
for k, c in enumerate(ctxs):
    c.encode_image_batch(pictures[k])
for c in ctxs:
    c.sync()
nprime, evs = 10 * S, []
for i in range(nprime + groups * S + S):
    ctxs[i % S].encode_image_batch(pictures[i % S])
    ev = torch.cuda.Event(enable_timing=True)
    ev.record(ext[i % S])
    evs.append(ev)
for c in ctxs:
    c.sync()
torch.cuda.synchronize()
done = [evs[0].elapsed_time(e) for e in evs]
a, b = nprime, nprime + groups * S
rate = W * H * FPL * groups * S / ((sum(done[b - S:b]) - sum(done[a - S:a])) / S * 1e-3) / 1e6
names = {0: "normal", 1: "high", 2: "low"}
by_class = {}
print(f"# {S} contexts x {FPL} frames per launch group, {groups} timed groups per context: {rate:.1f} Mpixel/s")
print("context  class   ms per frame of its stream")
for k, c in enumerate(ctxs):
    mine = [done[i] for i in range(a, b) if i % S == k]
    p = (mine[-1] - mine[0]) / (len(mine) - 1) / S / FPL
    by_class.setdefault(c.stream_class(), []).append(p)
    print(f"{k:7d}  {names[c.stream_class()]:6s}  {p:.4f}")
for cls, ps in sorted(by_class.items()):
    print(f"# {names[cls]:6s}: {len(ps):2d} contexts, mean {sum(ps) / len(ps):.4f}, min {min(ps):.4f}, max {max(ps):.4f}")
allp = [p for ps in by_class.values() for p in ps]
print(f"# all: min {min(allp):.4f}, max {max(allp):.4f}, max/min {max(allp) / min(allp):.3f}")
for c in ctxs:
    c.close()
