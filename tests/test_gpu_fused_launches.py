"""GPU: the frame loop's fused launches against the CPU oracle, the LF model and the reference.

A lane-form launch group coded by the in-stream LF coder runs six launches: the LF coder's token workgroups ride in the
table kernel's launch, its code builders in the chain kernel's and its pack workgroups in the emit kernel's, where they
write the packed LF area straight at the place the slots' bit counts give; no k_lf_tokens, k_lf_pack or k_lf_gather.
tests/fused_frames.py picks launch groups whose slots have one, two, 220 and differing numbers of windows and six slots in
two frames; here their sections, offsets[], total, LF area, read_lf_bits and whole files are compared, twice on one context
with longer streams coded in between.  The emit role's share is set to extremes beside many and few pack workgroups, the
routes that keep staging and gather (side stream, growing calls, HYDAMD_LF_CODES_RIDE=tables, a float picture in the launch
group) are held to the direct route's bytes, and a payload one byte short must rerun once and leave the same LF area."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu, reference_expected

import closing_frames as cf
import fused_frames as ff

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120


@pytest.fixture(scope="module")
def cases():
    """name -> (images, expectation), computed once; checked to hold the window counts the tests are about"""
    out = {name: (imgs, ff.expectation(imgs)) for name, imgs in ((n, f()) for n, f in ff.CASES.items())}
    assert ff.windows_of(out["8x8"][0][0]) == [1]
    assert ff.windows_of(out["104x184"][0][0]) == [2] and 3 * 13 * 23 == ff.WINDOW + 1
    assert ff.windows_of(out["4200x72"][0][0]) == [8, 8, 1]
    assert ff.windows_of(out["2048x2048"][0][0]) == [220]
    for name, (_, exp) in out.items():
        print(f"  {name}: LF bit counts {[n for _, n in exp['lf']]}")
    three = [n for _, n in out["4200x72"][1]["lf"]]
    assert all(n % 32 for n in three) and three[1] < three[0] // 8, "the flat plane's stream is not the short, unaligned one"
    assert len(out["batch_4200x72"][1]["lf"]) == 6 and out["batch_4200x72"][1]["lf"][0][1] != out["batch_4200x72"][1]["lf"][3][1]
    return out


def _child(tmp_path, cases, mode, case, extra_env):
    exp_path, report = str(tmp_path / "expectation.npz"), str(tmp_path / "report.json")
    ff.save_expectation(exp_path, cases[case][1])
    env = {k: v for k, v in os.environ.items() if not k.startswith("HYDAMD_")}
    env.update(extra_env, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_frames.py"), mode, case, exp_path, report],
                       capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT_S, cwd=ROOT)
    rep = {}
    if os.path.exists(report):
        with open(report) as f:
            rep = json.load(f)
    assert r.returncode == 0 and rep.get("done"), \
        f"child ended with {r.returncode}: {rep.get('error')}\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"
    return rep["runs"]


@pytest.mark.parametrize("name", list(ff.CASES))
def test_window_counts_that_differ_inside_one_launch(cases, ref_lib, name):
    from hydrium_amd import api, device

    images, exp = cases[name]
    with device.DeviceContext(0, max(3, len(exp["lf"])), 0) as ctx:
        ctx.set_lf_coder(2)
        ff.visit_twice(ctx, images, exp, name)
        assert ctx.overflow_reruns() == 0
    assert reference_expected()
    if len(images) == 1:
        assert bytes(api.encode_image(api.Library(), images[0].copy())) == bytes(api.encode_image(ref_lib, images[0].copy())), "whole file"
    else:
        h, w, _ = images[0].shape
        with device.FrameBatch(w, h, len(images)) as fb:
            fb.encode([cf.torch_image(i) for i in images])
            files = fb.read()
        for k, img in enumerate(images):
            assert bytes(files[k]) == bytes(api.encode_image(ref_lib, img.copy())), f"frame {k}: whole file"


@pytest.mark.parametrize("share,name", [(16, "2048x2048"), (3, "batch_4200x72")])
def test_emit_share_beside_pack_workgroups(cases, tmp_path, share, name):
    """HYDAMD_EMIT_SHARE=16 on one slot: ONE emit workgroup in front of 220 pack workgroups.  3 on six slots: 96 virtual
    blocks, which 3 divides, in 32 emit workgroups; the pack workgroups' indices start behind them."""
    runs = _child(tmp_path, cases, "visit", name, {"HYDAMD_EMIT_SHARE": str(share)})
    assert runs["visit"]["reruns"] == 0


def test_routes_that_keep_staging_agree_with_the_direct_one(cases, tmp_path):
    from hydrium_amd import device

    images, exp = cases["4200x72"]
    img = images[0]
    t = cf.torch_image(img)
    blobs = {}
    for name, coder in (("direct", 2), ("side stream", 1)):
        with device.DeviceContext(0, 3, 0) as ctx:
            ctx.set_lf_coder(coder)
            blobs[name] = ff.visit_twice(ctx, images, exp, name)
    with device.DeviceContext(0, 3, 0) as ctx:   # the slots coded by three growing calls in front of the entropy stage
        ctx.set_lf_coder(2)
        base, w = t.data_ptr(), img.shape[1]
        for visit in range(2):
            ctx.begin_frame(3)
            for s in range(3):
                p = base + s * 2048 * 3
                ctx.encode_lf_group(s, [p, p + 1, p + 2], 3 * w, 3, 0, min(2048, w - s * 2048), img.shape[0], s)
                ctx.submit_lf_group(s)
            for n in (1, 2, 3):
                ctx.run_lf_coder(n, n == 3)
            ctx.finish_frame(3)
            ctx.sync()
            ff.check_sections(ctx, exp, f"three growing calls, visit {visit}")
            blobs["growing"] = ff.check_lf_area(ctx, exp, f"three growing calls, visit {visit}")
    runs = _child(tmp_path, cases, "visit", "4200x72", {"HYDAMD_LF_CODES_RIDE": "tables"})
    md5 = hashlib.md5(blobs["direct"]).hexdigest()
    assert blobs["side stream"] == blobs["growing"] == blobs["direct"] and runs["visit"]["lf_md5"] == md5


def test_a_float_picture_in_the_launch_group_keeps_the_staged_route(cases):
    """The float picture's 8-byte records keep the whole launch group on the wave form, whose LF coder is the late one of the
    closing stage (kernels of their own, staging, gather): every file as when its picture is coded alone, where the integer
    picture takes the direct route."""
    import torch

    from hydrium_amd import device, synth

    a = cf.torch_image(cases["104x184"][0][0])
    b = torch.from_numpy(synth.make_image_f32("photo", 264, 200)).cuda()
    with device.MixedBatch(2) as mb:
        alone = []
        for t in (a, b):
            mb.encode([t])
            alone.append(bytes(mb.read(0)))
        mb.encode([a, b], sample_fmts="each")
        both = [bytes(f) for f in mb.read()]
        mb.encode([b, a], sample_fmts="each")
        swapped = [bytes(f) for f in mb.read()]
        mb.encode([a])
        again = bytes(mb.read(0))
    assert both == alone and swapped == alone[::-1] and again == alone[0]


def test_payload_one_byte_short_leaves_the_same_lf_area(cases, tmp_path):
    """The overflow rerun replays the launch sequence: one rerun, sections and LF area as at exact fit."""
    runs = _child(tmp_path, cases, "payload", "4200x72", {})
    print(f"  {runs}")
    assert runs["exact"]["reruns"] == 0 and runs["short"]["reruns"] == 1
    assert runs["exact"]["lf_md5"] == runs["short"]["lf_md5"]
