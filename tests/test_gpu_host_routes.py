"""GPU: every route by which hyd_send_tile brings a frame's results back to the host and writes the frame there
(csrc/host/encoder.c finish_frame_collect, csrc/host/hostframe.c), each on the smallest frame that takes it, against the
reference's file for the same picture.

The switches that choose a route are latched per process, so every case is a child process of its own; they run one at a
time, each under its own timeout, and after a child that crashed or timed out no further one is started (those cases fail).
The sharded routes are held by test_gpu_multi_device.py."""
import os
import subprocess
import sys

import pytest

from conftest import has_gpu
from hydrium_amd import api

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120
_state = {"stopped": None, "want": {}}

# 200x120: one group.  600x300: the smallest frame with several groups and a ragged edge in both directions (one LF group).
# 2304x264: the smallest frame with two LF groups.  shift 0: 256x256 tiles, six frames, the last ragged.
ROUTES = [
    ("one-group-staged-blob", 200, 120, -1, {}),
    ("one-group-separate-copies", 200, 120, -1, {"HYDAMD_STAGED_READBACK": "0"}),
    ("one-group-lf-ints-on-host", 200, 120, -1, {"HYDAMD_LF_CODER": "0"}),
    ("groups-early-lf-staged-tables", 600, 300, -1, {"HYDAMD_HOST_ASSEMBLY": "1"}),
    ("groups-early-lf-separate-copies", 600, 300, -1, {"HYDAMD_HOST_ASSEMBLY": "1", "HYDAMD_STAGED_READBACK": "0"}),
    ("two-lf-groups-parallel-sections", 2304, 264, -1, {"HYDAMD_HOST_ASSEMBLY": "1"}),
    ("two-lf-groups-lf-ints-on-host", 2304, 264, -1, {"HYDAMD_HOST_ASSEMBLY": "1", "HYDAMD_LF_CODER": "0"}),
    ("tile-mode-ring-of-3", 600, 300, 0, {"HYDAMD_TILE_PIPELINE": "3"}),
]

_CHILD = """
import sys
from hydrium_amd import api, synth
w, h, shift, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
data = api.encode_image(api.Library(), synth.make_image("photo", w, h, 8), shift_x=shift, shift_y=shift)
with open(out, "wb") as f:
    f.write(data)
"""


@pytest.mark.parametrize("route,w,h,shift,extra", ROUTES, ids=[r[0] for r in ROUTES])
def test_host_route_gives_the_reference_file(ref_lib, tmp_path, route, w, h, shift, extra):
    if _state["stopped"]:
        pytest.fail(f"not run: the child of {_state['stopped']} crashed or timed out before it")
    if (w, h, shift) not in _state["want"]:
        from hydrium_amd import synth

        _state["want"][w, h, shift] = api.encode_image(ref_lib, synth.make_image("photo", w, h, 8), shift_x=shift, shift_y=shift)
    want = _state["want"][w, h, shift]
    out = str(tmp_path / "file.jxl")
    env = {k: v for k, v in os.environ.items() if not k.startswith("HYDAMD_") or k == "HYDAMD_LIB"}
    env.update(extra, PYTHONPATH=ROOT)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD, str(w), str(h), str(shift), out], capture_output=True, text=True,
                           env=env, timeout=CHILD_TIMEOUT_S, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _state["stopped"] = route
        pytest.fail(f"{route}: timed out after {CHILD_TIMEOUT_S} s\n{e.stdout or ''}\n{e.stderr or ''}")
    if r.returncode < 0 or r.returncode in (134, 139):
        _state["stopped"] = route
    assert r.returncode == 0, f"{route}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(out, "rb") as f:
        got = f.read()
    assert len(got) == len(want) and got == want, f"{route}: the file differs from the reference's"
