"""GPU: token and payload buffers at exact fit, and one step short of it, against the reference.

Every kernel of the hot path writes into arrays sized by HYDAMD_TOKEN_CAP records per group (a split transform launch: a
share of tok_cap >> plog per part) and HYDAMD_PAYLOAD_CAP section bytes; a frame that does not fit is rerun at the hard
maxima.  A compare loose by one at these edges is silent: a record lands in the neighbouring group's array, a consumer reads
a round past an exact-fit one, and the bytes are wrong with HYD_OK.  tests/edge_frames.py builds frames whose need (n symbols
in the largest group, p in the part that holds a noise band, B section bytes) is known from the CPU oracle alone; here every
one of them runs with the caps set to exactly that need and to one step less:

    child                         cap                                   reruns
    HYDAMD_K1_SPLIT=0             r16(n)                                0
                                  r16(n) - 16                           >= 1, token_capacity() == 196608
                                  default, HYDAMD_PAYLOAD_CAP = B       0
                                  default, HYDAMD_PAYLOAD_CAP = B - 1   exactly 1
    default (four parts)          4 r16(p)                              0
                                  4 r16(p) - 64                         >= 1
                                  16 mod 64 and >= n                    0  (the unsplit kernel inside a split process)
    HYDAMD_K1_SPLIT_LOG=1         2 r32(p)                              0
                                  2 r32(p) - 64                         >= 1
    each                          tokens exact and payload exact        0

each under entropy-stage forms 4 and 5, each followed on the same context by another picture and the first one again.
Sections, symbol counts and section bits equal the oracle's in every run.  No expected figure comes from the device.

The split settings are process-wide statics: one child process per setting (python tests/edge_frames.py MODE REPORT), run
one at a time.  A child that dies (by a signal, an abort, an error of the device) or runs out of time stops the module: the
runs it did not reach fail, and no later child is started."""
import hashlib
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import has_gpu, reference_expected

import edge_frames as ef

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 240
_state = {"stopped": None, "children": {}}


def _child(mode, tmp_path_factory):
    """The report of child `mode`, which runs once (at the first test that asks for it)."""
    if mode in _state["children"]:
        return _state["children"][mode]
    if _state["stopped"]:
        pytest.fail(f"not run: child {_state['stopped']} died or timed out before it")
    report = str(tmp_path_factory.mktemp(f"edges_{mode}") / "report.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("HYDAMD_")}
    env.update(ef.MODES[mode][0], PYTHONPATH=ROOT)
    t0 = time.time()
    died, out, err = None, "", ""
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edge_frames.py"), mode, report],
                           capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT_S, cwd=ROOT)
        out, err = r.stdout, r.stderr
        if r.returncode != 0:   # a signal, an abort, or an error the device reported: the child records a wrong byte, it
            died = f"status {r.returncode}"   # does not raise for it, so whatever ended it early was not a comparison
        code = r.returncode
    except subprocess.TimeoutExpired as e:
        died, code = f"no end after {CHILD_TIMEOUT_S} s", None
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
    if died:
        _state["stopped"] = mode
    rep = {"runs": {}, "api": {}}
    if os.path.exists(report):
        with open(report) as f:
            rep = json.load(f)
    last = [line for line in out.splitlines() if line.startswith("CASE ")][-1:]
    rep.update(died=died, code=code, last=last, tail=err[-3000:], wall=time.time() - t0)
    print(f"\n  child {mode}: {len(rep['runs'])} runs in {rep['wall']:.1f} s, exit {code}")
    _state["children"][mode] = rep
    return rep


def _entry(rep, section, key):
    if key not in rep[section]:
        pytest.fail(f"{key} did not run: child {rep.get('mode')} ended with {rep['died'] or rep['code']} in {rep['last']}\n"
                    f"{rep['tail']}")
    return rep[section][key]


RUNS = [(mode, frame) for mode in ef.MODES for frame in ef.FRAMES[mode]]


@pytest.mark.parametrize("mode,frame", RUNS, ids=[f"{m}-{f}" for m, f in RUNS])
def test_exact_fit_and_one_step_short(tmp_path_factory, mode, frame):
    c = ef.case(frame, ef.band_plog(mode))
    assert ef.preconditions(mode, c) == []          # the oracle is the authority, here as on the CPU
    other = ef.second_image(c.img)
    other_res, _ = ef.orc.encode_lf_group(other)
    want = {"first": hashlib.md5(c.res.stream).hexdigest(), "second": hashlib.md5(other_res.stream).hexdigest()}
    want["again"] = want["first"]
    rep = _child(mode, tmp_path_factory)
    checked = 0
    for name, tok, pay, (low, high) in ef.plan(mode, c):
        for form in ef.FORMS:
            key = f"{frame}/{name}/form{form}"
            got = _entry(rep, "runs", key)
            where = f"{mode}/{key} (n {c.n}, p {c.p}, B {c.B}, HYDAMD_TOKEN_CAP {tok}, HYDAMD_PAYLOAD_CAP {pay})"
            print(f"  {where}: reruns {[got[s]['reruns'] for s in ('first', 'second', 'again')]}, "
                  f"token capacity {got['first']['token_capacity']}")
            for step in ("first", "second", "again"):
                g = got[step]
                assert g["payload_md5"] == want[step] and g["payload_ok"], f"{where}: sections of the {step} frame"
                assert g["counts_ok"], f"{where}: symbol counts of the {step} frame"
                assert g["bits_ok"], f"{where}: section bits of the {step} frame"
            first = got["first"]
            assert low <= first["reruns"] <= high, f"{where}: {first['reruns']} reruns, expected {low}..{high}"
            if name == "tokens_short":
                assert first["token_capacity"] == ef.TOKENS_PER_GROUP, where
            elif tok is not None:
                assert first["token_capacity"] == tok, where
            if high == 0 and ef.fits(other_res, c.width, c.height, mode, tok, pay):
                # neither the other picture nor the boundary frame's second visit outgrows what the first one fitted
                assert got["again"]["reruns"] == 0, f"{where}: {got['again']['reruns']} reruns by the third frame"
            checked += 1
    assert checked == len(ef.plan(mode, c)) * len(ef.FORMS)


@pytest.mark.parametrize("name", [r[0] for r in ef.API_RUNS])
def test_drop_in_api_at_the_edges(tmp_path_factory, ref_lib, name):
    """Frame A at (tokens exact, payload exact) and frame C at (tokens one step short, payload B - 1) through hyd_send_tile,
    twice each (the second meets the parked context of the first): the file the compiled reference writes."""
    from hydrium_amd import api

    assert reference_expected()
    c, tok, pay = ef.api_caps(name)
    assert ef.preconditions("plog2", c) == []
    want = hashlib.md5(bytes(api.encode_image(ref_lib, c.img.copy(), out_buf_size=1 << 22))).hexdigest()
    rep = _child("plog2", tmp_path_factory)
    for form in ef.FORMS:
        got = _entry(rep, "api", f"{name}/form{form}")
        assert got == [want, want], f"{name} form {form} (HYDAMD_TOKEN_CAP {tok}, HYDAMD_PAYLOAD_CAP {pay}): file differs"


def test_every_child_ran_to_its_end(tmp_path_factory):
    for mode in ef.MODES:
        rep = _child(mode, tmp_path_factory)
        assert not rep["died"] and rep["code"] == 0 and rep.get("done"), (mode, rep["died"], rep["code"], rep["last"], rep["tail"])
