"""GPU: every product build variant and every run-time A/B setting of tests/kernel_variants.py against the reference.

One child process per variant and per setting (most settings are read once into a static; a process that loaded one build
of libhydrium.so.0 may be handed it again for another), run ONE AT A TIME: the child proves from /proc/self/maps which
library it mapped, runs the corpus of tests/variant_corpus.py and writes a report.  The expected bytes are computed here,
once, from the compiled reference.  A child that crashes or times out stops the module: no later child is started."""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import has_gpu

import kernel_variants as kv
import variant_corpus as vc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 180
_state = {"stopped": None}


def _runs():
    """(test id, library, extra environment): the variants, then the A/B settings on the shipped library."""
    out = [(f"build-{n}", n, {}) for n in kv.variants()]
    out += [(f"env-{k}={v}", None, {k: v}) for k, v in kv.knob_settings()]
    return out


@pytest.fixture(scope="module")
def corpus(ref_lib, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("variant_corpus"))
    return d, vc.prepare(d, ref_lib)


@pytest.fixture(scope="module")
def libraries():
    from hydrium_amd import build as hb

    t0 = time.time()
    paths = hb.build_variants(kv.variants())
    paths[None] = os.path.realpath(hb.LIB_PATH)
    assert os.path.exists(paths[None]), "the shipped library is not built"
    print(f"variants ready in {time.time() - t0:.1f} s")
    return paths


@pytest.mark.parametrize("run_id,variant,extra", _runs(), ids=[r[0] for r in _runs()])
def test_variant_matches_the_reference(corpus, libraries, capsys, tmp_path, run_id, variant, extra):
    if _state["stopped"]:
        pytest.skip(f"not run: child {_state['stopped']} crashed or timed out before it")
    corpus_dir, spec = corpus
    lib = libraries[variant]
    report = str(tmp_path / "report.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("HYDAMD_")}
    env.update(extra, HYDAMD_LIB=lib, PYTHONPATH=ROOT)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "variant_corpus.py"), corpus_dir, report],
                           capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT_S, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _state["stopped"] = run_id
        pytest.fail(f"{run_id}: timed out after {CHILD_TIMEOUT_S} s\n{e.stdout or ''}\n{e.stderr or ''}")
    wall = time.time() - t0
    if r.returncode < 0 or r.returncode in (134, 139):
        _state["stopped"] = run_id
        pytest.fail(f"{run_id}: child died with status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}")
    assert os.path.exists(report), f"{run_id}: no report (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(report) as f:
        rep = json.load(f)
    cases = rep["cases"]
    top = max((c.get("token_max") or 0 for c in cases), default=0)
    with capsys.disabled():
        print(f"\n  {run_id}: {rep['mapped']} {len(cases)}/{len(spec['cases'])} cases, token max {top}, {wall:.1f} s")
    assert rep["mapped"] == [os.path.realpath(lib)], rep.get("error")
    assert rep.get("mapped_after") == [os.path.realpath(lib)], rep.get("mapped_after")
    assert r.returncode == 0, f"{run_id}: exit {r.returncode}: {[c for c in cases if not c['ok']]}\n{r.stderr[-4000:]}"
    assert [c["case"] for c in cases] == spec["cases"], "the child did not run the whole corpus"
    wrong = [(c["case"], c["md5"], spec["expect"][c["case"]]) for c in cases
             if c["case"] in spec["expect"] and c["md5"] != spec["expect"][c["case"]]]
    assert not wrong, f"{run_id}: bytes differ from the reference: {wrong}"
    assert all(c["ok"] for c in cases)
    assert top >= 28, f"{run_id}: no case reached token 28 ({top})"
