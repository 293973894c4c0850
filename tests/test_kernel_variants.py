"""CPU-only: every build-time and run-time switch is classified (tests/kernel_variants.py), every product build variant
cross-compiles for gfx950 with the resources the design rests on, and the edge corpus (tests/variant_corpus.py) reaches
what it claims to reach.  The variants themselves run on the GPU in tests/test_gpu_variants.py."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kernel_variants as kv  # noqa: E402
import variant_corpus as vc  # noqa: E402


def test_every_build_switch_is_classified():
    found = kv.preprocessor_switches()
    assert not found - kv.classified_build_switches(), \
        f"HYDK_* switches nobody classified (tests/kernel_variants.py): {sorted(found - kv.classified_build_switches())}"
    assert not kv.classified_build_switches() - found, \
        f"classified switches the sources no longer read: {sorted(kv.classified_build_switches() - found)}"
    assert not set(kv.PRODUCT) & set(kv.TIMING_ONLY)
    for name, values in kv.PRODUCT.items():
        assert values, f"{name}: a product switch without a value to test"
    for d in kv.COMBOS.values():
        assert set(d) <= set(kv.PRODUCT)


def test_every_environment_switch_is_classified():
    found = kv.environment_switches()
    loose = sorted(n for n in found if not kv.is_classified_knob(n))
    assert not loose, f"HYDAMD_* settings nobody classified (tests/kernel_variants.py): {loose}"
    listed = set(kv.KNOBS) | set(kv.COVERED) | set(kv.HOOKS)
    assert not listed - found, f"classified settings the sources no longer read: {sorted(listed - found)}"
    assert not set(kv.KNOBS) & set(kv.COVERED)
    for name, where in kv.COVERED.items():
        path, _, test = where.partition("::")
        with open(os.path.join(ROOT, path)) as f:
            src = f.read()
        assert re.search(r"def " + re.escape(test) + r"\b", src), f"{name}: {where} does not exist"
        assert name in src, f"{name}: {path} never names it"


@pytest.mark.parametrize("text,kind", [("#if HYDK_NEW_SWITCH\n#endif\n", "build"), ("#elif defined(HYDK_NEW_SWITCH)\n", "build"),
                                       ('const char *v = getenv("HYDAMD_NEW");\n', "env")])
def test_the_scan_sees_a_new_switch(tmp_path, text, kind):
    """The scanners above are what the completeness tests rest on: a new name in a scratch copy is found."""
    if kind == "build":
        (tmp_path / "x.hip").write_text(text)
        assert kv.preprocessor_switches(str(tmp_path)) == {"HYDK_NEW_SWITCH"}
    else:
        (tmp_path / "x.c").write_text(text)
        assert kv.environment_switches(str(tmp_path)) == {"HYDAMD_NEW"}


def _descriptors(flags, src="kernels.hip"):
    from hydrium_amd import build as hb

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([hb.HIPCC] + hb.HIP_FLAGS + list(flags) + ["--cuda-device-only", "-S", "-o", out, os.path.join(hb.CSRC, "hip", src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        text = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        body = m.group(2)
        res[m.group(1)] = {k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", body).group(1))
                           for k in ("group_segment_fixed_size", "next_free_vgpr", "private_segment_fixed_size")}
    return res


@pytest.fixture(scope="module")
def variant_descriptors():
    """name -> {kernel: descriptor} for the default build and every product variant (device-only -S, compiled in parallel)."""
    from hydrium_amd import build as hb

    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc")
    specs = dict(kv.variants(), default={})
    jobs = []
    for name, d in specs.items():
        flags = [f"-D{k}={v}" for k, v in d.items()]
        jobs.append((name, flags, "kernels.hip"))
        if any(k.startswith("HYDK_LF_") for k in d):
            jobs.append((name, flags, "lf_coder.hip"))
    n = max(1, min(16, int(os.environ.get("MAX_JOBS") or os.cpu_count() or 1)))
    with ThreadPoolExecutor(n) as ex:
        outs = list(ex.map(lambda j: _descriptors(j[1], j[2]), jobs))
    res = {}
    for (name, _, _), o in zip(jobs, outs):
        res.setdefault(name, {}).update(o)
    return res


def _instances(res, prefix):
    hits = {k: v for k, v in res.items() if k.startswith(prefix)}
    assert hits, prefix
    return hits


def _lanes(res, nc):
    return _instances(res, f"_Z12k_rans_lanesILi{nc}E")


def test_every_variant_compiles_and_uses_no_scratch(variant_descriptors):
    assert set(variant_descriptors) == set(kv.variants()) | {"default"}
    for name, res in variant_descriptors.items():
        accepted = kv.SCRATCH_ACCEPTED.get(name, {})
        for k, d in res.items():
            limit = next((b for p, b in accepted.items() if k.startswith(p)), 0)
            assert d["private_segment_fixed_size"] <= limit, (name, k, d)


def test_scratch_accepted_only_where_it_is_used(variant_descriptors):
    """An entry of SCRATCH_ACCEPTED that no longer spills is dropped, so the table does not hide a new spill later."""
    for name, accepted in kv.SCRATCH_ACCEPTED.items():
        for prefix in accepted:
            assert any(d["private_segment_fixed_size"] for k, d in _instances(variant_descriptors[name], prefix).items()), (name, prefix)


def test_dynamic_lds_chain_instances_hold_no_static_lds(variant_descriptors):
    """Under HYDK_CHAIN_DYN_LDS the chain kernel addresses its rows absolutely and traps when its LDS does not start at
    address 0: no static LDS may be laid out in front of the launch's.  And the point of it: no padded allocation."""
    dyn = [n for n, d in kv.variants().items() if d.get("HYDK_CHAIN_DYN_LDS")]
    assert "chain_dyn_lds_1" in dyn and "chanseq_dyn_pipe1" in dyn
    for name in dyn:
        for nc in (9, 3, 2, 1):
            for k, d in _lanes(variant_descriptors[name], nc).items():
                assert d["group_segment_fixed_size"] == 0, (name, k, d)
                assert d["next_free_vgpr"] <= 164, (name, k, d)
    for nc in (9, 3, 2, 1):  # and the default build keeps its static LDS (the trap's premise is the #if, not luck)
        assert all(d["group_segment_fixed_size"] > 0 for d in _lanes(variant_descriptors["default"], nc).values())


def test_chanseq_transform_lds(variant_descriptors):
    """The point of HYDK_K1_CHANSEQ: 21 granules per transform workgroup instead of 25 for 8- and 16-bit samples.  (The float
    instance is not held to it: it grows under CHANSEQ, 33 008 -> 39 152 bytes.)"""
    for name, d in kv.variants().items():
        if d.get("HYDK_K1_CHANSEQ"):
            for fmt in (0, 1):  # HYDK_FMT_U8, HYDK_FMT_U16
                for k, desc in _instances(variant_descriptors[name], f"_Z20k_transform_tokenizeILi{fmt}E").items():
                    assert desc["group_segment_fixed_size"] <= 21 * 1280, (name, k, desc)


def test_table_in_global_memory_leaves_the_chain_6kb_of_lds(variant_descriptors):
    for name, d in kv.variants().items():
        if d.get("HYDK_LANE_TAB_GLOBAL"):
            for nc in (9, 3, 2, 1):
                for k, desc in _lanes(variant_descriptors[name], nc).items():
                    assert desc["group_segment_fixed_size"] <= 6 * 1024, (name, k, desc)


# ---- the edge corpus ----------------------------------------------------------------------------------------------------
def test_corpus_reaches_the_largest_tokens():
    """Through the oracle: the DCT-basis sign pattern drives the integer path to token 28 (the synthetic kinds stop at 26),
    the primaries to the LF ints' extremes, the 16-bit extremes to both branches of the transfer curve."""
    from oracle import binding as orc

    tops = {}
    for n, kind, w, h, d, _ in vc.FILE_IMAGES:
        if kind in vc.EDGE_KINDS:
            res, _ = orc.encode_lf_group(vc.image(kind, w, h, d))
            tops[n] = (int(res.symbols["token"].max()), int(np.abs(res.quant).max()), int(np.abs(res.dc).max()))
    assert max(t for t, _, _ in tops.values()) >= 28, tops
    assert tops["basis_grey16_256"][0] >= 28 and tops["basis_grey8_256"][0] >= 28, tops
    assert tops["basis_grey16_256"][1] >= 512, tops
    assert tops["primaries16_264x200"][2] >= 800, tops
    for n, *_ in vc.STAGE_IMAGES:
        assert n in ("photo_256", "basis_grey16_256")
    ext = vc.image("extremes16", 300, 260, 16)
    assert {0, 1, 65534, 65535} <= set(np.unique(ext).tolist())
    assert ((ext >= 2640) & (ext <= 2650)).any() and ((ext >= 2651) & (ext <= 2661)).any()


def test_corpus_case_list_is_stable():
    names = vc.case_names()
    assert len(names) == len(set(names))
    assert sum(n.startswith("file_") for n in names) == len(vc.FILE_IMAGES) * len(vc.FORMS)
    assert sum(n.startswith("golden_") for n in names) >= 10
