"""CPU-only: what the two fused launches of the frame loop ask of a compute unit, read from the code objects hipcc
cross-compiles here.

k_build_tables carries the LF coder's token workgroups and k_rans_emit<true> its pack workgroups (lf_windows.h).  A fused
kernel's static LDS is one buffer that each role views as its own, so it must be the LARGER of its roles' needs and not
their sum, and neither role may make the other spill.  The roles alone are measured in the same compile: k_lf_tokens and
k_lf_pack of lf_coder.hip are the token and the pack role as kernels of their own.  The table and the emit role alone are
the kernels of the commit before the fusion, whose descriptors read (same compiler, same flags):
    k_build_tables    group_segment_fixed_size 28596 (its own arrays 25388 + the code builder's 3204, summed), 81 VGPRs, no scratch
    k_rans_emit<true> group_segment_fixed_size  8256 (four wavefronts' windows of 516 words), 74 VGPRs, no scratch"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENT_TABLES_LDS = 28596
PARENT_EMIT_LDS = 8256


def _descriptors(src):
    from hydrium_amd import build as hb

    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([hb.HIPCC] + hb.HIP_FLAGS + ["--cuda-device-only", "-S", "-o", out, os.path.join(hb.CSRC, "hip", src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        text = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        res[m.group(1)] = {k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", m.group(2)).group(1))
                           for k in ("group_segment_fixed_size", "next_free_vgpr", "private_segment_fixed_size")}
    return res


def _one(res, pattern):
    hits = [v for k, v in res.items() if re.search(pattern, k)]
    assert len(hits) == 1, (pattern, [k for k in res if re.search(pattern, k)])
    return hits[0]


def test_a_fused_kernel_asks_for_the_larger_role_not_the_sum():
    kernels, lf = _descriptors("kernels.hip"), _descriptors("lf_coder.hip")
    tokens, pack = _one(lf, r"11k_lf_tokensE"), _one(lf, r"9k_lf_packE")
    tables, emit = _one(kernels, r"^_Z14k_build_tables"), _one(kernels, r"^_Z11k_rans_emitILb1EE")
    print(f"  tokens {tokens}\n  pack {pack}\n  tables + tokens {tables}\n  emit + pack {emit}")
    for d in (tokens, pack, tables, emit):
        assert d["private_segment_fixed_size"] == 0, d
    assert tables["group_segment_fixed_size"] <= max(PARENT_TABLES_LDS, tokens["group_segment_fixed_size"]), tables
    assert emit["group_segment_fixed_size"] <= max(PARENT_EMIT_LDS, pack["group_segment_fixed_size"]), emit
    # the emit role alone (frames with a wave-form range keep it) carries no pack role and no more LDS than before
    plain = _one(kernels, r"^_Z11k_rans_emitILb0EE")
    assert plain["group_segment_fixed_size"] <= PARENT_EMIT_LDS and plain["private_segment_fixed_size"] == 0, plain
