"""What the code can be switched to, in one table (data and small helpers; no tests here).

Build-time switches: every HYDK_* name a preprocessor conditional of hydrium_amd/csrc/hip/*.hip reads.
  PRODUCT       must give the reference's bytes: every non-default value listed here is built, cross-compiled and run
                (tests/test_kernel_variants.py on the CPU, tests/test_gpu_variants.py on the GPU);
  TIMING_ONLY   wrong bytes by design (measurement builds): never run by the tests;
  NOT_SWITCHES  include guards and format constants.
Run-time switches: every HYDAMD_* name the sources under hydrium_amd/csrc read from the environment.
  KNOBS         product A/B settings ("same bytes"): each setting is run in a fresh process by tests/test_gpu_variants.py;
  COVERED       configuration tested elsewhere: the test that sets it;
  HOOKS         test and measurement hooks (HYD_TEST_HOOKS flavour, tracing).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "hydrium_amd", "csrc", "hip")
CSRC = os.path.join(ROOT, "hydrium_amd", "csrc")

# name -> the non-default values to build (the default is what kernels.hip / lf_coder.hip define)
PRODUCT = {
    "HYDK_CHAIN_DYN_LDS": [1],        # the chain's LDS asked for at launch (never defaulted: read by #if only)
    "HYDK_LANE_PIPE": [0, 1],
    "HYDK_LANE_STEP": [2],
    "HYDK_K1_CHANSEQ": [1],
    "HYDK_K1_TRIM": [1, 3],           # bit 0: 32-bit record offsets; bit 1: block bitmaps through LDS (2 compiles as 3)
    "HYDK_K1_ILP": [0, 1, 4],         # pixels per lock step: must divide 8
    "HYDK_K1_WAVELOCAL": [0],
    "HYDK_K1_GATHER": [0, 0x3F],      # no curve from the table / all six
    "HYDK_K1_WAVES": [5],
    "HYDK_LANE_TAB_GLOBAL": [1],
    "HYDK_CHAIN_LDS_MIN": [83200],    # 65 granules: one nine-cluster chain per compute unit
    "HYDK_CHAIN_HOG": [1],
    "HYDK_CHAIN_PRIO": [0],
    "HYDK_K1_PRIO": [2],
    "HYDK_EMIT_SHARE_DEFAULT": [5],
    "HYDK_LF_WPB": [3],               # 3 does not divide the 220 windows of an LF group
}
# combinations built as variants of their own (name -> defines)
COMBOS = {
    "chanseq_dyn_pipe1": {"HYDK_K1_CHANSEQ": 1, "HYDK_CHAIN_DYN_LDS": 1, "HYDK_LANE_PIPE": 1},  # VERDICT's next default
    "pipe0_step2": {"HYDK_LANE_PIPE": 0, "HYDK_LANE_STEP": 2},  # (PIPE=0 with STEP=1, the default step, is lane_pipe_0)
    "dyn_tabglobal": {"HYDK_CHAIN_DYN_LDS": 1, "HYDK_LANE_TAB_GLOBAL": 1},
}
# kernels that may use scratch in a variant: variant -> {mangled-name prefix: bytes accepted}.  HYDK_K1_WAVES=5 leaves the
# transform kernel 102 registers: five of its instances spill 60 bytes.  Slower, not wrong - it is run like every other.
SCRATCH_ACCEPTED = {
    "k1_waves_5": {"_Z20k_transform_tokenize": 64},
}

TIMING_ONLY = {
    "HYDK_K1_SKIP": "leaves stages of the transform kernel out",
    "HYDK_CHAIN_PROBE": "chain kernel without bank conflicts / traffic / stores, or with clocks in the section sizes",
    "HYDK_LANE_NC9_PROBE": "nine-cluster frames on a smaller table instance",
    "HYDK_LF_PROBE": "LF kernels without priorities / histograms / records",
}
NOT_SWITCHES = {
    "HYDK_ASSEMBLE_H_": "include guard",
    "HYDK_COMMON_H_": "include guard",
    "HYDK_SECTIONS_H_": "include guard",
    "HYDK_LF_HUFFMAN_H_": "include guard",
    "HYDK_LF_CODES": "format constant (LF alphabet size)",
    "HYDK_LF_RUN_BASE": "format constant (LF run-length symbol base)",
}

KNOBS = {
    "HYDAMD_EMIT_SHARE": ["3", "5", "16"],      # virtual blocks per emit workgroup: 3 and 5 do not divide 16
    "HYDAMD_LF_CODES_RIDE": ["tables"],
    "HYDAMD_WAVE_FORM_EMITS": ["1"],
    "HYDAMD_HOST_ASSEMBLY": ["1"],
    "HYDAMD_STAGED_READBACK": ["0"],
    "HYDAMD_CURVE_GATHERS": ["1", "2"],
    "HYDAMD_XYB_MODE": ["1", "2"],
    "HYDAMD_CONTEXT_CACHE": ["0", "1"],
    "HYDAMD_CONTEXT_CACHE_MB": ["0"],
    "HYDAMD_STAGE_THREADS": ["1", "3"],
    "HYDAMD_STREAM_HIGH": ["16"],
    "HYDAMD_EVENT_SCOPE": ["device"],
    "HYDAMD_K1_SPLIT": ["0"],
}
COVERED = {
    # (far from the edge as well: test_gpu_device_parity.py::test_frame_that_outgrows_its_buffers_is_rerun_transparently,
    # test_gpu_api_parity.py::test_tile_frame_rerun_for_overflow_after_its_results_were_staged)
    "HYDAMD_TOKEN_CAP": "tests/test_gpu_buffer_edges.py::test_exact_fit_and_one_step_short",
    "HYDAMD_PAYLOAD_CAP": "tests/test_gpu_buffer_edges.py::test_exact_fit_and_one_step_short",
    "HYDAMD_DEVICES": "tests/test_gpu_multi_device.py::test_c_client_unchanged_runs_on_the_device_list",
    "HYDAMD_DEVICE": "tests/test_gpu_multi_device.py::test_c_client_unchanged_runs_on_the_device_list",
    "HYDAMD_SHARD_MIN_LF_GROUPS":
        "tests/test_gpu_multi_device.py::test_small_frames_stay_on_one_device_and_encoders_take_devices_in_turn",
    "HYDAMD_VERIFY_PEERS":
        "tests/test_gpu_multi_device.py::test_verify_peers_checks_every_shards_view_and_names_the_pair_that_differs",
    "HYDAMD_TILE_PIPELINE": "tests/test_gpu_api_parity.py::test_tile_mode_default_timing_is_the_reference_s",
    "HYDAMD_EAGER": "tests/test_gpu_api_parity.py::test_sample_format_may_change_between_tiles",
    "HYDAMD_COPY_STREAMS": "tests/test_gpu_api_parity.py::test_upload_streams_shared_by_the_contexts_of_a_device",
    "HYDAMD_RANS_WAVES": "tests/test_gpu_fuzz.py::test_seeded_sweep_against_the_reference",
    "HYDAMD_K1_SPLIT_SLOTS": "tests/test_gpu_device_parity.py::test_splitting_every_transform_launch_never_changes_a_byte",
    "HYDAMD_K1_SPLIT_LOG": "tests/test_gpu_device_parity.py::test_splitting_every_transform_launch_never_changes_a_byte",
    "HYDAMD_LF_CODER": "tests/test_gpu_lf_coder.py::test_api_bytes_identical_with_host_lf_coder",
}
HOOK_PREFIXES = ("HYDAMD_DEBUG_", "HYDAMD_TEST_")
HOOKS = {"HYDAMD_TRACE": "device errors on stderr"}


def _value_name(v):
    return f"{v:x}" if isinstance(v, int) and v > 9 and v & 0xF == 0xF else str(v)


def variants():
    """variant name -> {define: value}: one per non-default value of every product switch, then the combinations."""
    out = {}
    for name, values in PRODUCT.items():
        for v in values:
            out[f"{name[5:].lower()}_{_value_name(v)}"] = {name: v}
    out.update(COMBOS)
    return out


def knob_settings():
    """(name, value) of every run-time A/B setting, one fresh process each."""
    return [(k, v) for k, vals in KNOBS.items() for v in vals]


_PP = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)


def preprocessor_switches(hip_dir=HIP_DIR):
    """Every HYDK_* name a preprocessor conditional of the HIP sources reads."""
    names = set()
    for f in sorted(os.listdir(hip_dir)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(hip_dir, f)) as fh:
                for m in _PP.finditer(fh.read()):
                    names.update(re.findall(r"\bHYDK_[A-Z0-9_]+", m.group(1)))
    return names


_ENV = re.compile(r"\b(?:getenv|env_int)\s*\(\s*\"(HYDAMD_[A-Z0-9_]+)\"")


def environment_switches(csrc=CSRC):
    """Every HYDAMD_* name the native sources read from the environment."""
    names = set()
    for base, _, files in os.walk(csrc):
        for f in files:
            if f.endswith((".hip", ".h", ".c", ".cpp")):
                with open(os.path.join(base, f)) as fh:
                    names.update(_ENV.findall(fh.read()))
    return names


def classified_build_switches():
    return set(PRODUCT) | set(TIMING_ONLY) | set(NOT_SWITCHES)


def is_classified_knob(name):
    return name in KNOBS or name in COVERED or name in HOOKS or name.startswith(HOOK_PREFIXES)
