"""CPU-only: bench.py's plain-run options.  --steps is checked, --dump-outputs is frame mode only, and dump_outputs writes
the frame it is asked for, as float32 / float64 .npy files within its byte budget (a seeded sample where the budget does
not hold a stream), the same files every time."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from hydrium_amd import device  # noqa: E402


def _bench(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=120)


def test_steps_below_one_and_dumps_outside_frame_mode_are_refused():
    r = _bench("--steps", "0")
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr
    r = _bench("--mode", "shard", "--dump-outputs", "x")
    assert r.returncode != 0 and "frame mode only" in r.stderr
    assert "--full" in _bench("--help").stdout


def test_dump_sample_is_whole_when_it_fits_and_a_fixed_spread_sample_when_not():
    data = (np.arange(10_000) * 7 % 251).astype(np.uint8)
    whole = bench.dump_sample(data, 10_000)
    assert whole.dtype == np.float32 and np.array_equal(whole, data)
    a, b = bench.dump_sample(data, 1000), bench.dump_sample(data, 1000)
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    assert np.isin(a, data).all()


class _Ctx:
    """A context that holds `frames` frames of `lfg` LF groups: frame f's sections are bytes of value f + 1."""

    def __init__(self, frames, lfg, section_bytes):
        self.frames, self.lfg, self.n = frames, lfg, section_bytes

    def sync(self):
        pass

    def read_sections(self, slot):
        bits = np.zeros(64, np.int64)
        bits[0] = self.n * 8 // self.lfg
        return bits, np.zeros(64, np.int64)

    def read_payload(self):
        return b"".join(bytes([f + 1]) * (self.n // self.lfg * self.lfg) for f in range(self.frames))

    def read_lf_streams(self, count, first=0):
        out = np.zeros(count, device.LF_INFO_DTYPE)
        out["bit_count"] = 16
        out["offset"] = np.arange(count) * 2
        out["lengths"] = np.arange(count)[:, None] % 7
        return out

    def read_lf_payload(self):
        return np.repeat(np.arange(1, self.frames + 1, dtype=np.uint8), 2 * self.lfg)


@pytest.mark.parametrize("budget", [64 << 20, 1 << 16])
def test_dump_outputs_writes_the_asked_frame_within_the_budget(tmp_path, monkeypatch, budget):
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    ctx = _Ctx(frames=2, lfg=4, section_bytes=40_000)
    names = bench.dump_outputs(str(tmp_path / "a"), ctx, 2, 1, 4)
    bench.dump_outputs(str(tmp_path / "b"), ctx, 2, 1, 4)
    assert names == sorted(os.listdir(tmp_path / "a"))
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in names)
    assert total <= budget
    arrays = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n, a in arrays.items():
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy")))
    assert (arrays["hf_sections"] == 2).all() and (arrays["lf_streams"] == 2).all()  # frame 1's bytes only
    assert arrays["hf_section_bits"].shape == (4, 64) and arrays["lf_code_lengths"].shape == (4, 384)
    if budget == 64 << 20:  # frame 1's 40 000 section bytes fit: all of them
        assert len(arrays["hf_sections"]) == 40_000 and len(arrays["lf_streams"]) == 8
    else:
        assert 0 < len(arrays["hf_sections"]) < 40_000
