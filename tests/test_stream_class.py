"""The placement rule of the contexts' own streams (csrc/host/streamclass.c), without a device: the text of
GPU_MAX_HW_QUEUES to a pool size, a live context's index to its queue pool, and the per-device table that hands out the
lowest free index — through the test flavour of the library, and once more as a stand-alone program under the host
sanitizers (address + undefined behaviour, and thread)."""
import ctypes as C
import os
import subprocess
import threading

import pytest

from hydrium_amd import build as hbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, L = 0, 1, 2


@pytest.fixture(scope="module")
def d():
    hbuild.build()
    d = C.CDLL(hbuild.HOSTTEST_PATH)
    d.hyd_queue_pool_size.argtypes = [C.c_char_p]
    d.hyd_stream_class.argtypes = [C.c_int, C.c_int]
    d.hyd_stream_slot_take.argtypes = [C.c_int]
    d.hyd_stream_slot_release.argtypes = [C.c_int, C.c_int]
    d.hyd_stream_slot_release.restype = None
    return d


@pytest.mark.parametrize("text,pool", [(None, 4), (b"", 4), (b"abc", 4), (b"0", 4), (b"4", 4), (b"22", 22)])
def test_pool_size_from_the_environment_text(d, text, pool):
    assert d.hyd_queue_pool_size(text) == pool


def test_sixteen_contexts_on_pools_of_four(d):
    assert [d.hyd_stream_class(i, 4) for i in range(16)] == [N] * 4 + [H] * 4 + [L] * 4 + [N] * 4


@pytest.mark.parametrize("pool", [9, 22])
def test_every_context_is_normal_above_eight_queues(d, pool):
    assert [d.hyd_stream_class(i, pool) for i in range(64)] == [N] * 64


def test_no_change_up_to_one_pool_of_contexts(d):
    for pool in range(1, 9):
        assert [d.hyd_stream_class(i, pool) for i in range(pool)] == [N] * pool
        assert d.hyd_stream_class(pool, pool) == H


def test_a_returned_slot_is_the_next_one_handed_out(d):
    dev = 5  # a table no other test of this process uses
    assert [d.hyd_stream_slot_take(dev) for _ in range(5)] == [0, 1, 2, 3, 4]
    d.hyd_stream_slot_release(dev, 1)
    d.hyd_stream_slot_release(dev, 3)
    assert [d.hyd_stream_slot_take(dev) for _ in range(2)] == [1, 3]
    assert d.hyd_stream_slot_take(dev) == 5


def test_eight_threads_never_hold_one_slot_twice(d):
    dev = 6
    held, twice = set(), []
    lock = threading.Lock()

    def work():
        for _ in range(1000):
            i = d.hyd_stream_slot_take(dev)  # (ctypes drops the interpreter lock for the call)
            with lock:
                if i < 0 or i in held:
                    twice.append(i)
                held.add(i)
            with lock:
                held.discard(i)
            d.hyd_stream_slot_release(dev, i)

    ts = [threading.Thread(target=work) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not twice and not held
    assert d.hyd_stream_slot_take(dev) == 0


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_the_rule_alone_under_host_sanitizers(tmp_path, sanitizers):
    """csrc/host/streamclass.c and tests/c/streamclass_main.c: a stand-alone host program, nothing loaded into python"""
    exe = str(tmp_path / "streamclass_main")
    cmd = [hbuild.CC, "-std=c11", "-O1", "-g", "-Wall", "-Wextra", f"-fsanitize={sanitizers}", "-fno-sanitize-recover=all",
           f"-I{os.path.join(hbuild.CSRC, 'host')}", os.path.join(ROOT, "tests", "c", "streamclass_main.c"),
           os.path.join(hbuild.CSRC, "host", "streamclass.c"), "-o", exe, "-lpthread"]
    made = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert made.returncode == 0 and not made.stderr, made.stderr  # no warning either
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert (ran.returncode, ran.stdout, ran.stderr) == (0, "ok\n", ""), (ran.stdout, ran.stderr)
