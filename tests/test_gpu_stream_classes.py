"""GPU: contexts in the runtime's three queue pools (csrc/host/streamclass.c, hydamd_stream_class) code what they coded
in one.  Every case is a process of its own (tests/stream_class_client.py) with its own GPU_MAX_HW_QUEUES: the runtime
reads it once."""
import os
import subprocess
import sys

import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

HERE = os.path.dirname(os.path.abspath(__file__))


def client(queues, *args, **extra):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(queues), PYTHONPATH=os.path.dirname(HERE), **extra)
    if "HYDAMD_STREAM_HIGH" not in extra:
        env.pop("HYDAMD_STREAM_HIGH", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "stream_class_client.py"), *map(str, args)], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    classes = [int(x) for x in next(l for l in lines if l.startswith("classes ")).split()[1:]]
    return classes, lines


def test_thirteen_contexts_on_four_queues_code_the_same_bytes():
    classes, lines = client(4, "rounds", 13, 13)
    assert classes == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 0]
    assert "same sections 13" in lines and "same file" in lines


def test_stream_high_knob_keeps_precedence():
    classes, lines = client(4, "rounds", 6, 2, HYDAMD_STREAM_HIGH="16")
    assert classes == [1] * 6
    assert "same sections 2" in lines and "same file" in lines


def test_every_context_is_normal_on_twenty_two_queues():
    classes, _ = client(22, "classes", 13)
    assert classes == [0] * 13


def test_a_destroyed_contexts_slot_and_class_are_reused():
    classes, lines = client(4, "reuse")
    assert classes == [0, 0, 0, 0, 1, 1, 1]
    assert "same file" in lines
