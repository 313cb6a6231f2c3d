"""Streams and events of a call on the CPU: the side-stream scope and the call clock of
csrc/asw_streams.h through the stand-alone program tests/cpp/streams_scope.cpp, against the fake runtime of
tests/cpp/devmem_fake_hip.h, which logs every event call with its stream and event.  Nothing of the HIP runtime is linked and no GPU
is touched; the program runs under AddressSanitizer and UndefinedBehaviorSanitizer and asserts each case itself: the lines below are
the calls it logged, "<call> <event> <stream>"."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shim_build import build_demo  # noqa: E402
from test_devmem_cpu import FLAGS  # noqa: E402

FORK = "record fork main"
JOIN0 = "record j0 side0, wait j0 main"
JOIN1 = "record j1 side1, wait j1 main"
EXPECTED = [
    "one side: %s, wait fork side0, %s" % (FORK, JOIN0),
    "both sides: %s, wait fork side0, wait fork side1, %s, %s" % (FORK, JOIN0, JOIN1),
    "side 1 first: %s, wait fork side1, wait fork side0, %s, %s" % (FORK, JOIN0, JOIN1),
    "never used: nothing",
    "left open: " + JOIN1,  # the destructor's join: side 1 alone
    "joined twice, then left: " + JOIN0,
    "fork record fails: nothing",
    "fork wait fails: " + FORK,
    "join record fails: " + JOIN1,  # side 0's record failed: ASW_ERR_HIP, side 1 joined all the same
    "clock: record total0 main, record agg0 main, record agg1 main, record total1 main, stream-sync - main",
    "clock, no wait: record total1 main",
    "marks: record agg0 main, record agg1 main",
    "added step: record total0 main, record total1 main, sync total1 -",  # the step's stop event, not the stream
    "added step fails: record total0 main",
    "ok",
]


def test_side_stream_scope_and_call_clock(tmp_path):
    exe = build_demo("streams_scope.cpp", tmp_path / "streams_scope", link=False, extra=FLAGS)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == EXPECTED
