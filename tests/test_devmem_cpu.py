"""Device memory of the host layer on the CPU: the owning DevBuf, the TableCache protocol of
csrc/asw_devmem.h and the destructor of asw_ctx, through stand-alone programs of tests/cpp that define the few HIP runtime calls
involved themselves (tests/cpp/devmem_fake_hip.h).  Nothing of the HIP runtime is linked and no GPU is touched; the programs run
under AddressSanitizer and UndefinedBehaviorSanitizer, which is what turns a host table that died before its copy ran, a double free
or a leaked block into a failure."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shim_build import PKG, build_demo  # noqa: E402

FLAGS = ("-Wextra", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(PKG, "csrc"), "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def run(exe, *args):
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cache_exe(tmp_path_factory):
    return build_demo("devmem_cache.cpp", tmp_path_factory.mktemp("devmem") / "devmem_cache", link=False, extra=FLAGS)


def test_context_frees_everything_it_holds(tmp_path):
    exe = build_demo("devmem_ownership.cpp", tmp_path / "devmem_ownership", link=False, extra=FLAGS)
    r = run(exe)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"live (\d+) mallocs (\d+) frees (\d+) streams (\d+) events (\d+)\n", r.stdout)
    assert m, r.stdout
    live, mallocs, frees, streams, events = map(int, m.groups())
    assert mallocs > 40  # every buffer-bearing member, 4 frames' worth of slots, scratch
    assert live == 0 and frees == mallocs
    assert streams == 0 and events == 0


def test_devbuf_contract_and_cache_protocol(cache_exe):
    r = run(cache_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["ensure contract ok: 5 allocations, 5 frees", "cache protocol ok: 9 builds"]


def test_fake_catches_a_host_table_that_died_before_the_wait(cache_exe):
    """the deferred copy is what gives the protocol test its teeth: waiting after the host data is gone must not go unnoticed"""
    r = run(cache_exe, "dead-host-table")
    assert r.returncode != 0 and "heap-use-after-free" in r.stderr and "went unnoticed" not in r.stdout, r.stdout + r.stderr
