"""The host library's one owner of device and pinned memory (fleet_amd/csrc/dev_mem.h) without
a GPU: tests/native/check_dev_mem.cpp defines the HIP allocation calls itself over malloc
and checks scope exit, moves, the grow policies, retiring, every failure point of a create
chain and a failing zero-fill; it is built and run stand-alone, plainly and under the host
sanitizers. And the rule that keeps the ownership in one place: no other unit of the
library calls the four allocation functions."""
import glob
import os
import shutil
import subprocess

import pytest

from fleet_amd.build import SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fleet_amd", "csrc")


def _rocm_include():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    return inc if os.path.exists(os.path.join(inc, "hip", "hip_runtime_api.h")) else "/opt/rocm/include"


def build_checker(tmp_path_factory, flags):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler for dev_mem.h")
    exe = tmp_path_factory.mktemp("native") / "check_dev_mem"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{_rocm_include()}", *flags,
           os.path.join(ROOT, "tests", "native", "check_dev_mem.cpp"), "-o", str(exe)]
    return cmd, str(exe)


def run_checker(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ALL OK" in r.stdout


def test_owners_against_the_fake_allocator(tmp_path_factory):
    cmd, exe = build_checker(tmp_path_factory, [])
    subprocess.check_call(cmd)
    run_checker(exe)


def test_owners_against_the_fake_allocator_under_sanitizers(tmp_path_factory):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    cmd, exe = build_checker(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitizer" in r.stderr.lower()):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-4000:]
    run_checker(exe)


def test_allocation_calls_live_in_dev_mem_only():
    """Every unit of the library and every header of csrc: the four allocation functions are
    called in dev_mem.h and nowhere else (comments and strings included)."""
    units = [os.path.join(CSRC, s) for s, _ in SOURCES]
    files = sorted(set(units + glob.glob(os.path.join(CSRC, "*.h"))))
    assert len(units) >= 15 and os.path.join(CSRC, "dev_mem.h") in files
    for f in files:
        src = open(f).read()
        for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree("):
            if os.path.basename(f) == "dev_mem.h":
                assert call in src, call
            else:
                assert call not in src, f"{os.path.relpath(f, ROOT)} calls {call}...)"
