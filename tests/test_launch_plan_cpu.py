"""The launch plan without a GPU.

tests/native/check_launch.hip includes kernels.hip whole with hipLaunchKernelGGL redefined
as a recorder, calls launch_update, launch_update_encode and launch_update_kardam over
every size, row count, window, plan spec and three CU counts, and prints what each would
launch: kernel, grid, block and every argument. tests/golden/launch_plan.txt is that
output recorded from the tree before launch_plan.h / launch_plan.cpp existed (one FNV-1a
hash per (spec, CUs, launcher) block, the default spec's 256-CU, M = 64 lines in full), so
the planner is held to the launchers it replaced. `check_launch --dump SPEC CUS` prints a
block's lines, to diff two trees when a hash differs.

launch_plan.cpp is plain C++: it is also built with g++ under the address and
undefined-behaviour sanitizers behind a small main and run.
"""
import os
import re
import shutil
import subprocess

import pytest

import test_capi_cpu as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "fleet_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SAN_MAIN = r"""
#include <cstdio>
#include "launch_plan.h"
int main() {
  fleet::PlanOverrides o;
  std::string norm, err;
  int bad = 0;
  for (const char* s : {"", " update=pipe ;fused=off,stage_threads=3", "tile=weave6,flat_w2=64,tile_enc_prio=auto"})
    bad += fleet::parse_plan(s, &o, &norm, &err) != 0;
  for (const char* s : {"update=fast", "grid", "stage_pieces=0", "flat_w2=65", "tile_enc_rows=9999999", "=", "a=b=c"})
    bad += fleet::parse_plan(s, &o, &norm, &err) == 0 || err.empty();
  bad += fleet::set_plan_overrides("grid=balanced", &err) != 0 || fleet::plan_spec() != "grid=balanced";
  for (long long g : {0LL, 1LL, 1000LL, 20000LL, 50000LL, 70000LL, 349526LL, 1LL << 40})
    for (int cus : {1, 64, 256, 304}) {
      const fleet::PlanOverrides ov = fleet::plan_overrides();
      printf("%s|%s|%s\n", fleet::kernel_name(fleet::plan_update(g, ov, cus)).c_str(),
             fleet::kernel_name(fleet::plan_update_encode(g, 3, ov, cus)).c_str(),
             fleet::kernel_name(fleet::plan_update_kardam(g, 3, ov, cus)).c_str());
    }
  return bad;
}
"""


@pytest.fixture(scope="session")
def check_launch(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc for the host build of kernels.hip")
    exe = str(tmp_path_factory.mktemp("launch_plan") / "check_launch")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", f"-I{CSRC}",
                           f"-I{os.path.join(ROOT, 'include')}", os.path.join(HERE, "native", "check_launch.hip"),
                           os.path.join(CSRC, "launch_plan.cpp"), "-rdynamic", "-o", exe])
    return exe


@pytest.fixture(scope="session")
def recorded(check_launch):
    return subprocess.run([check_launch], capture_output=True, text=True, timeout=300, check=True).stdout


def _golden():
    return open(os.path.join(HERE, "golden", "launch_plan.txt")).read()


def test_recorder_covers_the_sizes_and_specs_of_the_plan_tests(check_launch):
    out = subprocess.run([check_launch, "--sizes"], capture_output=True, text=True, check=True).stdout.splitlines()
    sizes = {int(x) for x in out[0].split()[1:]}
    assert set(T.GRID_SIZES) <= sizes
    for g in {row[0] for row in T.DEFAULT_PLAN} - {1_000, 349_526}:  # both sides of every boundary
        assert {g, g + 1} <= sizes or {g - 1, g} <= sizes, g
    assert out[1].split()[1:] == ["1", "23", "24", "25", "64", "256"] and out[2].split()[1:] == ["256", "304", "64"]
    specs = [ln[5:] for ln in out[3:]]
    grid_specs = next(m for m in T.test_launch_grid_covers_every_group.pytestmark if m.name == "parametrize").args[1]
    assert set(grid_specs) | {"fused=off", "grid=balanced", "tile_enc_rows=7", "tile_enc_prio=2",
                              "update=pipe,fused=off"} == set(specs)


def test_launches_equal_the_recording_of_the_old_launchers(recorded):
    new, old = recorded.splitlines(), _golden().splitlines()
    hashes = [ln for ln in old if ln.startswith("hash ")]
    assert len(hashes) == 18 * 3 * 4 and len(old) > len(hashes) + 300
    differ = [(a, b) for a, b in zip(old, new) if a != b]
    assert not differ and len(new) == len(old), differ[:5]


def test_reported_name_is_the_launched_kernel(recorded):
    """From the default block in full: what update_kernel_name / update_encode_kernel_name
    report for a size is the kernel on that size's launch line."""
    lines = [ln for ln in recorded.splitlines() if not ln.startswith("hash ")]
    first = {}  # (launcher, groups) -> the kernel of the call's first launch
    for ln in lines:
        m = re.match(r"(update|update_encode) groups=(\d+) M=64 g_begin=0 \| (\S.*?) grid=", ln)
        if m:
            first.setdefault((m.group(1), int(m.group(2))), m.group(3))
    names = [re.match(r"names groups=(\d+) .*? \| update=(.*) \| update_encode=(.*) \| kind=", ln) for ln in lines]
    names = [m for m in names if m]
    assert len(names) >= len(T.GRID_SIZES) and len(first) == 2 * len(names)
    for m in names:
        g = int(m.group(1))
        assert m.group(2) == first[("update", g)], g
        assert m.group(3).replace(" (with the encode's blocks)", "") == first[("update_encode", g)], g
    kinds = {k for k in first.values()}
    assert len(kinds) >= 8  # every form of both launchers is the default somewhere


def test_planner_is_plain_cxx_and_clean_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    main = tmp_path / "main.cpp"
    main.write_text(SAN_MAIN)
    exe = str(tmp_path / "plan_san")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", os.path.join(CSRC, "launch_plan.cpp"), str(main), "-o", exe, "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "k_update_mixed<256, false>|k_update_encode<256>|k_update_mixed<256, true>" in r.stdout
