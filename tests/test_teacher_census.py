"""Host census and mutants of the teacher forward (tests/native/check_teacher.cpp): the
kernel's loop nest over teacher_math.h, compiled for the host as test_native_math.py
compiles check_math (-ffp-contract=off -mfma).

* The plain build reproduces both teacher fixtures under the contract of
  tests/test_teacher.py, prints which data-dependent branches each fixture reaches, and
  fails unless tests/golden/teacher_edges.npz alone reaches every one of them.
* Each mutant build carries one deliberate error; teacher_edges.npz has to change a
  recorded bit or a NaN position under it.

Three of the mutants cannot be told from the original by any input, and the test pins
the reason instead: `mx < v` -> `mx <= v`, `mx2 < v` -> `mx2 <= v` (pooling scan) and
`v < 0` -> `v <= 0` (elu) only change which of two EQUAL values is taken, or turn +0
into 0.1f * (expf(+0) - 1) = +0. Values that compare equal have equal bits unless they
are +0 and -0, and -0 never arises inside the network: every sum starts from +0.0f,
x + (-x) and +0 + (-0) are +0 in round-to-nearest, so a pre-activation is never -0, and
elu of v < 0 is 0.1f * (expf(v) - 1): +0 where expf(v) rounds to 1, else at most
0.1f * -2^-24, never -0. The census counts -0 among pre-activations and pooled values
(0 in both fixtures, asserted), and the mutant runs show that the mutated comparison
decides differently (ties in pooling windows, +0 pre-activations) while not one picked
value or elu result changes.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import teacher_edges as TE  # noqa: E402

KILLABLE = [1, 2, 5, 6, 8, 9, 10, 11]
EQUIVALENT = [3, 4, 7]


def _clang():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def bench_dir(tmp_path_factory):
    if _clang() is None:
        pytest.skip("no clang++ for the host build of teacher_math.h")
    d = tmp_path_factory.mktemp("teacher_native")
    z = np.load(os.path.join(HERE, "golden", "teacher_mnist.npz"))
    TE.write_flat(str(d / "mnist.bin"), [(f"scale{i}", 1, z[f"w{i}"], z[f"b{i}"], z[f"x{i}"], z[f"probs{i}"])
                                         for i in range(3)])
    TE.write_flat(str(d / "edges.bin"), TE.load())
    return d


def _run(d, mutant, pool=0):
    exe = d / f"check_teacher_{mutant}_{pool}"
    subprocess.check_call([_clang(), "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", f"-DMUTANT={mutant}",
                           f"-DMUTANT_POOL={pool}", os.path.join(HERE, "native", "check_teacher.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(d / "mnist.bin"), str(d / "edges.bin")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    return r


def _counts(out, prefix):
    return {ln.split()[-2]: int(ln.split()[-1]) for ln in out.splitlines() if ln.startswith(prefix)}


def test_census_reproduces_fixtures_and_edges_reach_every_branch(bench_dir):
    r = _run(bench_dir, 0)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout and "MISSING" not in r.stdout and "MISMATCH" not in r.stdout
    # the rows the old fixture never visits (the reason for the new one)
    mnist = _counts(r.stdout, "census mnist  P1")
    assert mnist["denom_zero"] == 0 and mnist["all_equal"] == 0 and mnist["nan_slot0"] == 0
    for layer in ("P1", "P2"):
        edges = _counts(r.stdout, "census edges  " + layer)
        assert min(edges[k] for k in ("denom_zero", "denom_zero_other_bits", "all_equal", "largest_is_zero", "nan_slot0",
                                      "nan_other_slot", "cvtt_int_min", "cvtt_positive_overflow", "second_pick_other_bits",
                                      "t1_is_8", "t1_is_9", "t1_is_10")) > 0, layer
    assert "minus zero among pre-activations and pooled values: 0\n" in r.stdout


@pytest.mark.parametrize("mutant", KILLABLE)
def test_edge_fixture_kills_mutant(bench_dir, mutant):
    r = _run(bench_dir, mutant)
    assert r.returncode == 0 and f"mutant {mutant} KILLED" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("pool", [1, 2])
@pytest.mark.parametrize("mutant", [1, 2, 5, 6])
def test_edge_fixture_kills_pooling_mutant_in_one_layer(bench_dir, mutant, pool):
    """P1 (3x3) and P2 (2x2) are separate instantiations in the kernel: each alone has to be told."""
    r = _run(bench_dir, mutant, pool)
    assert r.returncode == 0 and f"mutant {mutant} KILLED" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("mutant", EQUIVALENT)
def test_equivalent_mutant_is_exercised_and_changes_no_value(bench_dir, mutant):
    """See the module docstring: no input can kill these. Pinned instead: the mutated
    comparison decides differently, and no value changes anywhere."""
    r = _run(bench_dir, mutant)
    assert f"mutant {mutant} SURVIVED" in r.stdout, r.stdout + r.stderr
    ln = next(x for x in r.stdout.splitlines() if x.startswith(f"mutant {mutant} ("))
    n = [int(t) for t in ln.split("): ")[1].replace("(", " ").replace(")", " ").replace(",", " ").split() if t.isdigit()]
    slot_differs, bits_differ, elu_differs, _elu_calls, at_plus_zero, at_minus_zero = n
    assert bits_differ == 0 and elu_differs == 0 and at_minus_zero == 0
    assert (at_plus_zero if mutant == 7 else slot_differs) > 0  # the mutated comparison did decide otherwise
