"""CPU check of the one-fma-per-step /10 chains of codec_math.h (the scaled
div10_mt with its MulEntry / StepTables rows, the fixed nine-step d9) against the
reference's chain of binary32 divisions by 10: every digit row d = 0..15, the
binades 2^-3 .. 2^31, both signs, +-0, and (float)c of int32 codes with the row of
their own last digit, sampled (~1.3e9 comparisons, a few seconds).
`tests/native/check_div10 exhaustive` covers every mantissa and every int32 code
(run during development; the result is in DESIGN.md §2)."""
import os
import subprocess

import pytest

from test_native_math import _clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_div10(tmp_path_factory):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of codec_math.h")
    exe = tmp_path_factory.mktemp("native") / "check_div10"
    subprocess.check_call([clang, "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-pthread",
                           os.path.join(ROOT, "tests", "native", "check_div10.cpp"), "-o", str(exe), "-lm"])
    return str(exe)


def test_scaled_chains_match_division_chain_sampled(check_div10):
    r = subprocess.run([check_div10, "sample"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
