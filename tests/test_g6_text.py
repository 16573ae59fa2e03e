"""CPU check of g6_text (fleet_amd/csrc/decimal6.h), the `ostream << float` text the
device emits for model parameters: compiled for the host and compared with libc's
snprintf("%g") byte for byte on every 4099th bit pattern and on the edge list
(tests/native/check_g6text.cpp sample). `check_g6text exhaustive` covers all 2^32
inputs (run during development) and gives the digest of
tests/golden/g6text_digest.json, which the GPU self-test (fn 24) must reproduce."""
import json
import os
import shutil
import subprocess

import pytest

import g6_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clang():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def check_g6text(tmp_path_factory):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of decimal6.h")
    exe = tmp_path_factory.mktemp("native") / "check_g6text"
    subprocess.check_call([clang, "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-pthread",
                           os.path.join(ROOT, "tests", "native", "check_g6text.cpp"), "-o", str(exe)])
    return str(exe)


def test_g6_text_matches_libc_sampled(check_g6text):
    r = subprocess.run([check_g6text, "sample"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
    assert "longest 12 bytes" in r.stdout and "edge lengths 1..12" in r.stdout


def test_edge_list_is_the_checkers_and_python_agrees(check_g6text):
    """g6_edges.EDGE_BITS is the checker's list, and Python's '%g' spells every edge as libc does
    (the GPU test compares the device's text with g6_edges.g_text)."""
    r = subprocess.run([check_g6text, "edges"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [ln.split(" ") for ln in r.stdout.splitlines()]
    assert [int(b, 16) for b, _ in rows] == g6_edges.EDGE_BITS
    assert [t for _, t in rows] == [g6_edges.g_text(b) for b in g6_edges.EDGE_BITS]
    lens = {len(t) for _, t in rows}
    assert lens == set(range(1, 13))
    by_bits = dict((int(b, 16), t) for b, t in rows)
    assert by_bits[0x3727C5AC] == "1e-05" and by_bits[0x38D1B717] == "0.0001"      # 1e-5 | 1e-4
    assert by_bits[0x38D1B710] == "9.99999e-05"                                    # 9.999995e-5 stays below
    assert by_bits[0x497423F0] == "999999" and by_bits[0x49742400] == "1e+06"      # 999999 | 1e+06
    assert by_bits[0x497423F8] == "1e+06"                                          # 999999.5 carries
    assert by_bits[0x497423E8] == "999998" and by_bits[0x497423D8] == "999998"     # ties to even
    assert by_bits[0x00000001] == "1.4013e-45" and by_bits[0x7F7FFFFF] == "3.40282e+38"
    assert by_bits[0x80800000] == "-1.17549e-38"


def test_golden_digest_file():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "g6text_digest.json")))
    assert g["inputs"] == 1 << 32 and g["mismatches"] == 0 and g["longest"] == 12
    assert len(g["fn24"]) == 16 and int(g["fn24"], 16) > 0
