"""The --mirror mode of tests/native/check_client_dp.cpp, without a GPU: fed the fixture's seven
cases it reproduces the recorded digests and the recorded sqsum, norm and scale
(tests/golden/client_dp_ref.npz: the reference's own bits); for a client with sigma = 0 under
cross-entropy it gives the vector check_client_grad --mirror gives; and built with
AddressSanitizer and UndefinedBehaviorSanitizer it runs, stand-alone, the whole job list the
device tests compare with (tests/client_dp_jobs.py) and writes the bytes the plain build writes."""
import os
import subprocess

import numpy as np
import pytest

import client_dp_jobs as J
import client_dp_ref as R
from test_native_math import _clang

f = np.float32


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("client_dp_mirror")


@pytest.fixture(scope="module")
def exe(workdir):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of client_backward.h")
    path = workdir / "check_client_dp"
    subprocess.check_call(J.compile_command(clang, path))
    return path


def _fixture_jobs():
    w, b = R.model()
    jobs = []
    for name, B, cost, clip, sigma, x, lab, sh in R.cases():
        jobs.append(J.Job(name, [(w, b)], x, lab, np.arange(B, dtype=np.int32).reshape(1, B), sh.reshape(1, B, 2),
                          np.zeros(1, np.int32), np.array([sigma], f), clip=np.array([clip], f), cost=cost,
                          temperature=R.TEMPERATURE))
    return jobs


def test_fixture_cases_as_mirror_jobs(exe, workdir):
    z = R.load()
    jobs = _fixture_jobs()
    assert [j.name for j in jobs] == ["a", "b", "c", "d", "e1", "e3", "f"]
    for j, r in zip(jobs, J.run_mirror(exe, workdir, "fixture", jobs)):
        assert R.sha(r.vec[0]) == R.sha_of(z, f"{j.name}_grad_sha256"), j.name
        assert r.blown[0] == 0
        if j.sigma[0] > 0:
            for k, field in enumerate(("sqsum", "norm", "scale")):
                assert np.array_equal(R.bits(r.stats[0, k, 1:]), R.bits(z[f"{j.name}_{field}"][1:])), (j.name, field)
            assert tuple(r.stats[0, :, 0]) == (0.0, 0.0, 1.0)
        else:
            assert not r.stats.any(), j.name


def test_sigma_zero_is_the_plain_mirror(exe, workdir):
    """client 0 (sigma = 0) of a cross-entropy job equals check_client_grad --mirror's vector in
    bits; client 1 (the same samples, sigma > 0 and a clip below its norms) does not"""
    inp = J.inputs()
    w, b = inp["models"][1]
    idx, sh = J._draw(1, 3, len(inp["x"]), 77)
    idx, sh = np.repeat(idx, 2, 0), np.repeat(sh, 2, 0)
    job = J.Job("pair", [(w, b)], inp["x"], inp["lab"], idx, sh, np.zeros(2, np.int32), np.array([0.0, J.SIGMA_TINY], f),
                clip=np.array([1.0, 1.0], f))
    got = J.run_mirror(exe, workdir, "pair", [job])[0]
    plain = workdir / "check_client_grad"
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-mfma", "-ffp-contract=off",
                           os.path.join(J.ROOT, "tests", "native", "check_client_grad.cpp"), "-o", str(plain)])
    pick = idx.reshape(-1)
    with open(workdir / "plain.jobs", "wb") as fh:
        fh.write(np.int32(1).tobytes() + w.tobytes() + b.tobytes() + np.array([2, 3], np.int32).tobytes() + f(2.0).tobytes())
        fh.write(np.ascontiguousarray(inp["x"][pick]).tobytes() + inp["lab"][pick].tobytes() + sh.tobytes())
    subprocess.check_call([str(plain), "--mirror", str(workdir / "plain.jobs"), str(workdir / "plain.out")], timeout=600)
    want = np.fromfile(workdir / "plain.out", f).reshape(2, J.N_UP)
    assert np.array_equal(J.bits(want[0]), J.bits(want[1]))
    assert np.array_equal(J.bits(got.vec[0]), J.bits(want[0]))
    assert not got.stats[0].any()
    assert (got.stats[1, 2, 1:] < 1).all() and got.stats[1, 2, 0] == 1
    differ = J.bits(got.vec[1]) != J.bits(want[1])
    felt = np.abs(want[1, :J.BIAS_START]) > 2.0 ** -20  # a noise of 2^-60 z changes only sums near zero
    assert differ[J.BIAS_START:].any() and felt.any() and not differ[:J.BIAS_START][felt].any()  # only dbias blocks are scaled


def test_job_list_under_sanitizers(exe, workdir):
    """the list's two passes through the sanitized build, stand-alone: clean, and byte for byte
    the plain build's output; the list's own conditions hold"""
    san = workdir / "check_client_dp_san"
    r = subprocess.run(J.compile_command(_clang(), san, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitizer" in r.stderr.lower()):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-4000:]
    inp = J.inputs()
    ex = J.expectations(lambda tag, jobs: J.run_mirror(san, workdir, "san_" + tag, jobs), inp)
    J.check_conditions(ex)
    samples = sum(j.C * j.B for j in J.with_twins([e.job for e in ex.values()]))
    assert samples <= 500, samples
    J.expectations(lambda tag, jobs: J.run_mirror(exe, workdir, "plain_" + tag, jobs), inp)
    for tag in ("pass1", "pass2"):
        assert open(workdir / f"san_{tag}.jobs", "rb").read() == open(workdir / f"plain_{tag}.jobs", "rb").read()
        assert open(workdir / f"san_{tag}.out", "rb").read() == open(workdir / f"plain_{tag}.out", "rb").read(), tag
