"""bench.py --dump-outputs and the plain / --full split.

CPU: the dump writer (float32 files, an array over its cap as the same seeded sample
every time) and the command line. GPU: a plain measurement of mnist64 times only the
form it reports, with exactly the steps asked for, and the pipelined and sequential
forms dump the same merged text, merged_f32 and encoded uploads, which are the
codec's own results for those uploads.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dumper_writes_float32_and_a_fixed_sample(tmp_path, monkeypatch):
    import torch
    bench = _bench()
    monkeypatch.setitem(bench.DUMP_CAP, "encoded_text", 1000)
    text = torch.arange(250 * 40, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(250, 40)
    f32 = torch.tensor([0.0, -0.0, 1.5, float("inf"), float("nan"), 1e-40], dtype=torch.float32)
    merged = torch.arange(64, dtype=torch.uint8)
    for d in ("a", "b"):
        bench.dumper(torch, str(tmp_path / d))({"merged_text": merged, "merged_f32": f32, "encoded_text": text})
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("merged_text", "merged_f32", "encoded_text")}
    assert all(v.dtype == np.float32 and v.ndim == 1 for v in a.values())
    assert np.array_equal(a["merged_text"], np.arange(64, dtype=np.float32))
    assert np.array_equal(a["merged_f32"].view(np.uint32), f32.numpy().view(np.uint32))  # bit for bit
    # over the cap: `cap` elements at seeded flat indices in index order, the same in every run
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, text.numel(), 1000))
    assert np.array_equal(a["encoded_text"], text.reshape(-1).numpy()[idx].astype(np.float32))
    assert np.array_equal(a["encoded_text"], np.load(tmp_path / "b" / "encoded_text.npy"))
    assert 4 * sum(bench.DUMP_CAP.values()) <= 64 * 10**6 - 3 * 128  # the files' bytes with their headers


def test_command_line_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         check=True).stdout
    assert "--full" in out and "--dump-outputs DIR" in out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_one_form_and_dumps_the_codecs_results(codec, tmp_path, monkeypatch):
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, "SETTLE_S", 0.0)
    steps = 5  # odd: the pipelined step's one-step graph, the last batch in buffer 1
    got = {}
    for form, sequential in (("pipelined", False), ("sequential", True)):
        res = bench.time_workload(torch, None, codec, "mnist64", steps, 1, 0, 1, True, full=False,
                                  sequential=sequential, dump=bench.dumper(torch, str(tmp_path / form)))
        got[form] = {n: np.load(tmp_path / form / f"{n}.npy") for n in ("merged_text", "merged_f32", "encoded_text")}
        assert res["steps"] == steps
        # only the reported form was timed
        assert res["eager_ms_per_step"] is None and res["update_kernel_ms"] is None and res["encode_kernel_ms"] is None
        if sequential:
            assert res["pipelined"] is None and res["ms_per_step"] > 0 and res["gib_s"] > 0
        else:
            assert res["ms_per_step"] is None and res["gib_s"] is None
            assert res["pipelined"]["ms_per_step"] > 0 and res["pipelined"]["kernel_ms"] is None
    for n, a in got["pipelined"].items():
        assert a.dtype == np.float32
        assert np.array_equal(a.view(np.uint32), got["sequential"][n].view(np.uint32)), n
    # the dumped arrays are the codec's own results for the workload's uploads
    from fleet_amd.layouts import LAYOUTS
    sh = bench.Shard(codec, torch, LAYOUTS["mnist"], 64, 0, 1)
    sh.encode()
    sh.aggregate()
    torch.cuda.synchronize()
    codec.check()
    p = got["pipelined"]
    assert np.array_equal(p["merged_text"], sh.merged[:sh.L].cpu().numpy().astype(np.float32))
    assert np.array_equal(p["merged_f32"].view(np.uint32),
                          sh.merged_f32[:sh.n_local].cpu().numpy().view(np.uint32))
    assert np.array_equal(p["merged_f32"].view(np.uint32),
                          codec.decode_floats(p["merged_text"].astype(np.uint8).tobytes()).view(np.uint32))
    cap = bench.DUMP_CAP["encoded_text"]
    assert sh.text.numel() > cap  # over the cap: the seeded sample of the 64 uploads
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, sh.text.numel(), cap))
    assert np.array_equal(p["encoded_text"], sh.text.reshape(-1).cpu().numpy()[idx].astype(np.float32))
