"""Jobs for the host mirror of DPgradients and the distillation cost
(tests/native/check_client_dp.cpp --mirror over fleet_amd/csrc/client_backward.h): the job
writer, the reader of its output and the job list tests/test_gpu_client_dp_shapes.py runs on the
device and tests/test_client_dp_mirror_cpu.py runs under the host sanitizers. Nothing here is
recorded: the mirror computes every expectation at test time.

The clips come from two mirror passes (expectations()):
  pass 1  every client with one more slot in front (slot 0 is never clipped, so it has no norm
          of its own), clip 1, sigma 2^-60: the norm of every sample of every job
  pass 2  the jobs with their clips settled from those norms (settle()), each followed by its
          plain twin (sigma = 0 everywhere) where it has a DP client: the expected rows
settle() per kind of job:
  median  a DP client's clip is the median of its norms over slots 1 .. B-1 (B - 1 is even for
          every B here, so the median lies between two norms: one slot is clipped, one is not);
          with B = 2 the DP clients take half and twice their one norm in turn; with B = 1
          nothing is clipped and the clip only scales the noise. The first DP client of a job
          gets its sample of the largest norm in slot 0, so that slot 0's norm exceeds the clip
          and a clipped slot 0 would show.
  edges   clip_scale's edges, one client each (test (e))
  blown   client 1 sits on a model whose forward is NaN; its clip is 1
"""
import dataclasses
import os
import re
import subprocess

import numpy as np

import client_grad_ref as G
import eval_ref as E

f = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "check_client_dp.cpp")
N_UP = G.N_UP
N_ROW = E.N_W + E.N_B
SIGMA_TINY = f(2.0 ** -60)  # DP for the host and the device; its noise changes only sums near zero
SUBNORMAL = np.nextafter(f(0), f(1))  # the smallest positive float
CYCLE = (f(0.0), SIGMA_TINY, f(1.0 / 128), f(4.0))
BIAS_START = 21455  # the dbias blocks of gradients() start behind this header


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@dataclasses.dataclass
class Job:
    """C clients of B samples: client c runs on models[model_of[c]] with clip[c] and sigma[c]
    over the samples idx[c] of the pool x, lab, shifted by shifts[c]"""
    name: str
    models: list  # [(w, b)]
    x: np.ndarray
    lab: np.ndarray
    idx: np.ndarray  # [C, B] int32
    shifts: np.ndarray  # [C, B, 2] int32
    model_of: np.ndarray  # [C] int32
    sigma: np.ndarray  # [C] float32
    clip: np.ndarray = None  # [C] float32, settled from pass 1 where None
    cost: int = 0
    temperature: float = 2.0
    kind: str = "median"

    @property
    def C(self):
        return self.idx.shape[0]

    @property
    def B(self):
        return self.idx.shape[1]

    @property
    def dp(self):
        return self.sigma > 0

    def model_rows(self):
        return np.stack([np.concatenate([w, b]) for w, b in self.models])

    def but(self, **kw):
        return dataclasses.replace(self, **kw)


@dataclasses.dataclass
class Result:
    vec: np.ndarray  # [C, 22961]
    stats: np.ndarray  # [C, 3, B]: sqsum, norm, scale
    blown: np.ndarray  # [C]: samples whose E is NaN


def write_jobs(path, jobs):
    with open(path, "wb") as fh:
        fh.write(np.int32(len(jobs)).tobytes())
        for j in jobs:
            rows = j.model_rows()
            assert rows.shape[1] == N_ROW and j.shifts.shape == (j.C, j.B, 2) and len(j.clip) == len(j.sigma) == j.C
            fh.write(np.int32(len(rows)).tobytes() + np.ascontiguousarray(rows, f).tobytes())
            fh.write(np.array([j.C, j.B], np.int32).tobytes() + f(j.temperature).tobytes() + np.int32(j.cost).tobytes())
            for a, t in ((j.model_of, np.int32), (j.clip, f), (j.sigma, f)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
            pick = j.idx.reshape(-1)
            fh.write(np.ascontiguousarray(j.x[pick], f).tobytes() + np.ascontiguousarray(j.lab[pick], np.int32).tobytes())
            fh.write(np.ascontiguousarray(j.shifts, np.int32).tobytes())


def read_results(path, stdout, jobs):
    raw = np.fromfile(path, f)
    blown = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"^job (\d+) client (\d+) blown (\d+)$", stdout, re.M)}
    out, o = [], 0
    for i, j in enumerate(jobs):
        nv, ns = j.C * N_UP, j.C * 3 * j.B
        out.append(Result(raw[o:o + nv].reshape(j.C, N_UP), raw[o + nv:o + nv + ns].reshape(j.C, 3, j.B),
                          np.array([blown[(i, c)] for c in range(j.C)])))
        o += nv + ns
    assert o == len(raw), "the mirror wrote another number of values than the jobs ask for"
    return out


def compile_command(clang, exe, flags=()):
    return [clang, "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", *flags, SOURCE, "-o", str(exe)]


def run_mirror(exe, directory, tag, jobs):
    """the mirror over these jobs: [Result], one per job"""
    jobs_path, out_path = os.path.join(str(directory), f"{tag}.jobs"), os.path.join(str(directory), f"{tag}.out")
    write_jobs(jobs_path, jobs)
    r = subprocess.run([str(exe), "--mirror", jobs_path, out_path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"mirror {tag}: exit {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return read_results(out_path, r.stdout, jobs)


# ------------------------------------------------------------------ the inputs and the job list

def inputs():
    """what tests/test_gpu_client_grad.py runs on: two models, 40 images, seeded labels"""
    lab = np.random.RandomState(5).randint(0, 10, 40).astype(np.int32)
    return dict(models=[G.model(), E.model_a(seed=9)], x=E.images_a(40, seed=777), lab=lab)


def overflowing_model(factor=1e22):
    """the first model with C1's 200 weights times `factor` and FC2's 1920 divided by it: the
    forward stays finite while a sample's squares overflow binary32"""
    w, b = G.model()
    w = w.copy()
    w[E.W_SPLITS[0]:E.W_SPLITS[1]] = (w[E.W_SPLITS[0]:E.W_SPLITS[1]] * f(factor)).astype(f)
    w[E.W_SPLITS[3]:E.W_SPLITS[4]] = (w[E.W_SPLITS[3]:E.W_SPLITS[4]] / f(factor)).astype(f)
    return w, b


def nan_model():
    """an inf pair in FC2: the forward comes out NaN (test_gpu_client_grad.py's blown model)"""
    w, b = G.model()
    w = w.copy()
    w[E.W_SPLITS[3]] = np.inf
    w[E.W_SPLITS[3] + 1] = np.inf
    return w, b


def _draw(C, B, n_images, seed, distinct=False):
    r = np.random.RandomState(seed)
    if distinct:
        idx = r.permutation(n_images)[:C * B].reshape(C, B).astype(np.int32)
    else:
        idx = r.randint(0, n_images, (C, B)).astype(np.int32)  # with repeats
    return idx, r.randint(-1, 2, (C, B, 2)).astype(np.int32)


def _cycle(C, start):
    return np.array([CYCLE[(start + c) % 4] for c in range(C)], f)


SWEEP = [(3, 1), (3, 2), (4, 3), (5, 7), (2, 33)]


def drafts(inp=None):
    """the job list before its clips are settled"""
    inp = inp or inputs()
    models, x, lab = inp["models"], inp["x"], inp["lab"]

    def job(name, C, B, seed, sigma, model_of=None, **kw):
        idx, sh = _draw(C, B, len(x), seed, distinct=kw.pop("distinct", False))
        of = np.array([(c + seed) % 2 for c in range(C)], np.int32) if model_of is None else np.array(model_of, np.int32)
        return Job(name, kw.pop("models", models), x, lab, idx, sh, of, np.asarray(sigma, f), **kw)
    out = []
    # (a) the shape sweep: the sigma mix starts elsewhere in the cycle from job to job, always with a plain client
    for n, ((C, B), start) in enumerate(zip(SWEEP, (0, 2, 1, 3, 3))):
        out.append(job(f"{C}x{B}", C, B, 500 + n, _cycle(C, start)))
    # (b) distillation: with the mix and without DP, temperature 2; the mix once at temperature 1
    for n, (C, B) in enumerate(((3, 2), (4, 3))):
        out.append(job(f"distill_{C}x{B}", C, B, 520 + n, _cycle(C, n + 2), cost=1))
        out.append(job(f"distill_{C}x{B}_plain", C, B, 520 + n, np.zeros(C, f), cost=1))
    out.append(job("distill_3x2_t1", 3, 2, 525, _cycle(3, 3), cost=1, temperature=1.0))
    # (c) the chunk walk: at chunk 2 a DP chunk, a plain chunk, a DP tail of one client
    out.append(job("walk", 5, 3, 530, [4.0, SIGMA_TINY, 0.0, 0.0, 1.0 / 128]))
    # (d) the second call of the reuse sequence: other shapes, clips and sigmas than 5x7's
    out.append(job("reuse_3x2", 3, 2, 540, [4.0, 1.0 / 128, SIGMA_TINY]))
    # (e) clip_scale's edges
    sigma = np.full(6, SIGMA_TINY, f)
    sigma[4] = SUBNORMAL
    out.append(job("edges", 6, 3, 550, sigma, model_of=[0, 1, 0, 1, 0, 2], models=models + [overflowing_model()],
                   kind="edges", distinct=True))
    # (i) a NaN forward beside two sound clients, DP for all
    out.append(job("blown", 3, 2, 560, [SIGMA_TINY, 1.0 / 128, 4.0], model_of=[0, 2, 1], models=models + [nan_model()],
                   kind="blown"))
    return out


def pass1(jobs):
    """every client with its slot 0 doubled in front, clip 1, sigma 2^-60: slots 1 .. B of the
    result hold the norms of the job's slots 0 .. B-1"""
    return [j.but(idx=np.concatenate([j.idx[:, :1], j.idx], 1), shifts=np.concatenate([j.shifts[:, :1], j.shifts], 1),
                  clip=np.ones(j.C, f), sigma=np.full(j.C, SIGMA_TINY, f)) for j in jobs]


def _swap(j, norms, c, a, b):
    for arr in (j.idx[c], j.shifts[c], norms[c]):
        arr[[a, b]] = arr[[b, a]]


def settle(job, norms):
    """the job with its clips chosen from norms [C, B] (a copy; norms is permuted along with the
    slots where the job's samples are)"""
    j = job.but(idx=job.idx.copy(), shifts=job.shifts.copy(), clip=np.ones(job.C, f))
    C, B, dp = j.C, j.B, j.dp
    if j.kind == "blown":
        sound = [c for c in range(C) if c != 1]
        for c in sound:
            j.clip[c] = f(0.5) * norms[c, 1]
        return j
    if j.kind == "edges":
        for c in range(C):  # slot 1 takes the smaller of the two norms: slot 2 is clipped at every edge of slot 1
            if norms[c, 1] > norms[c, 2]:
                _swap(j, norms, c, 1, 2)
        n1 = norms[:, 1]
        j.clip[0] = n1[0]
        j.clip[1] = np.nextafter(n1[1], f(0))
        j.clip[2] = np.nextafter(n1[2], f(np.inf))
        j.clip[3] = SUBNORMAL
        j.clip[4] = f(0.5) * n1[4]
        j.clip[5] = f(1.0)
        return j
    first = True
    below = True
    for c in np.flatnonzero(dp):
        if B >= 2 and first:
            _swap(j, norms, c, 0, int(np.argmax(norms[c])))
            first = False
        if B >= 3:
            j.clip[c] = f(np.median(norms[c, 1:].astype(np.float64)))
        elif B == 2:
            j.clip[c] = (f(0.5) if below else f(2.0)) * norms[c, 1]
            below = not below
        else:
            j.clip[c] = f(2.0 ** 40)  # nothing to clip; a noise of 2^-20 z shows in the row
    return j


def plain_of(j):
    return j.but(name=j.name + "/plain", sigma=np.zeros(j.C, f))


@dataclasses.dataclass
class Expectation:
    job: Job
    want: Result
    plain: np.ndarray  # the rows of the job's plain twin, or None where no client is DP
    norms: np.ndarray  # [C, B] from pass 1, slot 0 included


def settled_jobs(run, inp=None):
    """([Job] with clips, {name: norms}) after pass 1; run(tag, jobs) -> [Result]"""
    d = drafts(inp)
    out, norms = [], {}
    for j, r in zip(d, run("pass1", pass1(d))):
        n = r.stats[:, 1, 1:].copy()
        out.append(settle(j, n))
        norms[j.name] = n
    return out, norms


def with_twins(jobs):
    return [k for j in jobs for k in ([j, plain_of(j)] if j.dp.any() else [j])]


def expectations(run, inp=None):
    """{name: Expectation} of the whole list, in two mirror passes"""
    jobs, norms = settled_jobs(run, inp)
    everything = with_twins(jobs)
    res = dict(zip((j.name for j in everything), run("pass2", everything)))
    return {j.name: Expectation(j, res[j.name], res[j.name + "/plain"].vec if j.dp.any() else None, norms[j.name])
            for j in jobs}


def check_conditions(ex):
    """what must hold of the mirror's output before anything is compared with it, so that no job
    passes vacuously; the edges and the blown model have conditions of their own in their tests"""
    for name, e in ex.items():
        j, want = e.job, e.want
        dp = j.dp
        if j.kind != "blown":
            assert not np.isnan(want.vec).any() and not want.blown.any(), name
        if j.kind != "median":
            continue
        scale = want.stats[:, 2, 1:]
        for c in np.flatnonzero(dp):
            if j.B >= 3:
                assert (scale[c] < 1).any() and (scale[c] == 1).any(), (name, c, scale[c])
        clipped = [c for c in np.flatnonzero(dp) if j.B >= 2 and (scale[c] < 1).any()]
        if clipped:
            assert any(e.norms[c, 0] > j.clip[c] for c in clipped), (name, "slot 0 lies under every clip")
        if j.B == 2 and dp.sum() >= 2:
            assert (scale[dp] < 1).any() and (scale[dp] == 1).any(), (name, "B = 2: a clip below and one above")
        for c in range(j.C):
            differs = (bits(want.vec[c, BIAS_START:]) != bits(e.plain[c, BIAS_START:])).any() if dp.any() else False
            if dp[c]:
                assert differs, (name, c, "the DP row equals the plain row in every bias block")
            elif dp.any():
                assert not (bits(want.vec[c]) != bits(e.plain[c])).any(), (name, c)
