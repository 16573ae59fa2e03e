"""The one-fma-per-step /10 chains (codec_math.h div10_mt, d9) inside the aggregation
kernels, on inputs built to walk every row of their step tables: the stream plan
(k_update_mixed<256>) and the flat tiles (k_update_flat) against the oracle's fused
update, byte for byte.

Shape: 3 clients (the first client, one two-client trip and the odd tail of the
stream kernel's client loop) of 3 * (256 + 21) + 2 = 833 values (one full block of
group-per-lane waves, a value-per-lane wave, and a ragged last group). The payload
repeats a 61-value pattern (61 is prime to 3 and to the 64 lanes of a wave, so every
region of the grid meets all of it), shifted by 20 per client so the running sums mix
magnitudes. The pattern holds, with both signs: every power of ten of the codec's
domain and the binary32 value just below it (numDigits 0..9 on either side of each
step of the digit count, so every last digit 0..9 of a code in int2float), 0, values
that encode to code 0 (|x| < 1e-8, with and without a sign: the -0.0 start of a chain),
a value whose dampened form does, and mid-mantissa values of every magnitude."""
import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import synthetic

pytestmark = pytest.mark.gpu

M = 3
N_UP = 3 * (256 + 21) + 2
DAMPEN = [1.0, 0.1, 0.25]  # 0.1 is no binary32 value: scalarMultiply's f64 branch
PERIOD, SHIFT = 61, 20


def _below(x):
    return np.nextafter(np.float32(x), np.float32(0))


def _pattern():
    p = [np.float32(10.0 ** m) for m in range(0, 9)]          # numDigits 1..9
    p += [_below(10.0 ** m) for m in range(0, 10)]            # numDigits 0..9
    p += [np.float32(-(10.0 ** m)) for m in range(0, 8)]      # '-' counts: numDigits 2..9
    p += [-_below(10.0 ** m) for m in range(0, 9)]            # numDigits 0 (int 0), 2..9
    p += [0.0, 5e-8, -5e-8, 3e-10, -3e-10]                    # code 0; -5e-8 * 0.1 gives the signed code 0
    for v in (3.7e-7, 3.7e-4, 0.037, 37.5, 3.7e3, 3.7e5, 3.7e7):
        p += [v, -v]
    p += [3.7e8, 0.5, -0.5, 123456.789, -123456.789, 2.5]
    p = np.asarray(p, np.float32)
    assert len(p) == PERIOD
    return p


def _num_digits(x):
    """Base64::numDigits((int)x), '-' counted, for |x| < 2^31."""
    t = np.trunc(x.astype(np.float64))
    a = np.abs(t)
    return np.where(a >= 1, np.floor(np.log10(np.maximum(a, 1))) + 1, 0).astype(np.int64) + (t < 0)


@pytest.fixture(scope="module")
def case(oracle):
    lay = synthetic(N_UP)
    pat = _pattern()
    i = np.arange(N_UP - 3)
    vals, ups = [], []
    for c in range(M):
        v = oracle.synth_upload(11, c, list(lay.w_sizes), list(lay.b_sizes))
        v[2:N_UP - 1] = pat[(i + SHIFT * c) % PERIOD]  # the layout's header ([1, N], trailing 0) stays
        vals.append(v)
        ups.append(oracle.encode_floats(v))
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))
    merged, f32 = oracle.update_fused(ups, DAMPEN, hm, want_f32=True)
    return lay, vals, ups, merged, f32


def test_inputs_walk_every_row(oracle, case):
    """Stage A (Q of the decoded value), B (Q of the dampened value) and C (Q of the running
    sum) together meet every numDigits 0..9 of either sign; the uploads' codes end in
    every digit 0..9 and include code 0."""
    _, vals, ups, _, _ = case
    q = lambda x: oracle.int2float(oracle.float2int(np.ascontiguousarray(x, np.float32)))
    seen, last = set(), set()
    acc = None
    for c in range(M):
        codes = oracle.decode_ints(ups[c])[2:N_UP - 1]
        last |= set(np.abs(codes.astype(np.int64)) % 10)
        assert (codes == 0).any()
        a_in = oracle.int2float(codes)
        b_in = (q(a_in).astype(np.float64) * DAMPEN[c]).astype(np.float32)
        b = q(b_in)
        stage_inputs = [a_in, b_in]
        if acc is None:
            acc = b
        else:
            stage_inputs.append(acc + b)
            acc = q(acc + b)
        for x in stage_inputs:
            x = x[np.abs(x) < 2.0 ** 31]
            seen |= set(zip(_num_digits(x).tolist(), np.signbit(x).tolist()))
    assert last == set(range(10))
    # no negative value has numDigits 1: (int)x is 0 above -1 and "-1" .. "-9" count two
    assert seen >= {(d, s) for d in range(10) for s in (False, True)} - {(1, True)}


@pytest.mark.parametrize("spec,kernel", [("update=stream", "k_update_mixed<256"), ("update=tiled,tile=flat", "k_update_flat")])
def test_update_matches_oracle_on_every_row(codec, plan, case, spec, kernel):
    lay, _, ups, merged, f32 = case
    plan(spec)
    assert F.update_kernel(F.b64_len(lay.n_up)).startswith(kernel)
    got, got_f32 = codec.update(ups, DAMPEN, want_f32=True)
    assert got == merged
    assert np.array_equal(got_f32.view(np.uint32), f32.view(np.uint32))
