#!/usr/bin/env python3
"""An allocation census of the host library: every handle kind created at its smallest
shape, used once, grown where it can grow, and destroyed, in one short process.

Run it under HIP API tracing with statistics, in a run of its own (no counters):

  rocprofv3 --hip-trace --stats -d OUT -- python scripts/alloc_census.py

and compare the call counts of hipMalloc, hipFree, hipHostMalloc, hipHostFree and
hipMemset between two builds of the library (`FLEET_CODEC_LIB` picks a build):
profiles/dev_mem/README.md keeps the tables. The script checks nothing but that every
call succeeds; it prints the steps it took. No fallback: without a GPU it fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def uploads(codec, layout, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        v = rng.normal(0, 0.05, layout.n_up).astype(np.float32)
        v[layout.header_positions()] = layout.header_values()
        out.append(codec.encode_floats(v))
    return out


def main():
    import torch
    import fleet_amd as F
    from fleet_amd.layouts import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the census counts device allocations only")
    small, large = synthetic(64), synthetic(4096)
    codec = F.Codec(0)
    step = lambda s: print("census:", s, flush=True)  # noqa: E731

    # the context's own buffers: host-buffer calls, then larger ones (the doubling grows)
    for lay, M in ((small, 2), (large, 5)):
        ups = uploads(codec, lay, M, M)
        d = [1.0 / (1 + c % 3) for c in range(M)]
        merged, _ = codec.update(ups, d, want_f32=True)
        codec.decode_floats(merged)
        codec.getNorm(codec.getFlatGradient(ups[0]))
        codec.addNative(ups[0], codec.scalarMulNative(ups[1], 0.5))
        # the device-resident parameters: a larger M retires the dampen buffer
        L = len(ups[0])
        groups = (F.b64_count(L) + 2) // 3
        rows = torch.zeros((M, 16 * groups + 16), dtype=torch.uint8, device="cuda")
        for c in range(M):
            rows[c, :L] = torch.from_numpy(np.frombuffer(ups[c], np.uint8).copy()).cuda()
        out_u8 = torch.zeros(16 * groups + 16, dtype=torch.uint8, device="cuda")
        out_f32 = torch.zeros(3 * groups + 4, dtype=torch.float32, device="cuda")
        codec.update_device(rows, L, d, lay.header_positions(), out_u8, out_f32)
        codec.check()
        step(f"context: {M} uploads of {L} bytes")
    codec.selftest_digest(0)
    w = np.linspace(-1, 1, 24, dtype=np.float32)
    codec.model_weights_text(w, [2, 3, 4])
    codec.values_text(w)
    step("context: temporaries of the model codec")

    # accumulator: pushes, then bursts that grow its staging
    ups = uploads(codec, small, 6, 7)
    L, hp = len(ups[0]), small.header_positions()
    acc = codec.accumulator(L, hp)
    acc.push(ups[0], 1.0)
    acc.finish()
    acc.push_many(ups[:3], [1.0, 0.5, 0.25])
    acc.push_finish(ups[:6], [1.0] * 6)
    acc.close()
    step("accumulator")

    # pool, gate, ledger, filter
    pool = codec.pool(L, hp, 4)
    for s in range(4):
        pool.put(s, ups[s])
    pool.update([2, 0, 3], [1.0, 0.5, 1.0])
    gate = pool.gate(small.header_values())
    gate.vet([0, 1, 2, 3])
    gate.close()
    ledger = pool.ledger(4)
    ledger.update([0, 1], [1.0, 1.0], [0, 1], [1, 1], 0.05)
    n = F.b64_count(L)
    filt = ledger.filter(n, 0, 0)
    filt.set_model(np.zeros(n, np.float32), np.zeros(0, np.float32))
    filt.update([2, 3], [1.0, 1.0], [2, 3], [2, 2], 0.05)
    filt.resolve([True, False])
    filt.close()
    ledger.close()
    pool.close()
    step("pool, gate, ledger, filter")

    # model ledger: two versions, an update of more pairs than the first one sized
    ml = codec.model_ledger(40, 0, 0, 3, 3)
    rng = np.random.default_rng(3)
    for vid in range(3):
        ml.stage(vid, rng.normal(0, 1, 40).astype(np.float32), np.zeros(0, np.float32))
    ml.update([0], [0])
    ml.update([1, 2, 1], [0, 1, 2])
    ml.close()
    step("model ledger")

    # the resident model: load, a step from a host text, both texts, a solver, destroy
    session = np.load(os.path.join(ROOT, "tests", "golden", "session_mnist.npz"))
    rm = F.ResidentModel(codec, bytes(session["init"]), distillation_mode=1, max_versions=3)
    rm.initUpdater(session["lrates"])
    rm.descentNative(bytes(session["merged0"]), int(session["batch"]), int(session["stale"]))
    rm.getParametersNative(0)
    rm.getModelParametersNative(0)
    allocs = rm.stats()["device_allocs"]
    rm.close()
    rm = F.ResidentModel(codec, bytes(session["init"]), distillation_mode=1, max_versions=3, solver="adam")
    rm.close()
    step(f"resident model ({allocs} allocations counted by its stats)")
    codec.close()
    step("done")


if __name__ == "__main__":
    main()
