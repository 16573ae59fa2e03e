"""The streaming natives of the JNI shim (pushNative / finishNative / pendingNative /
discardNative on apps.cppNN.FleetUpdater) through the fake JVM's function table: M pushes
and a finish give aggregateNative's bytes and the oracle's, within the JNI rules."""
import ctypes as C
import os

import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST, synthetic

pytestmark = pytest.mark.gpu

JNI = os.path.join(os.path.dirname(F.LIB_PATH), "libfleet_native.so")
FU = "Java_apps_cppNN_FleetUpdater_"


@pytest.fixture(scope="module")
def shim():
    F.lib()  # same HIP runtime as torch
    L = C.CDLL(JNI)
    vp = C.c_void_p

    class Natives:
        pass

    sig = {"pushNative": ([vp, vp, vp, C.c_double], C.c_uint8), "finishNative": ([vp, vp], vp),
           "pendingNative": ([vp, vp], C.c_int32), "discardNative": ([vp, vp], None),
           "aggregateNative": ([vp, vp, vp, vp], vp)}
    for name, (args, res) in sig.items():
        f = getattr(L, FU + name)
        f.argtypes, f.restype = args, res
        setattr(Natives, name, staticmethod(f))
    return Natives


def check_rules(J):
    assert J.stat("overflows") == 0, "local references beyond the frame's capacity"
    assert J.stat("critical_violations") == 0, "JNI call inside a critical region"
    assert J.stat("critical_depth") == 0, "critical region left open"
    assert J.stat("pins") == 0, "array elements not released"


def uploads_for(oracle, layout, M, seed):
    return [oracle.encode_floats(oracle.synth_upload(seed, c, list(layout.w_sizes), list(layout.b_sizes)))
            for c in range(M)]


def test_push_finish_equals_aggregate_and_oracle(shim, oracle):
    import jnifake as J
    env = J.env()
    M = 6
    ups = uploads_for(oracle, MNIST, M, seed=12)
    d = [1.0 / ((c % 3) + 1) for c in range(M)]
    J.begin()
    assert shim.finishNative(env, None) is None  # nothing pushed: null
    assert shim.pendingNative(env, None) == 0
    for c in range(M):
        assert shim.pushNative(env, None, J.new_bytes(ups[c]), d[c]) == 1
        assert shim.pendingNative(env, None) == c + 1
    assert J.stat("criticals") == M  # each array read in place, in one critical region
    merged = J.read_bytes(shim.finishNative(env, None))
    assert shim.pendingNative(env, None) == 0
    check_rules(J)
    J.begin()
    objs = J.new_object_array([J.new_bytes(u) for u in ups])
    batch = J.read_bytes(shim.aggregateNative(env, None, objs, J.new_doubles(d)))
    check_rules(J)
    assert merged == batch == oracle.update_faithful(ups, d)


def test_malformed_push_discard_and_relayout(shim, oracle):
    import jnifake as J
    env = J.env()
    ups = uploads_for(oracle, MNIST, 3, seed=13)
    d = [1.0, 0.5, 1 / 3]
    J.begin()
    assert shim.pushNative(env, None, J.new_bytes(ups[0]), d[0]) == 1
    bad = ups[1][:500] + b"*" + ups[1][501:]
    assert shim.pushNative(env, None, J.new_bytes(bad), d[1]) == 0       # malformed text
    assert shim.pushNative(env, None, J.new_bytes(ups[1][:-16]), d[1]) == 0  # another length mid-batch
    assert shim.pushNative(env, None, None, d[1]) == 0
    assert shim.pendingNative(env, None) == 1  # the batch is intact
    assert shim.pushNative(env, None, J.new_bytes(ups[1]), d[1]) == 1
    assert J.read_bytes(shim.finishNative(env, None)) == oracle.update_faithful(ups[:2], d[:2])
    check_rules(J)
    # discardNative empties the accumulator
    J.begin()
    assert shim.pushNative(env, None, J.new_bytes(ups[2]), d[2]) == 1
    assert shim.pendingNative(env, None) == 1
    shim.discardNative(env, None)
    assert shim.pendingNative(env, None) == 0
    assert shim.finishNative(env, None) is None
    # an upload of another length while empty: the accumulator is re-created from its layout
    lay = synthetic(1001)
    small = uploads_for(oracle, lay, 2, seed=14)
    for u in small:
        assert shim.pushNative(env, None, J.new_bytes(u), 0.5) == 1
    assert J.read_bytes(shim.finishNative(env, None)) == oracle.update_faithful(small, [0.5, 0.5])
    check_rules(J)
