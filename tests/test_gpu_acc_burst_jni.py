"""pushBatchNative of the JNI shim (apps.cppNN.FleetUpdater) through the fake JVM's function
table: a burst, single pushes and a finish give the oracle's bytes within the JNI rules,
and a burst that cannot be taken whole changes nothing."""
import ctypes as C
import os

import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST

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

    sig = {"pushNative": ([vp, vp, vp, C.c_double], C.c_uint8), "pushBatchNative": ([vp, vp, vp, vp], C.c_uint8),
           "finishNative": ([vp, vp], vp), "pendingNative": ([vp, vp], C.c_int32), "discardNative": ([vp, vp], None)}
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


@pytest.fixture(scope="module")
def ups(oracle):
    return [oracle.encode_floats(oracle.synth_upload(15, c, list(MNIST.w_sizes), list(MNIST.b_sizes)))
            for c in range(6)]


@pytest.mark.parametrize("frame_limit", [1 << 30, 3], ids=["in-place", "copied"])
def test_burst_push_finish_equals_oracle(shim, oracle, ups, frame_limit):
    """With the references granted the arrays are read in place inside one critical region;
    a JVM that refuses them gets each array copied in turn."""
    import jnifake as J
    env = J.env()
    d = [1.0 / ((c % 3) + 1) for c in range(6)]
    shim.discardNative(env, None)
    J.fakejvm().fakejvm_set_frame_limit(frame_limit)
    try:
        J.begin()
        objs = J.new_object_array([J.new_bytes(u) for u in ups[:4]])
        assert shim.pushBatchNative(env, None, objs, J.new_doubles(d[:4])) == 1
        assert (J.stat("criticals") == 4) == (frame_limit > 4)
        check_rules(J)
    finally:
        J.fakejvm().fakejvm_set_frame_limit(1 << 30)
    assert shim.pendingNative(env, None) == 4
    J.begin()
    assert shim.pushNative(env, None, J.new_bytes(ups[4]), d[4]) == 1
    objs = J.new_object_array([J.new_bytes(ups[5])])
    assert shim.pushBatchNative(env, None, objs, J.new_doubles(d[5:])) == 1  # a burst of one
    assert shim.pendingNative(env, None) == 6
    merged = J.read_bytes(shim.finishNative(env, None))
    assert shim.pendingNative(env, None) == 0
    check_rules(J)
    assert merged == oracle.update_faithful(ups, d)


def test_burst_that_cannot_be_taken_changes_nothing(shim, oracle, ups):
    import jnifake as J
    env = J.env()
    d = [1.0, 0.5, 1 / 3, 0.25]
    shim.discardNative(env, None)
    J.begin()
    assert shim.pushNative(env, None, J.new_bytes(ups[0]), d[0]) == 1
    good = lambda: [J.new_bytes(u) for u in ups[1:4]]
    ragged, null, star = good(), good(), good()
    ragged[1] = J.new_bytes(ups[2][:-16])
    null[2] = None
    star[0] = J.new_bytes(ups[1][:500] + b"*" + ups[1][501:])
    for objs in (ragged, null, star):
        assert shim.pushBatchNative(env, None, J.new_object_array(objs), J.new_doubles(d[1:])) == 0
        assert shim.pendingNative(env, None) == 1
    assert shim.pushBatchNative(env, None, None, J.new_doubles(d[1:])) == 0
    assert shim.pushBatchNative(env, None, J.new_object_array(good()), None) == 0
    assert shim.pushBatchNative(env, None, J.new_object_array(good()), J.new_doubles(d[1:3])) == 0  # 3 uploads, 2 factors
    assert shim.pendingNative(env, None) == 1
    check_rules(J)
    J.begin()
    assert shim.pushBatchNative(env, None, J.new_object_array(good()), J.new_doubles(d[1:])) == 1
    assert J.read_bytes(shim.finishNative(env, None)) == oracle.update_faithful(ups[:4], d)
    assert shim.pendingNative(env, None) == 0
    check_rules(J)
