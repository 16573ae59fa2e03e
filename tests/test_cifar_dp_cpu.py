"""DPgradients on the CIFAR network without a GPU: the entry points are declared, exported and
refuse a NULL context; the noise table continues MNIST's; the Python keywords left at their
defaults make the call made before they existed; and the host form of the arithmetic
(tests/native/check_cifar_dp.cpp over fleet_amd/csrc/cifar_backward.h, built plainly and under the
host sanitizers) equals the numpy reference of test_gpu_cifar_dp.py in bits."""
import os
import subprocess

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd import cifar_client as K
from fleet_amd import client as M

import cifar_grad_ref as G
from test_client_dp_cpu import _FakeCodec
from test_gpu_cifar_dp import _reference, _same

NEW = ["fleet_rgb_dp_grads", "fleet_rgb_dp_grads_device", "fleet_rgb_dp_noise", "fleet_rmodel_rgb_dp_grads_device"]


def test_entry_points_are_declared_exported_and_refuse_a_null_context():
    declared, L = F.exported_symbols_from_header(), F.lib()
    assert sorted(s for s in declared if "rgb_dp" in s) == NEW
    assert all(hasattr(L, s) for s in NEW)
    one = np.ones(1, np.float32).ctypes.data
    assert L.fleet_rgb_dp_grads(None, 10, one, 306480, one, 666, one, 2, 3072, one, None, None, 1, 2, 2.0, one, one, one,
                                None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_rgb_dp_grads_device(None, 10, 1, 307146, 1, None, 1, 2, 3072, 1, None, None, 1, 2, 2.0, one, one, 1,
                                       313867, None, 0, None) == F.FLEET_ERR_ARG
    assert L.fleet_rmodel_rgb_dp_grads_device(None, None, 1, 2, 3072, 1, None, None, 1, 2, 2.0, one, one, 1, 313867, None,
                                              0, None) == F.FLEET_ERR_ARG


def test_noise_table_continues_the_mnist_table():
    t = K.dp_noise_table()
    assert t.shape == (K.grad_len(100),) and t.dtype == np.float64
    head = M.dp_noise_table()
    assert np.array_equal(t[:len(head)].view(np.uint64), head.view(np.uint64))
    assert np.array_equal(K.dp_noise_table(len(head) + 7), t[:len(head) + 7])  # the same on a second call
    with pytest.raises(ValueError):
        K.dp_noise_table(K.grad_len(100) + 1)


@pytest.mark.parametrize("kw,name,n_args", [(dict(), "fleet_rgbnet_grads", 18), (dict(clip=None, sigma=None), "fleet_rgbnet_grads", 18),
                                            (dict(clip=2.0, sigma=[0.0, 0.5]), "fleet_rgb_dp_grads", 20)])
def test_keywords_route_to_the_entry_point(kw, name, n_args):
    w, b = np.zeros(306480, np.float32), np.zeros(666, np.float32)
    x, lab = np.zeros((4, 3072), np.float32), np.zeros(4, np.int32)
    c = _FakeCodec()
    K.client_gradients(c, 10, w, b, x, lab, idx=np.array([[0, 1], [2, 3]], np.int32), **kw)
    (got, args), = c._L.calls
    assert got == name and len(args) == n_args and args[12:15] == (2, 2, 2.0)
    with pytest.raises(ValueError):
        K.client_gradients(c, 10, w, b, x, lab, clip=1.0)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
@pytest.mark.parametrize("classes,B", [(10, 3), (100, 2)])
def test_host_form_against_the_numpy_reference(tmp_path, flags, classes, B):
    from test_native_math import _clang
    plain = G.build_checker(tmp_path)
    assert plain is not None, "no clang++ for the host mirror"
    exe = str(tmp_path / "check_cifar_dp")
    subprocess.check_call([_clang(), "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", *flags,
                           os.path.join(G.ROOT, "tests", "native", "check_cifar_dp.cpp"), "-o", exe])
    (w, b), x = G.model(classes, classes), G.images(classes + 1, B)
    lab, sh = np.arange(B, dtype=np.int32), np.array([(-1, 1), (1, 0), (0, -1)][:B], np.int32)
    rows = G.mirror(plain, tmp_path, [(classes, w, b, x[k:k + 1], lab[k:k + 1], sh[k:k + 1], 2.0) for k in range(B)])
    sigma = np.array([1 / 128], np.float32)
    clip, want = _reference(classes, np.stack([r for r, _ in rows])[None], sigma, K.dp_noise_table())
    np.concatenate([clip, sigma]).astype(np.float32).tofile(str(tmp_path / "grad_in.bin.dp"))
    (got, blown), = G.mirror(exe, tmp_path, [(classes, w, b, x, lab, sh, 2.0)])
    assert blown == 0
    _same(got, want[0], (classes, B))
