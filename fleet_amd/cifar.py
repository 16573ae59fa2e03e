"""The Driver's ``test()`` (Driver/src/main/c++/cppNN_backend.cpp:53-75) on the reference's CIFAR
network (:128-138) -- input 32x32x3, two 3x3 convolutions with max pooling, fully connected
layers of 384 and 192, and a softmax head of 10 or 100 classes -- evaluated on the device, bit
for bit (``fleet_cifar_*`` of include/fleet_codec.h).

Module functions over a :class:`~fleet_amd.Codec`, a :class:`~fleet_amd.Model` or a
:class:`~fleet_amd.ResidentModel`; all return, or fill the tensors of, a
:class:`~fleet_amd.Evaluation`. Images are rows of at least 3072 floats, planar (channel, row,
column) as cifar_parser.h delivers them; a row's first 3072 floats are read.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import _ptr, _stream, lib
from .codec import Evaluation, _eval_device_out, _eval_host_args, _eval_host_call

PIXELS = 3072


def weight_count(classes: int) -> int:
    """Length of the weight vector (the non-null W in order): 306480 for 10 classes, 323760 for
    100, 0 for any other head."""
    return int(lib().fleet_cifar_weight_count(int(classes)))


def bias_count(classes: int) -> int:
    """Length of the bias vector (the use_bias() layers in layer order): 666, 756, or 0."""
    return int(lib().fleet_cifar_bias_count(int(classes)))


def block_images() -> int:
    """Images a block of the forward kernel takes at a time."""
    return int(lib().fleet_cifar_block_images())


class grid_override:
    """``with grid_override(2): ...`` caps the forward kernel's grid at that many blocks, so that
    a small set walks more than one grid-stride pass (tests; process-wide)."""

    def __init__(self, max_blocks: int):
        self.max_blocks = int(max_blocks)

    def __enter__(self):
        self.prev = lib().fleet_cifar_set_grid(self.max_blocks)
        return self

    def __exit__(self, *exc):
        lib().fleet_cifar_set_grid(self.prev)
        return False


def evaluate(codec, w, b, images, labels, idx=None, classes: int = 10, out=None) -> Evaluation:
    """``test()`` of the CIFAR network with weights ``w`` and biases ``b`` over ``images[idx]``
    (every image in order when ``idx`` is None): bit for bit the reference's error, accuracy,
    predictions and their probabilities. Host arrays in, synchronous. A dict given as ``out``
    receives ``costs`` [B] and ``probsN`` [B, classes]."""
    wv = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    bv = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    x, lab, ix, B = _eval_host_args(images, labels, idx)
    err, acc, cor = C.c_float(0), C.c_float(0), C.c_int32(0)
    pred, prob = np.empty(max(B, 1), np.int32), np.empty(max(B, 1), np.float32)
    cost = probs = None
    if out is not None:
        cost, probs = np.empty(max(B, 1), np.float32), np.empty((max(B, 1), max(int(classes), 1)), np.float32)
    rc = codec._L.fleet_cifar_test(codec._h, int(classes), wv.ctypes.data, len(wv), bv.ctypes.data, len(bv), x.ctypes.data,
                                   x.shape[0], x.shape[1], lab.ctypes.data, None if ix is None else ix.ctypes.data, B,
                                   C.byref(err), C.byref(acc), C.byref(cor), pred.ctypes.data, prob.ctypes.data,
                                   None if cost is None else cost.ctypes.data, None if probs is None else probs.ctypes.data)
    codec._check(rc)
    if out is not None:
        out["costs"], out["probsN"] = cost[:B], probs[:B]
    return Evaluation(np.float32(err.value), np.float32(acc.value), int(cor.value), pred[:B], prob[:B])


def _device_out(images_f32, labels_i32, idx, out, classes):
    n_img, F, B, o = _eval_device_out(images_f32, labels_i32, idx, out)
    t = o.get("probsN")
    if t is not None:
        import torch
        if t.dtype != torch.float32 or t.numel() < B * classes or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"out['probsN']: a contiguous float32 CUDA tensor of at least {B * classes} elements")
    return n_img, F, B, o


def evaluate_device(codec, w_f32, b_f32, images_f32, labels_i32, idx_i32=None, classes: int = 10, out=None,
                    stream=None) -> dict:
    """Device-resident :func:`evaluate`: CUDA tensors w, b, images [N, F >= 3072] float32, labels
    [N] int32, idx int32 or None. Runs on ``stream`` (default: torch's current) and does not
    synchronise. ``out`` may hold tensors to write -- ``predictions`` [B] int32, ``probabilities``
    [B], ``result`` [3] (float error, float accuracy, the bits of int32 correct), and optionally
    ``costs`` [B], ``probsN`` [B, classes]; ``predictions`` or ``probabilities`` given as None are
    not written. Returns the dict of tensors written (:func:`fleet_amd.evaluation_from_device`
    reads it). Index errors at ``codec.check()``."""
    classes = int(classes)
    if not weight_count(classes) or w_f32.numel() != weight_count(classes) or b_f32.numel() != bias_count(classes):
        raise ValueError("weights / biases of the wrong size, or a head that is not 10 or 100 classes")
    n_img, F, B, o = _device_out(images_f32, labels_i32, idx_i32, out, classes)
    codec._check(codec._L.fleet_cifar_test_device(codec._h, classes, w_f32.data_ptr(), b_f32.data_ptr(),
                                                  images_f32.data_ptr(), n_img, F, labels_i32.data_ptr(), _ptr(idx_i32), B,
                                                  _ptr(o.get("predictions")), _ptr(o.get("probabilities")),
                                                  _ptr(o.get("costs")), _ptr(o.get("probsN")), o["result"].data_ptr(),
                                                  _stream(stream)))
    return o


def model_evaluate(model, images, labels, idx=None, version=None) -> Evaluation:
    """:func:`evaluate` of a version of a :class:`~fleet_amd.Model` that holds the CIFAR network
    (``version`` None: the newest, -1: ``cnn``); the head's size is read from its FC2. Any other
    network is refused with FLEET_ERR_ARG, the first differing layer named."""
    rc, ev = _eval_host_call(model._L.fleet_model_cifar_test, (model._h, model._eval_version(version)), images, labels, idx)
    model._check(rc)
    return ev


def resident_evaluate(rm, images, labels, idx=None, version=None) -> Evaluation:
    """:func:`model_evaluate` from a :class:`~fleet_amd.ResidentModel`'s row where it lives: host
    images, labels and indices are uploaded, no weight crosses PCIe; returns synchronised."""
    rc, ev = _eval_host_call(rm._L.fleet_rmodel_cifar_test, (rm._h, rm._eval_version(version)), images, labels, idx)
    rm._check(rc)
    return ev


def resident_evaluate_device(rm, images_f32, labels_i32, idx=None, version=None, out=None, stream=None) -> dict:
    """:func:`resident_evaluate` on tensors where they live, on ``stream`` (default: torch's
    current), not synchronised; returns device tensors ``predictions``, ``probabilities`` and
    ``result`` as :func:`evaluate_device` does. Index errors at ``codec.check()``."""
    n_img, F, B, o = _eval_device_out(images_f32, labels_i32, idx, out)
    rm._check(rm._L.fleet_rmodel_cifar_test_device(rm._h, rm._eval_version(version), images_f32.data_ptr(), n_img, F,
                                                   labels_i32.data_ptr(), _ptr(idx), B, _ptr(o.get("predictions")),
                                                   _ptr(o.get("probabilities")), o["result"].data_ptr(),
                                                   _stream(stream)))
    return o
