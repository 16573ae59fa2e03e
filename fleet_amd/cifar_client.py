"""The client's gradients on the reference's CIFAR-10/100 network: what
``cnn.gradients()`` returns after B ``train_class`` calls, for C clients in one launch sequence,
with the cross-entropy cost (``fleet_rgbnet_*`` of include/fleet_codec.h), or, for the clients given
a ``sigma`` > 0, what ``cnn.DPgradients(clip, sigma)`` returns (``fleet_rgb_dp_*``).

* :func:`client_gradients` -- host buffers, one model, on a :class:`~fleet_amd.Codec`;
* :func:`client_gradients_device` -- tensors where they live, any number of model rows;
* :func:`resident_client_gradients_device` -- the models taken from a
  :class:`~fleet_amd.ResidentModel`'s versions, so that a CIFAR model trains, steps
  (``descent_device``) and is evaluated (:func:`fleet_amd.cifar.resident_evaluate_device`)
  without leaving HBM;
* :func:`grad_len`, :func:`sample_tile`, :class:`chunk_override`, :func:`dp_noise_table`.

The shifts are :func:`fleet_amd.client.client_shifts`'s and the upload rows' texts
:func:`fleet_amd.client.upload_texts` (with ``grad_len(classes)``). ``clip`` and ``sigma`` are
:mod:`fleet_amd.client`'s keywords, a scalar or one value per client; left at None a call is the
one it was before they existed. The distillation cost exists on the MNIST network only."""
from __future__ import annotations

import numpy as np

from ._capi import _ptr, _stream, b64_len, lib
from .cifar import PIXELS, bias_count, weight_count
from .client import _fptr, ex_args, host_args


def grad_len(classes: int) -> int:
    """Values of one client's row: ``layouts.CIFAR10.n_up`` = 313867, ``CIFAR100.n_up`` =
    331237; 0 for any other number of classes."""
    return int(lib().fleet_rgbnet_grad_len(int(classes)))


def sample_tile() -> int:
    """Samples the fully connected dW kernel stages at a time (tests: B at and above it)."""
    return int(lib().fleet_rgbnet_sample_tile())


class chunk_override:
    """``with chunk_override(2): ...`` walks the clients of a call at most two at a time, so that
    a small fleet runs the chunk walk and its tail (tests; process-wide)."""

    def __init__(self, max_clients: int):
        self.max_clients = int(max_clients)

    def __enter__(self):
        self.prev = lib().fleet_rgbnet_set_chunk(self.max_clients)
        return self

    def __exit__(self, *exc):
        lib().fleet_rgbnet_set_chunk(self.prev)
        return False


def dp_noise_table(n: int = None) -> np.ndarray:
    """float64 [n] (default all ``grad_len(100)`` = 331237): the standard-normal draws a DP call
    adds to the slots of its vector before scaling them by ``clip * sigma``:
    :func:`fleet_amd.client.dp_noise_table`'s sequence continued, slot i taking draw i."""
    n = grad_len(100) if n is None else int(n)
    out = np.empty(n, np.float64)
    if lib().fleet_rgb_dp_noise(out.ctypes.data, n) != 0:
        raise ValueError(f"at most {grad_len(100)} draws")
    return out


def _dp(clip, sigma, C):
    """(clip float32[C], sigma float32[C]) of a call's keywords, or None for the plain call"""
    ex = ex_args("cross_entropy", clip, sigma, C)
    return None if ex is None else ex[1:]


def _need_classes(classes) -> int:
    classes = int(classes)
    if grad_len(classes) == 0:
        raise ValueError("classes: 10 or 100")
    return classes


def client_gradients(codec, classes, w, b, images, labels, idx=None, shifts=None, temperature=2.0, uploads=False, *,
                     clip=None, sigma=None):
    """float32 [C, grad_len(classes)]: the rows of :func:`fleet_amd.client.client_gradients` on
    the CIFAR network with weights ``w`` and biases ``b`` (:func:`fleet_amd.cifar.weight_count`,
    ``bias_count``); images [N, >= 3072] planar. With ``uploads``: (rows, [bytes]). ``clip`` and
    ``sigma``: a client with sigma > 0 gets ``cnn.DPgradients(clip, sigma)``'s vector."""
    classes = _need_classes(classes)
    wv = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    bv = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    x, lab, ix, sh, C, B = host_args(images, labels, idx, shifts)
    n = grad_len(classes)
    grads = np.empty((max(C, 1), n), np.float32)
    pitch = b64_len(n)
    up = np.zeros((max(C, 1), pitch), np.uint8) if uploads else None
    head = (codec._live(), classes, wv.ctypes.data, len(wv), bv.ctypes.data, len(bv), x.ctypes.data, x.shape[0],
            x.shape[1], lab.ctypes.data, None if ix is None else ix.ctypes.data, None if sh is None else sh.ctypes.data,
            C, B, float(temperature))
    tail = (grads.ctypes.data, None if up is None else up.ctypes.data, pitch)
    dp = _dp(clip, sigma, C)
    if dp is None:
        codec._check(codec._L.fleet_rgbnet_grads(*head, *tail))
    else:
        codec._check(codec._L.fleet_rgb_dp_grads(*head, _fptr(dp[0]), _fptr(dp[1]), *tail))
    return (grads, [up[c].tobytes() for c in range(C)]) if uploads else grads


def _device_args(classes, images_f32, labels_i32, idx, shifts, C, B, grads, uploads):
    """:func:`fleet_amd.client.device_args` for a row of grad_len(classes) values"""
    import torch
    if images_f32.dim() != 2 or images_f32.shape[1] < PIXELS or labels_i32.numel() != images_f32.shape[0]:
        raise ValueError(f"images [N, >= {PIXELS}] and one label per image")
    for t, dt, name in ((images_f32, torch.float32, "images"), (labels_i32, torch.int32, "labels"),
                        (idx, torch.int32, "idx"), (shifts, torch.int32, "shifts")):
        if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous {dt} CUDA tensor")
    if idx is not None:
        if idx.dim() != 2:
            raise ValueError("idx [C, B]")
        C, B = idx.shape
    elif shifts is not None and C is None:
        C, B = shifts.shape[:2]
    if C is None or B is None:
        raise ValueError("C and B, or idx [C, B]")
    C, B = int(C), int(B)
    if shifts is not None and tuple(shifts.shape) != (C, B, 2):
        raise ValueError("shifts [C, B, 2]")
    n, dev = grad_len(classes), images_f32.device
    groups = 16 * ((n + 2) // 3)
    if grads is None:
        grads = torch.empty((C, n), dtype=torch.float32, device=dev)
    if grads.dtype != torch.float32 or not grads.is_cuda or grads.dim() != 2 or grads.shape[0] < C or \
            grads.shape[1] < n or grads.stride(1) != 1:
        raise ValueError(f"grads: a float32 CUDA tensor [C, >= {n}] with unit stride along a row")
    if uploads is True:
        uploads = torch.empty((C, groups), dtype=torch.uint8, device=dev)
    elif uploads is False:
        uploads = None
    if uploads is not None and (uploads.dtype != torch.uint8 or not uploads.is_cuda or uploads.dim() != 2 or
                                uploads.shape[0] < C or uploads.stride(1) != 1 or uploads.stride(0) % 16 or
                                uploads.shape[1] < groups):
        raise ValueError("uploads: a uint8 CUDA tensor [C, pitch], pitch a multiple of 16 holding whole groups")
    tail = (grads.data_ptr(), grads.stride(0), _ptr(uploads), 0 if uploads is None else uploads.stride(0))
    return images_f32.shape[0], images_f32.shape[1], C, B, grads, uploads, tail


def client_gradients_device(codec, classes, models_f32, images_f32, labels_i32, idx=None, shifts=None,
                            model_of_client=None, C=None, B=None, temperature=2.0, grads=None, uploads=False,
                            stream=None, *, clip=None, sigma=None):
    """Device-resident :func:`client_gradients`, the tensors of
    :func:`fleet_amd.client.client_gradients_device`: models [rows, >= weights + biases] (w then
    b per row), images [N, F >= 3072]. Runs on ``stream`` (default: torch's current) and does
    not synchronise; index errors and a NaN forward at ``codec.check()``. Returns the rows
    [C, grad_len(classes)], or (rows, upload rows [C, pitch] uint8) with ``uploads``."""
    import torch
    classes = _need_classes(classes)
    if models_f32.dim() == 1:
        models_f32 = models_f32.reshape(1, -1)
    need = weight_count(classes) + bias_count(classes)
    if models_f32.dtype != torch.float32 or not models_f32.is_cuda or models_f32.dim() != 2 or \
            models_f32.shape[1] < need or models_f32.stride(1) != 1:
        raise ValueError(f"models: a float32 CUDA tensor [rows, >= {need}] (w then b per row)")
    if model_of_client is not None and (model_of_client.dtype != torch.int32 or not model_of_client.is_cuda or
                                        not model_of_client.is_contiguous()):
        raise ValueError("model_of_client: a contiguous int32 CUDA tensor [C]")
    n_img, F, C, B, grads, up, tail = _device_args(classes, images_f32, labels_i32, idx, shifts, C, B, grads, uploads)
    if model_of_client is not None and model_of_client.numel() != C:
        raise ValueError("model_of_client: one row per client")
    head = (codec._live(), classes, models_f32.data_ptr(), models_f32.stride(0), models_f32.shape[0],
            _ptr(model_of_client), images_f32.data_ptr(), n_img, F, labels_i32.data_ptr(), _ptr(idx), _ptr(shifts), C, B,
            float(temperature))
    dp = _dp(clip, sigma, C)
    if dp is None:
        codec._check(codec._L.fleet_rgbnet_grads_device(*head, *tail, _stream(stream)))
    else:
        codec._check(codec._L.fleet_rgb_dp_grads_device(*head, _fptr(dp[0]), _fptr(dp[1]), *tail, _stream(stream)))
    return (grads, up) if up is not None else grads


def resident_client_gradients_device(rm, classes, versions, images_f32, labels_i32, idx=None, shifts=None,
                                     uploads=False, C=None, B=None, temperature=2.0, grads=None, stream=None, *,
                                     clip=None, sigma=None):
    """The gradients C clients compute on versions of the resident CIFAR model ``rm`` (of
    ``classes`` classes), where the versions live; ``versions`` as
    :func:`fleet_amd.client.resident_client_gradients_device` takes them. Returns the fp32 rows
    and, with ``uploads``, the upload rows ``update_device`` and ``Pool.put_device`` take."""
    classes = _need_classes(classes)
    n_img, F, C, B, grads, up, tail = _device_args(classes, images_f32, labels_i32, idx, shifts, C, B, grads, uploads)
    vs = [versions] * C if versions is None or np.isscalar(versions) else list(versions)
    if len(vs) != C:
        raise ValueError("one version per client")
    v = np.array([rm._eval_version(x) for x in vs], np.int32)
    head = (rm._live(), v.ctypes.data, images_f32.data_ptr(), n_img, F, labels_i32.data_ptr(), _ptr(idx), _ptr(shifts),
            C, B, float(temperature))
    dp = _dp(clip, sigma, C)
    if dp is None:
        rm._check(rm._L.fleet_rmodel_rgbnet_grads_device(*head, *tail, _stream(stream)))
    else:
        rm._check(rm._L.fleet_rmodel_rgb_dp_grads_device(*head, _fptr(dp[0]), _fptr(dp[1]), *tail, _stream(stream)))
    return (grads, up) if up is not None else grads
