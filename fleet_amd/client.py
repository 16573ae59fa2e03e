"""The client's gradients: what ``cnn.gradients()`` returns after B
``train_class`` calls (Client/app/src/main/cpp/cppNN-lib.cpp:101-113, 218-234), for C clients in
one launch sequence.

* :func:`client_gradients` -- host buffers, one model, on a :class:`~fleet_amd.Codec`;
* :func:`client_gradients_device` -- tensors where they live, any number of model rows;
* :func:`resident_client_gradients_device` -- the models taken from a
  :class:`~fleet_amd.ResidentModel`'s versions;
* :func:`client_shifts` -- the ``rand()`` draw of the shifts; :class:`client_chunk_override`
  and :func:`upload_texts` for tests and callers of the upload rows;
* :func:`dp_noise_table` -- the draws ``addGaussian`` adds, before scaling.

The three gradient functions take the keyword-only ``cost`` ("cross_entropy", or "distillation"
for the client built with DISTILLATION_MODE 1, cppNN-lib.cpp:251-252) and ``clip`` / ``sigma``
(a scalar or one value per client; ``sigma`` > 0 is ``cnn.DPgradients(clip, sigma)``,
cppNN-lib.cpp:218-219). Left at their defaults a call is the one it was before they existed.

They are functions of this module rather than methods: the package's recorded surface
(tests/api_surface.json) admits new modules only."""
from __future__ import annotations

import numpy as np

from ._capi import _ptr, _stream, b64_len, lib

SHIFT_RANGE = (-1, 0, 1)


def client_grad_len() -> int:
    """Values of one client's row: ``layouts.MNIST.n_up`` = 22961."""
    return int(lib().fleet_client_grad_len())


class client_chunk_override:
    """``with client_chunk_override(2): ...`` walks the clients of a call at most two at a time,
    so that a small fleet runs the chunk walk and its tail (tests; process-wide, as
    :class:`~fleet_amd.evaluate_grid_override`)."""

    def __init__(self, max_clients: int):
        self.max_clients = int(max_clients)

    def __enter__(self):
        self.prev = lib().fleet_client_grad_set_chunk(self.max_clients)
        return self

    def __exit__(self, *exc):
        lib().fleet_client_grad_set_chunk(self.prev)
        return False


def client_shifts(seed_or_stream, C: int, B: int) -> np.ndarray:
    """int32 [C, B, 2] = (dx, dy) per sample as train_class draws them (network.h:1840:
    ``m.shift((rand() % 3) - 1, (rand() % 3) - 1, augment_pad)``), clients and samples in order.
    ``seed_or_stream``: an int seeds libc's generator first (``srand``, cppNN-lib.cpp:277 uses 1);
    a callable is drawn from as ``rand()``. C++ leaves the order of the two draws open; the
    reference's g++ build evaluates the arguments right to left, so the first draw of a sample
    is dy and the second dx (the recorded fixture, tests/golden/client_grad_ref.npz, shows it)."""
    if callable(seed_or_stream):
        rand = seed_or_stream
    else:
        from .sampler import _rand as rand, srand
        srand(int(seed_or_stream))
    out = np.empty((int(C), int(B), 2), np.int32)
    for c in range(int(C)):
        for k in range(int(B)):
            dy = rand() % 3 - 1
            dx = rand() % 3 - 1
            out[c, k] = (dx, dy)
    return out


def host_args(images, labels, idx, shifts):
    """(images [N, F], labels [N], idx [C, B] or None, shifts [C, B, 2] or None, C, B) of a
    host call: without idx the images are one client's B samples; idx [B] is one client."""
    x = np.ascontiguousarray(images, dtype=np.float32)
    if x.ndim == 1:
        x = x.reshape(1, -1)
    lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    if x.ndim != 2 or len(lab) != x.shape[0]:
        raise ValueError("images [N, F] and one label per image")
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    if ix is not None and ix.ndim == 1:
        ix = ix.reshape(1, -1)
    sh = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.int32)
    if sh is not None and sh.ndim == 2:
        sh = sh.reshape(1, -1, 2)
    if ix is not None:
        C, B = ix.shape
    elif sh is not None:
        C, B = sh.shape[:2]
    else:
        C, B = 1, x.shape[0]
    if ix is not None and ix.ndim != 2 or sh is not None and sh.shape != (C, B, 2):
        raise ValueError("idx [C, B] and shifts [C, B, 2]")
    return x, lab, ix, sh, int(C), int(B)


def device_args(images_f32, labels_i32, idx, shifts, C, B, grads, uploads):
    """checks the tensors of a device call and makes the outputs: (n_images, F, C, B, grads,
    uploads or None). ``uploads``: False / None, True (allocate) or a uint8 tensor [C, pitch]."""
    import torch
    if images_f32.dim() != 2 or labels_i32.numel() != images_f32.shape[0]:
        raise ValueError("images [N, F] and one label per image")
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
    n = client_grad_len()
    dev = images_f32.device
    if grads is None:
        grads = torch.empty((C, n), dtype=torch.float32, device=dev)
    if grads.dtype != torch.float32 or not grads.is_cuda or grads.dim() != 2 or grads.shape[0] < C or \
            grads.shape[1] < n or grads.stride(1) != 1:
        raise ValueError(f"grads: a float32 CUDA tensor [C, >= {n}] with unit stride along a row")
    if uploads is True:
        uploads = torch.empty((C, 16 * ((n + 2) // 3)), dtype=torch.uint8, device=dev)
    elif uploads is False:
        uploads = None
    if uploads is not None and (uploads.dtype != torch.uint8 or not uploads.is_cuda or uploads.dim() != 2 or
                                uploads.shape[0] < C or uploads.stride(1) != 1 or uploads.stride(0) % 16 or
                                uploads.shape[1] < 16 * ((n + 2) // 3)):
        raise ValueError("uploads: a uint8 CUDA tensor [C, pitch], pitch a multiple of 16 holding whole groups")
    return images_f32.shape[0], images_f32.shape[1], C, B, grads, uploads


def upload_texts(uploads) -> list:
    """The Base64 texts of upload rows (device or host), one ``bytes`` per client."""
    n = b64_len(client_grad_len())
    a = uploads.cpu().numpy() if hasattr(uploads, "cpu") else np.asarray(uploads)
    return [a[c, :n].tobytes() for c in range(a.shape[0])]


COSTS = {"cross_entropy": 0, "distillation": 1}


def dp_noise_table(n: int = None) -> np.ndarray:
    """float64 [n] (default all 22961): the standard-normal draws ``addGaussian`` adds to the
    slots of a DP vector, before it scales them by ``C * sigma`` (commonLib/cppNN/network.h:
    1125-1130): the same on every call, as the reference constructs its engine anew each time.
    Host only; they come from the C++ library this package is built with."""
    n = client_grad_len() if n is None else int(n)
    out = np.empty(n, np.float64)
    if lib().fleet_client_dp_noise(out.ctypes.data, n) != 0:
        raise ValueError(f"at most {client_grad_len()} draws")
    return out


def ex_args(cost, clip, sigma, C):
    """(cost code, clip float32[C] or None, sigma float32[C] or None) of a call's keywords, or
    None where all three are the defaults (the call is then the one without them)."""
    if cost == "cross_entropy" and clip is None and sigma is None:
        return None
    if cost not in COSTS:
        raise ValueError(f"cost: one of {sorted(COSTS)}")
    if (clip is None) != (sigma is None):
        raise ValueError("clip and sigma: both or neither")

    def per_client(v):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float32)
        a = np.full(C, a, np.float32) if a.ndim == 0 else np.ascontiguousarray(a.reshape(-1))
        if len(a) != C:
            raise ValueError("clip and sigma: a scalar or one value per client")
        return a
    return COSTS[cost], per_client(clip), per_client(sigma)


def _fptr(a):
    return None if a is None else a.ctypes.data


def client_gradients(codec, w, b, images, labels, idx=None, shifts=None, temperature=2.0, uploads=False, *,
                     cost="cross_entropy", clip=None, sigma=None):
    """What ``cnn.gradients()`` returns after ``train_class`` on each sample of a client's
    mini-batch (Client/app/src/main/cpp/cppNN-lib.cpp:101-113, 218-234), bit for bit, for the
    MNIST network with weights ``w`` and biases ``b``: float32 [C, 22961]. ``idx`` [C, B] picks
    every client's samples from ``images`` (None: one client, every image in order), ``shifts``
    [C, B, 2] their (dx, dy) in {-1, 0, 1} (None: no shift; :func:`client_shifts` draws them as
    the reference does). ``temperature`` 2 is the client's call. With ``uploads`` the Base64
    upload of every row is returned too: (rows, [bytes])."""
    L, h = codec._L, codec._live()
    wv = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    bv = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    x, lab, ix, sh, C, B = host_args(images, labels, idx, shifts)
    n = client_grad_len()
    grads = np.empty((max(C, 1), n), np.float32)
    pitch = b64_len(n)
    up = np.zeros((max(C, 1), pitch), np.uint8) if uploads else None
    head = (h, wv.ctypes.data, len(wv), bv.ctypes.data, len(bv), x.ctypes.data, x.shape[0], x.shape[1], lab.ctypes.data,
            None if ix is None else ix.ctypes.data, None if sh is None else sh.ctypes.data, C, B, float(temperature))
    tail = (grads.ctypes.data, None if up is None else up.ctypes.data, pitch)
    ex = ex_args(cost, clip, sigma, C)
    if ex is None:
        codec._check(L.fleet_client_grads(*head, *tail))
    else:
        codec._check(L.fleet_client_ex_grads(*head, ex[0], _fptr(ex[1]), _fptr(ex[2]), *tail))
    return (grads, [up[c].tobytes() for c in range(C)]) if uploads else grads


def client_gradients_device(codec, models_f32, images_f32, labels_i32, idx=None, shifts=None, model_of_client=None,
                            C=None, B=None, temperature=2.0, grads=None, uploads=False, stream=None, *,
                            cost="cross_entropy", clip=None, sigma=None):
    """Device-resident :func:`client_gradients`: CUDA tensors models [rows, >= 21530] (w then b
    per row), images [N, F >= 784] float32, labels [N] int32, idx [C, B] int32 or None (images
    c*B + k; give C and B), shifts [C, B, 2] int32 or None, model_of_client [C] int32 or None
    (row 0). Runs on ``stream`` (default: torch's current) and does not synchronise; index
    errors and a NaN forward at ``codec.check()``. Returns the rows [C, 22961], or (rows, upload
    rows [C, pitch] uint8) with ``uploads`` (True, or a tensor to write)."""
    import torch
    L, h = codec._L, codec._live()
    if models_f32.dim() == 1:
        models_f32 = models_f32.reshape(1, -1)
    need = L.fleet_teacher_weight_count() + L.fleet_teacher_bias_count()
    if models_f32.dtype != torch.float32 or not models_f32.is_cuda or models_f32.dim() != 2 or \
            models_f32.shape[1] < need or models_f32.stride(1) != 1:
        raise ValueError(f"models: a float32 CUDA tensor [rows, >= {need}] (w then b per row)")
    if model_of_client is not None and (model_of_client.dtype != torch.int32 or not model_of_client.is_cuda or
                                        not model_of_client.is_contiguous()):
        raise ValueError("model_of_client: a contiguous int32 CUDA tensor [C]")
    n_img, F, C, B, grads, up = device_args(images_f32, labels_i32, idx, shifts, C, B, grads, uploads)
    if model_of_client is not None and model_of_client.numel() != C:
        raise ValueError("model_of_client: one row per client")
    head = (h, models_f32.data_ptr(), models_f32.stride(0), models_f32.shape[0], _ptr(model_of_client),
            images_f32.data_ptr(), n_img, F, labels_i32.data_ptr(), _ptr(idx), _ptr(shifts), C, B, float(temperature))
    tail = (grads.data_ptr(), grads.stride(0), _ptr(up), 0 if up is None else up.stride(0), _stream(stream))
    ex = ex_args(cost, clip, sigma, C)
    if ex is None:
        codec._check(L.fleet_client_grads_device(*head, *tail))
    else:
        codec._check(L.fleet_client_ex_grads_device(*head, ex[0], _fptr(ex[1]), _fptr(ex[2]), *tail))
    return (grads, up) if up is not None else grads


def resident_client_gradients_device(rm, versions, images_f32, labels_i32, idx=None, shifts=None, uploads=False,
                                     C=None, B=None, temperature=2.0, grads=None, stream=None, *,
                                     cost="cross_entropy", clip=None, sigma=None):
    """The gradients C clients compute on versions of the resident model ``rm``, where the
    versions live (:func:`client_gradients_device` names the tensors). ``versions``: one per
    client, or one for all: a version index, -1 for ``cnn``, None for the newest; a client on
    an older version is FLeet's staleness. Returns the fp32 rows [C, 22961] and, with
    ``uploads``, the upload rows ``update_device`` and ``Pool.put_device`` take."""
    n_img, F, C, B, grads, up = device_args(images_f32, labels_i32, idx, shifts, C, B, grads, uploads)
    vs = [versions] * C if versions is None or np.isscalar(versions) else list(versions)
    if len(vs) != C:
        raise ValueError("one version per client")
    v = np.array([rm._eval_version(x) for x in vs], np.int32)
    head = (rm._live(), v.ctypes.data, images_f32.data_ptr(), n_img, F, labels_i32.data_ptr(), _ptr(idx), _ptr(shifts),
            C, B, float(temperature))
    tail = (grads.data_ptr(), grads.stride(0), _ptr(up), 0 if up is None else up.stride(0), _stream(stream))
    ex = ex_args(cost, clip, sigma, C)
    if ex is None:
        rm._check(rm._L.fleet_rmodel_client_grads_device(*head, *tail))
    else:
        rm._check(rm._L.fleet_rmodel_client_ex_grads_device(*head, ex[0], _fptr(ex[1]), _fptr(ex[2]), *tail))
    return (grads, up) if up is not None else grads
