"""One-sample calls of the four host forms that share their bodies in net_entry.cpp
(fleet_evaluate, fleet_cifar_test, fleet_client_ex_grads, fleet_rgbnet_grads), made through
ctypes so that the library's own checks answer and not the Python layer's. Every call here is
refused before anything is launched; what comes back is (return code, fleet_last_error)."""
import numpy as np

import fleet_amd as F

FORMS = ("evaluate", "cifar_test", "client_grads", "rgbnet_grads")


def counts(form, classes=10):
    L = F.lib()
    if form in ("evaluate", "client_grads"):
        return L.fleet_teacher_weight_count(), L.fleet_teacher_bias_count()
    return L.fleet_cifar_weight_count(classes), L.fleet_cifar_bias_count(classes)


def grad_len(form, classes=10):
    return F.lib().fleet_client_grad_len() if form == "client_grads" else F.lib().fleet_rgbnet_grad_len(classes)


def refusal(codec, form, *, classes=10, sized_for=10, extra_w=0, extra_b=0, n_images=1, idx=None, shifts=None, B=1,
            upload_pitch=None):
    """The call with a model sized for `sized_for` classes plus extra_w / extra_b values, a
    dataset of n_images zero images, one client of B samples; upload_pitch: take uploads too."""
    L, h = codec._L, codec._h
    n_w, n_b = counts(form, sized_for)
    n_w, n_b = n_w + extra_w, n_b + extra_b
    feat = 28 * 28 if form in ("evaluate", "client_grads") else 3 * 32 * 32
    w, b = np.zeros(n_w, np.float32), np.zeros(n_b, np.float32)
    x, lab = np.zeros((n_images, feat), np.float32), np.zeros(n_images, np.int32)
    ix = None if idx is None else np.asarray(idx, np.int32)
    sh = None if shifts is None else np.asarray(shifts, np.int32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    head = (p(w), n_w, p(b), n_b, p(x), n_images, feat, p(lab), p(ix))
    if form in ("evaluate", "cifar_test"):
        pred, prob = np.zeros(B, np.int32), np.zeros(B, np.float32)
        if form == "evaluate":
            rc = L.fleet_evaluate(h, *head, B, None, None, None, p(pred), p(prob))
        else:
            rc = L.fleet_cifar_test(h, classes, *head, B, None, None, None, p(pred), p(prob), None, None)
    else:
        grads = np.zeros(grad_len(form, sized_for), np.float32)
        up = None if upload_pitch is None else np.zeros(upload_pitch + 16, np.uint8)
        tail = (p(grads), p(up), upload_pitch or 0)
        if form == "client_grads":
            rc = L.fleet_client_ex_grads(h, *head, p(sh), 1, B, 2.0, 0, None, None, *tail)  # cost 0: cross entropy
        else:
            rc = L.fleet_rgbnet_grads(h, classes, *head, p(sh), 1, B, 2.0, *tail)
    return rc, L.fleet_last_error(h).decode()
