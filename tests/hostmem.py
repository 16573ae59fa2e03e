"""Page-locked host arrays for the copy-free ingress tests (fleet_host_register,
registerDirectNative). The rows are ALLOCATED page-locked, as a long-lived upload
buffer is: a driver that cannot lock memory a process already has (hipHostRegister
fails on some virtual machines) still DMAs from these. TEST INFRASTRUCTURE ONLY."""
import numpy as np


def page_locked(shape, fill: int = 0) -> np.ndarray:
    """A uint8 array of `shape` in memory allocated page-locked (torch's pinned
    allocator, hipHostMalloc); the array keeps the allocation alive."""
    import torch
    t = torch.empty(tuple(np.atleast_1d(shape)), dtype=torch.uint8, pin_memory=True).fill_(fill)
    assert t.is_pinned()
    return t.numpy()
