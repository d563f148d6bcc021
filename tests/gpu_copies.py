"""Host <-> device copies for every GPU test: through hostpipe's pinned
buffers, like the product, so no test adds a pageable DMA to a process that
may hold registered host memory (DESIGN.md sections 7 and 13).  GPU tests move
arrays only through these helpers; tests/test_gpu_copies_rule.py keeps it so."""
import numpy as np
import torch

DEV = "cuda:0"


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _dev(x, misalign=False, device=DEV):
    """``x`` flat on ``device`` (None stays None); ``misalign``: offset by
    one element, so the vector is element-aligned only."""
    from sfl_amd import hostpipe as H

    if x is None:
        return None
    flat = H.h2d(np.ascontiguousarray(x).reshape(-1), torch.device(device))
    if not misalign:
        return flat
    t = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=device)  # element-aligned only
    t[1:].copy_(flat)
    return t[1:]


def _host(t):
    from sfl_amd import hostpipe as H

    return H.d2h(t, pooled=False)


def _u64(t):
    """Host uint64 view of a uint64-carrying int64 device tensor."""
    return _host(t).view(np.uint64)


def _item(t):
    """The Python value of a one-element device tensor."""
    return _host(t).item()
