"""Host <-> device copies for the GPU tests of the compression kernels
(test_gpu_stc.py, test_gpu_scr.py): through hostpipe's pinned buffers, like
the product, so the tests add no pageable DMA to a process that may hold
registered host memory (DESIGN.md sections 7 and 13)."""
import numpy as np
import torch

DEV = "cuda:0"


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _dev(x, misalign=False):
    """``x`` flat on the device (None stays None); ``misalign``: offset by
    one element, so the vector is element-aligned only."""
    from sfl_amd import hostpipe as H

    if x is None:
        return None
    flat = H.h2d(np.ascontiguousarray(x).reshape(-1), torch.device(DEV))
    if not misalign:
        return flat
    t = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=DEV)  # element-aligned only
    t[1:].copy_(flat)
    return t[1:]


def _host(t):
    from sfl_amd import hostpipe as H

    return H.d2h(t, pooled=False)
