"""The loop every ``load_state_dict`` of the avatar-head modules runs over a fresh handle of the C API."""
import ctypes as C

import numpy as np
import torch

from . import capi


def load_tensors(L, prefix, h, items, errors=None):
    """Hands every ``(key, value)`` of ``items`` to ``artalk_<prefix>_set_tensor`` as contiguous fp32 on the host and, when none was
    refused, calls ``artalk_<prefix>_finalize``.  Returns the messages of what went wrong, in order (``errors``, when given, is the
    list they are added to); the caller raises and decides what becomes of the handle."""
    errors = [] if errors is None else errors
    set_tensor, finalize, last_error = (getattr(L, f"artalk_{prefix}_{f}") for f in ("set_tensor", "finalize", "last_error"))
    for key, val in items:
        t = val.detach().cpu() if isinstance(val, torch.Tensor) else torch.from_numpy(np.asarray(val))
        t = t.to(torch.float32).contiguous()
        shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
        if set_tensor(h, key.encode(), C.c_void_p(t.data_ptr()), t.dim(), shape) != capi.OK:
            errors.append(last_error(h).decode())
    if not errors and finalize(h) != capi.OK:
        errors.append(last_error(h).decode())
    return errors
