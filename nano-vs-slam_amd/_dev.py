"""The torch <-> ctypes plumbing every wrapper of the C ABI shares (``_lib`` itself stays torch-free)."""
from __future__ import annotations

import ctypes as C

import torch


def ptr(t):
    """Address of a tensor's data for a pointer argument; None -> NULL."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(dev):
    """torch's current stream on ``dev`` for the ``void* stream`` argument."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def require_device(name, t, hint="pass device tensors"):
    """There is no CPU path behind the kernels: a CPU tensor raises."""
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: CPU tensors are not supported (no CPU fallback)" + (f"; {hint}" if hint else ""))
    return t


def scratch(nbytes, dev):
    """Uninitialised scratch of at least ``nbytes`` bytes, never empty (a null pointer is refused); pass ``numel()``."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def model_device(model):
    """The device a model answers on, with an explicit index."""
    dev = getattr(model, "device", None)
    dev = torch.device(next(model.parameters()).device if dev is None else dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev
