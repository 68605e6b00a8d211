"""What every ctypes wrapper of the package needs from a tensor: its address, the handle of the current stream, and the fp32 form
the kernels read.  Imports torch, ctypes and _abi only -- never ops, so that a wrapper of the loss or optimiser kernels does not
import the render's autograd module to get a pointer cast.
"""
import ctypes as C

import torch

from . import _abi


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _launch(name, device, *args):
    """One library entry on the current stream of `device` (made the current device for the call): name(*args, stream), checked."""
    with torch.cuda.device(device):
        _abi.check(getattr(_abi.lib(), name)(*args, _stream_ptr(device)), name)


def _f32(t, shape, name):
    """Detached, contiguous fp32 view/copy of a tensor argument (reference tensors are already fp32 contiguous)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    # (the usual case first: an fp32, contiguous, aligned GPU tensor of the right shape is used as it stands -- only its
    #  address travels to the library, autograd never sees it)
    if t.dtype is torch.float32 and t.is_cuda and t.shape == shape and t.is_contiguous() and not t.data_ptr() % 16:
        return t
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the MI355X rasterizer needs GPU tensors (there is no CPU fallback)")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    t = t.contiguous()
    if t.data_ptr() % 16:            # the kernels stage rows with 16-byte accesses (views into a larger storage may be offset)
        t = t.clone()
    return t


def _gpu_f32(t, name, who):
    """`t` as it stands, for the wrappers that convert nothing (`who`: knn, filter3d): anything but a contiguous fp32 GPU tensor raises."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{who} needs contiguous fp32 GPU tensors ({name}; there is no CPU fallback)")
    return t
