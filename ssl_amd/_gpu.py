"""Whether a call goes to the C ABI at all -- the switch of set_native_criteria and `native`: fp32 tensors on one GPU --
and how it reaches the GPU: the device that holds the call's tensors is made current, the handle of torch's current
stream on it is the entry point's last argument, and the status is checked.  The one spelling of both for the whole
package, and of the few helpers that go with them; it imports torch and ._lib only.
"""
import contextlib

import torch

from . import _lib

# the current stream's handle without a Stream object around it (a call is a handful of launches: the host's time per
# call is what is left to save); torch.cuda.current_stream() where this torch has no such function
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_NOTHING = contextlib.nullcontext()


_NATIVE_CRITERIA = True


def set_native_criteria(on):
    """The switch behind ssl_amd.losses.set_native_criteria; returns the previous setting."""
    global _NATIVE_CRITERIA
    prev, _NATIVE_CRITERIA = _NATIVE_CRITERIA, bool(on)
    return prev


def native_criteria():
    return _NATIVE_CRITERIA


def readable(*tensors):
    """Whether the kernels can be handed these tensors' addresses at all: fp32 tensors on one GPU.  Whatever the switch
    says: a tensor of another type or device must never reach the C ABI."""
    dev = None
    for t in tensors:       # (one plain loop: this runs on every call of every criterion)
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            return False
        if dev is None:
            dev = t.device
        elif t.device != dev:
            return False
    return dev is not None


def native(*tensors):
    """Whether a module's call takes the kernels, as far as every family agrees: the switch is on and the kernels can
    read the tensors.  Each family adds its own conditions ("Which calls take the kernels").  The switch is
    tested first: a deferred handle (losses/lazy.py) is refused once per image, by `isinstance`."""
    return _NATIVE_CRITERIA and readable(*tensors)


def ptr(t):
    return None if t is None else t.data_ptr()


def need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"ssl_amd: expected a GPU tensor, got device {t.device}; the SSG engine has no CPU path")


def workspace(nbytes, dev):
    """(buffer, nbytes) for a size the library reported: at least one byte, so that the pointer is never NULL."""
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def address_array(values):
    """Host addresses or element counts as the size_t array that the ragged entry points take (pass .ctypes.data)."""
    import numpy as np
    return np.ascontiguousarray(values, dtype=np.uintp)


def dense_strides(t):
    """Non-overlapping and dense: the strides are those of some permutation of a contiguous layout (contiguous,
    channels_last, any other permutation without gaps), so that one flat walk over the memory of two such tensors of
    equal strides meets corresponding elements.  Dimensions of size 1 do not count, whatever their strides.  The one
    spelling of this for the ragged kernels' callers (engine.multi_pair_is_native, ssl_amd/ema.py)."""
    expect = 1
    for stride, size in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def current_gpu(message):
    """The current GPU, where host data goes when the caller named no device; RuntimeError(message) without one."""
    if not torch.cuda.is_available():
        raise RuntimeError(message)
    return torch.device("cuda", torch.cuda.current_device())


def on(device):
    """The context in which `device` is current: nothing to do where it already is, for a `cuda` device without an index
    (it means the current one) and for a device that is no GPU (the CPU tests' stand-ins)."""
    if device.type != "cuda" or device.index is None or device.index == torch.cuda.current_device():
        return _NOTHING
    return torch.cuda.device(device)


def stream(device=None):
    """The raw handle of torch's current stream on `device` (None or no index: the current GPU); None for a device that
    is no GPU."""
    if device is not None and device.type != "cuda":
        return None
    index = device.index if device is not None and device.index is not None else torch.cuda.current_device()
    return _RAW_STREAM(index) if _RAW_STREAM else torch.cuda.current_stream(index).cuda_stream


def launch(device, fn, *args):
    """One call of the C ABI on the GPU that holds the call's tensors (whatever the current device is), on torch's
    current stream of that GPU -- the last argument of every launching entry point."""
    with on(device):
        _lib.check(fn(*args, stream(device)))
