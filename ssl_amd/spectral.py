"""Spectral normalisation of a discriminator's layers as one call per forward, on the kernels of
ssl_amd/csrc/ssg_specnorm.hip (include/ssg_hip.h section (Y)).

torch.nn.utils.spectral_norm hangs a forward-pre-hook on every wrapped layer; in training mode each hook runs two mv +
normalize, two clones, a third mv, a dot and a full-size divide, per layer and per forward, and autograd walks the chain
back.  basicsr's UNetDiscriminatorSN and KAIR's Discriminator_UNet / Discriminator_PatchGAN / Discriminator_VGG_128_SN
wrap their layers that way.  `fuse_spectral_norm(net)` keeps torch's modules, parameters (`weight_orig`), buffers
(`weight_u`, `weight_v`), state_dict keys and load hooks, and `remove_spectral_norm`, and replaces the per-layer chains by
ONE autograd.Function over the whole layer set: three launches per training forward, two per eval forward, two per
backward, whatever the number of layers.

    handle = fuse_spectral_norm(net)      # the hooks of the layers with dim == 0 and n_power_iterations == 1 go quiet
    net(x)                                # one forward-pre-hook of `net` refreshes every layer's `weight`
    handle.unfuse()                       # torch's hooks again

Semantics are torch's SpectralNorm.compute_weight: u and v are updated in place in training mode (also under
torch.no_grad() and when the weights do not require grad -- the generator's step) and left alone in eval mode; they are
constants for autograd.  Every forward allocates its own saved block of u, v and sigma, so `D(real) - D(fake)` followed by
one backward() sees each forward's own vectors (what torch's clones are for).

The native domain: a layer is native when weight_orig, weight_u and weight_v are fp32 on one GPU and contiguous, eps is
torch's 1e-12, and `ssl_amd.losses.set_native_criteria` is on (`_gpu.native`, the one place for it).  Any other layer of
the set -- CPU, fp64, half -- runs torch's own hook on that forward and gives torch's bits; layers with dim != 0
(transposed convolutions) or n_power_iterations != 1 are not touched at all.

The weights are refreshed once per forward OF `net`.  A layer that `net` calls twice within one forward therefore gets
one power iteration where torch's per-layer hook does two; none of the reference's discriminators does that.  A fused
layer called on its own, outside `net`, runs torch's hook.

The forward reads nothing back from the device and takes its blocks from torch's allocator, so a forward may be
captured into a HIP graph once the table is built (one eager forward first).  The backward uploads the addresses of the
incoming gradients when they differ from the previous call's: it is not meant for capture.

As in ssl_amd/ema.py, EVERY call compares data_ptr(), shape and dtype of every weight_orig, u and v with the cached ones
and rebuilds the table on a difference, and the cache keeps the storages alive.
"""
import numpy as np
import torch
from torch.nn.utils.spectral_norm import SpectralNorm

from . import _gpu, _lib
from ._gpu import address_array

__all__ = ["fuse_spectral_norm", "FusedSpectralNorm"]

EPS = 1e-12
_RECORD, _HEADER = 8, 8                     # words of a layer's record / of the header in the table image


# ---- the seam between this module and the library (tests count and replace it) ----
def _library():
    return _lib.lib()


class _QuietSpectralNorm(SpectralNorm):
    """torch's hook object with a switch in front: while the set's own hook has refreshed this layer's weight for the
    running forward of the net, the layer's hook does nothing.  The object keeps its identity (fuse changes its class, not
    the hook table), so the state_dict hooks that refer to it and remove_spectral_norm work as before."""

    def __call__(self, module, inputs):
        if getattr(self, "_fused_done", False):
            return
        SpectralNorm.__call__(self, module, inputs)


class Plan:
    """The table of one group of native layers (one GPU, one training flag) and what a call needs besides: block sizes,
    the layers' places in the blocks, the device array of gradient addresses."""

    def __init__(self, tensors, device):
        """tensors: [(W, u, v)], detached aliases that keep the storages alive."""
        L = _library()
        self.device, self.keep = device, tensors
        self.shapes = [W.shape for W, _, _ in tensors]
        self.rows = [W.shape[0] for W, _, _ in tensors]
        self.cols = [W.numel() // W.shape[0] for W, _, _ in tensors]
        n = self.n = len(tensors)
        r, c = address_array(self.rows), address_array(self.cols)
        sizes = [f(n, r.ctypes.data, c.ctypes.data) for f in (L.ssg_sn_table_bytes, L.ssg_sn_output_bytes,
                                                              L.ssg_sn_workspace_bytes, L.ssg_sn_saved_bytes)]
        if 0 in sizes:
            _lib.check(_lib.CONSTANTS["SSG_E_TOOLARGE"])
        table_bytes, self.out_bytes, self.ws_bytes, self.saved_bytes = sizes
        w, u, v = (address_array([t[k].data_ptr() for t in tensors]) for k in range(3))
        self.image = np.zeros(table_bytes // 8, dtype=np.uint64)
        _lib.check(L.ssg_sn_table_fill(n, w.ctypes.data, u.ctypes.data, v.ctypes.data, r.ctypes.data, c.ctypes.data,
                                       self.image.ctypes.data, table_bytes))
        records = self.image[_HEADER:_HEADER + _RECORD * n].reshape(n, _RECORD)
        self.out_off = [int(x) for x in records[:, 5]]
        self.saved_off = [int(x) for x in records[:, 7]]
        pin = device.type == "cuda" and torch.cuda.is_available()
        host = torch.from_numpy(self.image.view(np.int64))
        host = host.pin_memory() if pin else host
        with _gpu.on(device):
            self.table = torch.empty(len(self.image), dtype=torch.int64, device=device).copy_(host, non_blocking=True)
            self.grad_addresses = torch.zeros(n, dtype=torch.int64, device=device)
            if device.type == "cuda":
                torch.cuda.current_stream().synchronize()
        self._uploaded = [0] * n

    def views(self, block):
        return [block[o:o + r * c].view(s) for o, r, c, s in zip(self.out_off, self.rows, self.cols, self.shapes)]

    def forward(self, training, out=None):
        """(the layers' W_sn, views of one block; the call's saved block).  out: the block to write, of out_bytes (a
        new one where None)."""
        dev = self.device
        with _gpu.on(dev):
            if out is None:
                out = torch.empty(self.out_bytes // 4, dtype=torch.float32, device=dev)
            saved = torch.empty(max(self.saved_bytes // 4, 1), dtype=torch.float32, device=dev)
            ws, _ = _gpu.workspace(self.ws_bytes, dev)
        _gpu.launch(dev, _library().ssg_sn_forward, self.table.data_ptr(), self.image.ctypes.data, int(bool(training)),
                    out.data_ptr(), self.out_bytes, ws.data_ptr(), self.ws_bytes, saved.data_ptr(), self.saved_bytes)
        return self.views(out), saved

    def backward(self, saved, grads, block=None):
        """The gradients with respect to the weight_origs for `grads` (a None: no gradient for that layer), views of one
        block laid out as the output block (`block`, or a new one)."""
        dev = self.device
        grads = [None if g is None else g.contiguous() for g in grads]
        addresses = [0 if g is None else g.data_ptr() for g in grads]
        with _gpu.on(dev):
            if addresses != self._uploaded:
                host = torch.tensor(addresses, dtype=torch.int64).pin_memory()
                self.grad_addresses.copy_(host, non_blocking=True)
                self._uploaded = addresses
            if block is None:
                block = torch.empty(self.out_bytes // 4, dtype=torch.float32, device=dev)
            ws, _ = _gpu.workspace(self.ws_bytes, dev)
        _gpu.launch(dev, _library().ssg_sn_backward, self.table.data_ptr(), self.image.ctypes.data,
                    self.grad_addresses.data_ptr(), saved.data_ptr(), self.saved_bytes, block.data_ptr(), self.out_bytes,
                    ws.data_ptr(), self.ws_bytes)
        return [None if g is None else d for g, d in zip(grads, self.views(block))]


class _SpectralNormFunction(torch.autograd.Function):
    """W_sn of every layer of a plan from the weight_origs, in one call; u and v are constants."""

    @staticmethod
    def forward(ctx, plan, training, *weights):
        outs, saved = plan.forward(training)
        ctx.plan, ctx.block = plan, saved
        ctx.save_for_backward(*weights)          # (for autograd's check that no weight changed in between)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        ctx.saved_tensors                        # raises where a weight_orig was modified in place since the forward
        needs = ctx.needs_input_grad[2:]
        grads = [g if need and g is not None and _gpu.readable(g) else None for g, need in zip(grads, needs)]
        if all(g is None for g in grads):
            return (None, None) + (None,) * len(grads)
        return (None, None) + tuple(ctx.plan.backward(ctx.block, grads))


def _parts(module, fn):
    return getattr(module, fn.name + "_orig"), getattr(module, fn.name + "_u"), getattr(module, fn.name + "_v")


def _native_layer(module, fn):
    W, u, v = _parts(module, fn)
    return (_gpu.native(W, u, v) and fn.eps == EPS and W.dim() >= 1 and W.numel() > 0 and W.is_contiguous()
            and u.is_contiguous() and v.is_contiguous() and u.numel() == W.shape[0]
            and v.numel() * W.shape[0] == W.numel())


class FusedSpectralNorm:
    """The handle fuse_spectral_norm returns: `layers` [(module, hook)], `rebuilds`, `unfuse()`."""

    def __init__(self, net):
        self.net = net
        self.layers = [(m, h) for m in net.modules() for h in m._forward_pre_hooks.values()
                       if isinstance(h, SpectralNorm) and h.dim == 0 and h.n_power_iterations == 1]
        for _, h in self.layers:
            if type(h) is not SpectralNorm:
                raise RuntimeError("fuse_spectral_norm: a layer of this net is fused already")
        for _, h in self.layers:
            h.__class__ = _QuietSpectralNorm
        self._sig, self._plans = None, []
        self.rebuilds = 0
        self._handles = [net.register_forward_pre_hook(lambda net, inputs: self.refresh()),
                         net.register_forward_hook(lambda net, inputs, output: self.release(), always_call=True)]

    def unfuse(self):
        """torch's per-layer hooks again; the buffers keep what the fused forwards left in them."""
        for handle in self._handles:
            handle.remove()
        self._handles = []
        for _, h in self.layers:
            h._fused_done = False
            h.__class__ = SpectralNorm
        self._sig, self._plans = None, []

    def _signature(self):
        sig = [_gpu.native_criteria()]
        for m, h in self.layers:
            sig.append(m.training)
            for t in _parts(m, h):
                sig.append((t.data_ptr(), t.shape, t.stride(), t.dtype, t.device))
        return sig

    def _build(self):
        groups = {}
        for i, (m, h) in enumerate(self.layers):
            if _native_layer(m, h):
                groups.setdefault((_parts(m, h)[0].device, m.training), []).append(i)
        self._plans = [(idx, training, Plan([tuple(t.detach() for t in _parts(*self.layers[i])) for i in idx], device))
                       for (device, training), idx in groups.items()]
        self.rebuilds += 1

    def refresh(self):
        """What a forward of the net does first: every native layer's `weight` from one call per plan; those layers'
        own hooks stay quiet until release()."""
        sig = self._signature()
        if sig != self._sig:
            self._build()
            self._sig = sig
        for _, h in self.layers:
            h._fused_done = False
        for idx, training, plan in self._plans:
            weights = [_parts(*self.layers[i])[0] for i in idx]
            if torch.is_grad_enabled() and any(w.requires_grad for w in weights):
                outs = _SpectralNormFunction.apply(plan, training, *weights)
            else:
                outs, _ = plan.forward(training)
            for i, out in zip(idx, outs):
                m, h = self.layers[i]
                setattr(m, h.name, out)
                h._fused_done = True

    def release(self):
        """What a forward of the net does last: the layers' own hooks wake up (a layer called outside the net runs
        torch's lines)."""
        for _, h in self.layers:
            h._fused_done = False


def fuse_spectral_norm(net):
    """Fuse the spectral normalisation of every layer of `net` that carries torch's SpectralNorm hook with dim == 0 and
    n_power_iterations == 1 (see the module's text); returns the handle, whose unfuse() undoes it."""
    return FusedSpectralNorm(net)
