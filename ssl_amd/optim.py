"""torch.optim.Adam and AdamW with the step of a parameter group as ONE launch of ssl_amd/csrc/ssg_multi.hip's Adam kernel
(include/ssg_hip.h section (X)), behind torch's own classes:

    get_optimizer          GAN-Based-SR/basicsr/models/base_model.py:103-120 (all eight options/train/*SSL/*.yml: type Adam,
                           weight_decay 0, betas [0.9, 0.99])
    Adam                   train_BSGRAN/models/model_ssl.py:229-230: Adam(..., weight_decay=0) for G and D
    AdamW                  the Diffusion fork's configure_optimizers

With torch's defaults the step is a chain of _foreach_ passes over the whole set, each split into several launches; here a
group is one launch.  Adam and AdamW subclass torch's and override step() ONLY: param_groups, state[p] with `step` /
`exp_avg` / `exp_avg_sq`, state_dict, load_state_dict, add_param_group, the hooks and every lr scheduler are torch's, and
a checkpoint written by either class loads into the other (the reference's save_training_state / resume_training).

The kernel computes torch's single-tensor Adam operation by operation in fp32, each rounded on its own.  That is NOT
torch's bits: torch's lerp_ and fused multiply-adds round differently in a share of the elements, by one rounding of the
operands; tests/adam_reference.py holds both to an fp64 evaluation within a derived bound.

The native domain, per parameter group: the package's rule (_gpu.native: the switch of set_native_criteria, fp32 tensors
on one GPU) for the parameter, its dense gradient, exp_avg and exp_avg_sq, all four of equal shape and strides and dense
(contiguous or channels_last: the step walks the storage), no two of them overlapping; amsgrad, maximize, capturable,
differentiable and fused all off; lr, betas, eps and weight_decay Python numbers; `step` counters on the host (where
torch keeps them without capturable / fused).  A group outside it goes through torch's own functional adam(), as
torch.optim.Adam.step would send it, and so gives torch's bits.  Parameters of a group whose `step` disagree (a group
extended by add_param_group after some steps shares one) are split by step value: one launch per value.

The bias corrections are host scalars of step t in the launch's arguments, exactly as in torch's non-capturable Adam: a
captured graph would replay step t's scalars.  DO NOT capture step() into a HIP graph.

Stale tables are the one way this could write where it should not, so, as ssl_amd.ema does, the cache keeps the storage
of every tensor of a table alive, and EVERY call compares data_ptr(), shape, strides and dtype of every tensor with the
cached ones.  A moved parameter or state rebuilds the table; gradients move between steps under
zero_grad(set_to_none=True), so their addresses live in an array of their own, and a moved gradient costs one small
upload on the current stream (no synchronisation), not a rebuild.
"""
import ctypes

import torch
from torch.optim.adam import adam as _torch_adam
from torch.optim.optimizer import _use_grad_for_differentiable

from . import _gpu, _lib
from ._gpu import address_array
from ._gpu import dense_strides as _dense
from .ema import _DTYPE, _PTR, _SIZE, _STRIDE, _host_buffer

__all__ = ["Adam", "AdamW", "get_optimizer"]

PLAIN, L2, DECOUPLED = (_lib.CONSTANTS["SSG_ADAM_" + k] for k in ("PLAIN", "L2", "DECOUPLED"))
_WORD = 8


class Scalars(ctypes.Structure):
    """include/ssg_hip.h: ssg_adam_scalars (a double assigned to a field is cast to float once, as the contract says)."""
    _fields_ = [(k, ctypes.c_float) for k in ("a", "w1", "b2", "w2", "s2", "eps", "wd", "cwd")] + [("mode", ctypes.c_int)]


def scalars(lr, beta1, beta2, eps, weight_decay, decoupled, step):
    """The launch's scalars for step t, formed in Python doubles by torch's own expressions (_single_tensor_adam)."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    mode = PLAIN if weight_decay == 0 else (DECOUPLED if decoupled else L2)
    return Scalars(step_size, 1 - beta1, beta2, 1 - beta2, bias_correction2_sqrt, eps,
                   weight_decay if mode == L2 else 0.0, 1 - lr * weight_decay if mode == DECOUPLED else 1.0, mode)


# ---- the seams between this module and the library / the device (tests count and replace them) ----
def _library():
    return _lib.lib()


def _on_gpu(t):
    return t.is_cuda


def _upload(host, device):
    """A new device image of the pinned `host` tensor, copied on the current stream and waited for (at build time only)."""
    with _gpu.on(device):
        image = torch.empty(host.numel(), dtype=torch.uint8, device=device).copy_(host, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return image


def _refresh(host, image, device):
    """`image` overwritten from the pinned `host` tensor on the current stream, in front of the launch that reads it and
    behind the one that read it last; no wait (torch's host allocator keeps `host` until the copy has run)."""
    with _gpu.on(device):
        image.copy_(host, non_blocking=True)


def _native_quad(p, g, m, v):
    if not (_on_gpu(p) and g.layout == torch.strided and _dense(p)):
        return False
    for t in (p, g, m, v):
        if not (_on_gpu(t) and t.device == p.device and t.dtype == torch.float32 and t.shape == p.shape
                and t.stride() == p.stride()):
            return False
    return True


def build_tables(p_ptrs, g_ptrs, m_ptrs, v_ptrs, counts, device):
    """(the table on `device`, the gradient addresses on `device`, the chunk count, the table's host image) for host
    lists of addresses and element counts; None where two of the tensors overlap."""
    L, n = _library(), len(counts)
    p, g, m, v, c = (address_array(x) for x in (p_ptrs, g_ptrs, m_ptrs, v_ptrs, counts))
    nbytes = L.ssg_adam_table_bytes(n, c.ctypes.data)
    if nbytes == 0:
        _lib.check(_lib.CONSTANTS["SSG_E_TOOLARGE"])
    host, ghost = _host_buffer(nbytes, device), _host_buffer(_WORD * max(n, 1), device)
    rc = L.ssg_adam_table_fill(n, p.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, c.ctypes.data,
                               host.data_ptr(), nbytes, ghost.data_ptr(), _WORD * n)
    if rc == _lib.CONSTANTS["SSG_E_BADARG"]:
        return None                          # (the arrays and the addresses of live tensors are not null: an overlap)
    _lib.check(rc)
    return _upload(host, device), _upload(ghost, device), L.ssg_multi_chunks(n, c.ctypes.data), host


class _Plan:
    """The cached table of one set of (p, g, m, v), or the decision that the set is torch's.  validate() compares the
    cache with the tensors it is handed, every call.  (The switch of set_native_criteria is `_eligible`'s: with it off no
    plan is asked, and a table stays valid for as long as its tensors do.)"""

    def __init__(self):
        self._sig = self._gsig = self._gptr = None
        self.native = False
        self.keep, self.table, self.grads, self.host, self.n_chunks, self.device = [], None, None, None, 0, None
        self.rebuilds = self.grad_uploads = 0

    def _build(self, params, grads, ms, vs):
        # detached aliases: they share (and keep alive) the storage the table points into
        keep = [[t.detach() for t in ts] for ts in (params, grads, ms, vs)]
        self.keep, self.table, self.grads, self.host = keep, None, None, None
        self.rebuilds += 1
        self.native = all(_native_quad(*q) for q in zip(*keep))
        if not self.native:
            return
        built = build_tables(*([t.data_ptr() for t in ts] for ts in keep), [t.numel() for t in keep[0]], keep[0][0].device)
        if built is None:
            self.native = False              # two of the tensors overlap: the set is torch's
            return
        self.table, self.grads, self.n_chunks, self.host = built
        self.device = keep[0][0].device

    def _move_grads(self, grads):
        """The new gradient addresses into the device's array; False where the library refuses them."""
        n = len(grads)
        g = address_array([t.data_ptr() for t in grads])
        ghost = _host_buffer(_WORD * n, self.device)
        if _library().ssg_adam_grads_fill(self.host.data_ptr(), n, g.ctypes.data, ghost.data_ptr(), _WORD * n) != 0:
            return False
        _refresh(ghost, self.grads, self.device)
        self.keep[1] = [t.detach() for t in grads]
        self.grad_uploads += 1
        return True

    def validate(self, params, grads, ms, vs):
        """Whether the set takes the kernel, with the tables made current for these tensors."""
        flat = params + ms + vs
        sig = (list(map(_PTR, flat)), list(map(_SIZE, flat)), list(map(_STRIDE, flat)), list(map(_DTYPE, flat)))
        gptr, gsig = list(map(_PTR, grads)), (list(map(_STRIDE, grads)), list(map(_DTYPE, grads)))
        if sig != self._sig or gsig != self._gsig:
            self._build(params, grads, ms, vs)
            self._sig, self._gsig, self._gptr = sig, gsig, gptr
        elif gptr != self._gptr:
            if not self.native:
                self.keep[1] = [t.detach() for t in grads]
            elif not self._move_grads(grads):
                self._build(params, grads, ms, vs)
            self._gptr = gptr
        return self.native


_IS_CUDA = torch.Tensor.is_cuda.__get__


def _number(x):
    return type(x) in (float, int)


def _eligible(group, steps, has_complex):
    """The conditions on a group that cost nothing per tensor but the device of its counters."""
    return (_gpu.native_criteria() and not (group["amsgrad"] or group["maximize"] or group["capturable"]
                                            or group["differentiable"] or group["fused"] or has_complex)
            and _number(group["lr"]) and _number(group["eps"]) and _number(group["weight_decay"])
            and all(map(_number, group["betas"])) and not any(map(_IS_CUDA, steps)))


class Adam(torch.optim.Adam):
    """torch.optim.Adam with its constructor; step() takes the kernel for every group of the native domain (module
    docstring) and torch's functional adam() for every other."""

    def _plan(self, key):
        plans = self.__dict__.setdefault("_plans", {})       # (torch pickles defaults, state and param_groups only)
        if key not in plans:
            plans[key] = _Plan()
        return plans[key]

    def _torch_step(self, group, lists, has_complex):
        params, grads, ms, vs, max_vs, steps = lists
        beta1, beta2 = group["betas"]
        _torch_adam(params, grads, ms, vs, max_vs, steps, amsgrad=group["amsgrad"], has_complex=has_complex, beta1=beta1,
                    beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"],
                    maximize=group["maximize"], foreach=group["foreach"], capturable=group["capturable"],
                    differentiable=group["differentiable"], fused=group["fused"],
                    grad_scale=getattr(self, "grad_scale", None), found_inf=getattr(self, "found_inf", None),
                    decoupled_weight_decay=group["decoupled_weight_decay"])

    @_use_grad_for_differentiable
    def step(self, closure=None):
        self._cuda_graph_capture_health_check()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            lists = ([], [], [], [], [], [])
            has_complex = self._init_group(group, *lists)         # torch's: the tensors with a gradient, states made
            params, grads, ms, vs, _, steps = lists
            if not params:
                continue
            if not _eligible(group, steps, has_complex):
                self._torch_step(group, lists, has_complex)
                continue
            lo, hi = torch.aminmax(torch.stack(steps))
            if lo.item() == hi.item():
                subsets = [lists]
            else:                                                 # one launch per step value
                by_value = {}
                for i, t in enumerate(torch.stack(steps).tolist()):
                    by_value.setdefault(t, []).append(i)
                subsets = [tuple([ts[i] for i in idx] for ts in (params, grads, ms, vs)) + ([], [steps[i] for i in idx])
                           for idx in by_value.values()]
            for k, sub in enumerate(subsets):
                plan = self._plan((gi, k))
                if not plan.validate(sub[0], sub[1], sub[2], sub[3]):
                    self._torch_step(group, sub, has_complex)
                    continue
                # torch's `step_t += 1`, all of them in one call (a tensor 1 as in torch's own foreach form: a Python
                # number is wrapped once per counter, four times the host time at 702 of them)
                torch._foreach_add_(sub[5], torch.tensor(1.0, device="cpu"), alpha=1.0)
                beta1, beta2 = group["betas"]
                s = scalars(group["lr"], beta1, beta2, group["eps"], group["weight_decay"],
                            group["decoupled_weight_decay"], sub[5][0].item())
                _gpu.launch(plan.device, _library().ssg_adam_apply, plan.table.data_ptr(), plan.grads.data_ptr(),
                            plan.n_chunks, ctypes.addressof(s))
        return loss


class AdamW(torch.optim.AdamW, Adam):
    """torch.optim.AdamW with its constructor (torch's AdamW is its Adam with decoupled_weight_decay=True) and Adam's
    step() above."""
    step = Adam.step


def get_optimizer(optim_type, params, lr, **kwargs):
    """base_model.py:103-120 as a function: `self.get_optimizer = ssl_amd.optim.get_optimizer` keeps its callers."""
    if optim_type == 'Adam':
        return Adam(params, lr, **kwargs)
    if optim_type == 'AdamW':
        return AdamW(params, lr, **kwargs)
    if optim_type in ('Adamax', 'SGD', 'ASGD', 'RMSprop', 'Rprop'):
        return getattr(torch.optim, optim_type)(params, lr, **kwargs)
    raise NotImplementedError(f'optimizer {optim_type} is not supported yet.')
