"""The exponential moving average of a model's weights behind the reference's three call sites, on the one-launch
multi-tensor kernel of ssl_amd/csrc/ssg_multi.hip (include/ssg_hip.h section (S)).

    ModelEma / model_ema   GAN-Based-SR/basicsr/models/base_model.py:75-82
                           ema[k].data.mul_(decay).add_(net[k].data, alpha=1 - decay) over the EMA network's names
    update_E               GAN-Based-SR/train_BSGRAN/models/model_base.py:192-197: the same over the generator's names
    LitEma                 Diffusion-Based-SR/ldm/modules/ema.py: shadow.sub_(one_minus_decay * (shadow - param)) with the
                           warm-up decay = min(decay, (1 + n) / (10 + n)), and copy_to / store / restore

Each is a Python loop of two or three device operations per parameter in the reference; here the whole set is one launch.
A device-resident table lists (dst, src, n) per tensor; the host builds and uploads it once per parameter set (one copy
from pinned memory) and a steady-state call only launches.

The native domain: a pair is native when both tensors are fp32, on one GPU, of the same shape and strides, dense and
non-overlapping (contiguous and channels_last weights both qualify: the update walks the storage).  Any other pair --
CPU, fp16 / bf16 / fp64, different strides -- takes the reference's torch expression for that pair and gives its bits,
and `ssl_amd.losses.set_native_criteria(False)` routes every pair that way.  A set in which the memory of two different
pairs overlaps goes that way as a whole.

Stale tables are the one way this could write where it should not, so the cache keeps a reference to the storage of every
tensor in a table (none can be freed and handed out again), and EVERY call compares the current data_ptr(), shape,
strides and dtype of every tensor with the cached ones and rebuilds the table on a difference (`p.data = ...`, `.to()`,
`load_state_dict` into new storage).  That check is host time proportional to the number of tensors
(tools/ema_time.py reports it); it is the price of safety and cannot be switched off.

Parameters only, not buffers, as in the reference.  The Parameter OBJECTS of ModelEma are those of its construction, and
LitEma's trainable set is that of its construction.
"""
import operator
import weakref

import torch
from torch import nn
from torch.nn.parallel import DataParallel, DistributedDataParallel

from . import _gpu, _lib
from ._gpu import address_array
from ._gpu import dense_strides as _dense

__all__ = ["ModelEma", "model_ema", "update_E", "LitEma", "get_bare_model"]

EMA, LIT, COPY = (_lib.CONSTANTS["SSG_MT_" + k] for k in ("EMA", "LIT", "COPY"))
_PTR, _SIZE, _STRIDE, _DTYPE = torch.Tensor.data_ptr, torch.Tensor.size, torch.Tensor.stride, operator.attrgetter("dtype")


def get_bare_model(net):
    """The module inside DistributedDataParallel / DataParallel (base_model.py's get_bare_model)."""
    return net.module if isinstance(net, (DataParallel, DistributedDataParallel)) else net


# ---- the seams between this module and the library / the device (tests count and replace them) ----
def _library():
    return _lib.lib()


def _on_gpu(t):
    return t.is_cuda


def _upload(host, device):
    """The table image on `device`, copied from the pinned `host` tensor on the current stream and waited for (at build
    time only: a later call may run on any stream)."""
    with _gpu.on(device):
        table = torch.empty(host.numel(), dtype=torch.uint8, device=device).copy_(host, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return table


def _host_buffer(nbytes, device):
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=device.type == "cuda" and torch.cuda.is_available())


def _native_pair(e, p):
    if not (_on_gpu(e) and _on_gpu(p) and e.device == p.device and e.dtype == torch.float32 and p.dtype == torch.float32
            and e.shape == p.shape and e.stride() == p.stride() and _dense(e)):
        return False
    a, b, nbytes = e.data_ptr(), p.data_ptr(), 4 * e.numel()
    return a == b or a + nbytes <= b or b + nbytes <= a


def _pairs_overlap(pairs):
    """Whether the memory of two DIFFERENT pairs overlaps (a sweep over the sorted ranges with the two furthest ends of
    distinct pairs)."""
    spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel(), i) for i, pair in enumerate(pairs) for t in pair
                   if t.numel())
    (end1, who1), (end2, who2) = (-1, -1), (-1, -2)
    for start, end, who in spans:
        if (start < end1 and who != who1) or (start < end2 and who != who2):
            return True
        if who == who1:
            end1 = max(end1, end)
        elif end > end1:
            (end2, who2), (end1, who1) = (end1, who1), (end, who)
        elif who == who2:
            end2 = max(end2, end)
        elif end > end2:
            end2, who2 = end, who
    return False


def build_table(dst_ptrs, src_ptrs, counts, device):
    """(the table on `device`, its chunk count, the host image) for host lists of addresses and element counts."""
    L = _library()
    d, s, c = (address_array(v) for v in (dst_ptrs, src_ptrs, counts))
    n = len(c)
    nbytes = L.ssg_multi_table_bytes(n, c.ctypes.data)
    if nbytes == 0:
        _lib.check(_lib.CONSTANTS["SSG_E_TOOLARGE"])
    host = _host_buffer(nbytes, device)
    _lib.check(L.ssg_multi_table_fill(n, d.ctypes.data, s.ctypes.data, c.ctypes.data, host.data_ptr(), nbytes))
    return _upload(host, device), L.ssg_multi_chunks(n, c.ctypes.data), host


def _torch_update(kind, e, p, decay, w):
    """The reference's expression for one pair (the fallback, and what the kernel restates)."""
    if kind == EMA:
        e.mul_(decay).add_(p, alpha=1 - decay)
    elif kind == LIT:
        e.sub_(w * (e - p))
    else:
        e.copy_(p)


class _Updater:
    """One update form over a list of (dst, src) pairs: the cached tables of the native pairs, one per GPU, and the
    pairs left to torch.  run() validates the cache against the tensors it is handed, every call."""

    def __init__(self):
        self._sig = self._flag = None
        self._keep, self._tables, self._fallback = [], [], []
        self.rebuilds = 0

    def __deepcopy__(self, memo):
        return _Updater()            # a copy of the module starts without tables: they point into the original's storage

    def __reduce__(self):
        return _Updater, ()          # (pickled the same way: addresses mean nothing in another process)

    @staticmethod
    def signature(tensors):
        """What a table depends on, of every tensor: address, shape, strides, dtype (four C-level calls per tensor, mapped:
        this runs every call and is most of a call's host time)."""
        return (list(map(_PTR, tensors)), list(map(_SIZE, tensors)), list(map(_STRIDE, tensors)), list(map(_DTYPE, tensors)))

    def _build(self, dst, src):
        # detached aliases: they share (and keep alive) the storage the table points into, whatever happens to p.data
        keep = [(e.detach(), p.detach()) for e, p in zip(dst, src)]
        native = [i for i, (e, p) in enumerate(keep) if self._flag and _native_pair(e, p)]
        if _pairs_overlap([keep[i] for i in native]):
            native = []
        groups = {}
        for i in native:
            groups.setdefault(keep[i][0].device, []).append(i)
        self._tables = []
        for device, idx in groups.items():
            table, n_chunks, host = build_table([keep[i][0].data_ptr() for i in idx], [keep[i][1].data_ptr() for i in idx],
                                                [keep[i][0].numel() for i in idx], device)
            self._tables.append((device, table, n_chunks, host))
        taken = set(native)
        self._fallback = [pair for i, pair in enumerate(keep) if i not in taken]
        self._keep = keep
        self.rebuilds += 1

    def run(self, dst, src, kind, decay=0.0, w=None):
        sig = self.signature(dst + src)
        if sig != self._sig or self._flag != _gpu.native_criteria():
            self._flag = _gpu.native_criteria()
            self._build(dst, src)
            self._sig = sig
        if self._tables:
            L = _library()
            d, a = (float(decay), 1 - float(decay)) if kind == EMA else (0.0, 0.0)
            for device, table, n_chunks, _ in self._tables:
                wd = None if w is None else (w if w.device == device else w.to(device))
                _gpu.launch(device, L.ssg_multi_apply, table.data_ptr(), n_chunks, kind, d, a, _gpu.ptr(wd))
        if self._fallback:
            with torch.no_grad():
                for e, p in self._fallback:
                    _torch_update(kind, e, p, decay, w)


class ModelEma:
    """ModelEma(net, net_ema): net_ema's parameters follow net's.

    update(decay=0.999) is base_model.py's model_ema loop, copy() sets net_ema's parameters to net's (model_ema(0) without
    its arithmetic).  Both networks are unwrapped from DistributedDataParallel / DataParallel; parameters are paired by
    name as the reference's dict(named_parameters()) lookups pair them, over net_ema's names (names='ema', model_ema) or
    over net's (names='net', update_E); a name the other network lacks raises KeyError."""

    def __init__(self, net, net_ema, names="ema"):
        src, dst = dict(get_bare_model(net).named_parameters()), dict(get_bare_model(net_ema).named_parameters())
        keys = list(dst if names == "ema" else src)
        self.names = keys
        self.dst, self.src = [dst[k] for k in keys], [src[k] for k in keys]
        self._ema, self._copy = _Updater(), _Updater()

    def update(self, decay=0.999):
        self._ema.run(self.dst, self.src, EMA, decay)

    def copy(self):
        self._copy.run(self.dst, self.src, COPY)


_CACHE = weakref.WeakKeyDictionary()      # net_ema -> {net (weakly) -> {names: ModelEma}}


def _cached(net, net_ema, names):
    per_net = _CACHE.setdefault(net_ema, weakref.WeakKeyDictionary())
    forms = per_net.setdefault(net, {})
    if names not in forms:
        forms[names] = ModelEma(net, net_ema, names)
    return forms[names]


def model_ema(net_g, net_g_ema, decay=0.999):
    """base_model.py:75-82 with the two networks as arguments: `model_ema(self.net_g, self.net_g_ema, decay)`."""
    _cached(net_g, net_g_ema, "ema").update(decay)


def update_E(netG, netE, decay=0.999):
    """model_base.py:192-197 with the two networks as arguments: `update_E(self.netG, self.netE, decay)`."""
    _cached(netG, netE, "net").update(decay)


class LitEma(nn.Module):
    """ldm/modules/ema.py's LitEma: the same constructor (its spelling `use_num_upates` included), the same buffers
    (`decay`, `num_updates`, one per trainable parameter under its name with the dots removed), so a state_dict of either
    class loads into the other, and the same forward(model), copy_to(model), store(parameters), restore(parameters).

    forward keeps the warm-up on the device: num_updates is incremented, min(decay, (1 + n) / (10 + n)) and 1 - decay are
    a handful of 0-d operations (torch.minimum where the reference's Python min reads the device), and the weight
    reaches the kernel as a device float with the reference's bits.  Whether the counter counts (num_updates >= 0) is
    known on the host: it is fixed by the constructor and read again once after load_state_dict."""

    def __init__(self, model, decay=0.9999, use_num_upates=True):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError('Decay must be between 0 and 1')
        self.m_name2s_name = {}
        self.register_buffer('decay', torch.tensor(decay, dtype=torch.float32))
        self.register_buffer('num_updates', torch.tensor(0 if use_num_upates else -1, dtype=torch.int))
        for name, p in model.named_parameters():
            if p.requires_grad:
                s_name = name.replace('.', '')          # a buffer's name may not hold a '.'
                self.m_name2s_name[name] = s_name
                self.register_buffer(s_name, p.clone().detach().data)
        self.collected_params = []
        self._counting = bool(use_num_upates)
        self._forward, self._copy_to, self._store, self._restore = _Updater(), _Updater(), _Updater(), _Updater()

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._counting = bool(self.num_updates >= 0)

    def _pairs(self, model):
        """(shadows, parameters) of the model's trainable parameters, in its order (a trainable parameter that had no
        shadow at construction raises KeyError, as the reference's lookup does)."""
        shadows, params = [], []
        for name, p in model.named_parameters():
            if p.requires_grad:
                shadows.append(self._buffers[self.m_name2s_name[name]])
                params.append(p)
        return shadows, params

    def forward(self, model):
        decay = self.decay
        with torch.no_grad():
            if self._counting:
                self.num_updates += 1
                decay = torch.minimum(self.decay, (1 + self.num_updates) / (10 + self.num_updates))
            one_minus_decay = 1.0 - decay
            shadows, params = self._pairs(model)
            self._forward.run(shadows, params, LIT, w=one_minus_decay)

    def copy_to(self, model):
        shadows, params = self._pairs(model)
        self._copy_to.run(params, shadows, COPY)

    def store(self, parameters):
        """Save the current parameters for restoring later (copies of them, in self.collected_params)."""
        params = list(parameters)
        held = self.collected_params
        if len(held) != len(params) or any(h.shape != p.shape or h.stride() != p.stride() or h.dtype != p.dtype
                                           or h.device != p.device for h, p in zip(held, params)):
            held = [torch.empty_like(p, requires_grad=False) for p in params]
        self._store.run(held, params, COPY)
        self.collected_params = held

    def restore(self, parameters):
        """Restore the parameters saved with `store` (validate with the EMA weights between the two)."""
        params = list(parameters)[:len(self.collected_params)]
        self._restore.run(params, self.collected_params[:len(params)], COPY)
