"""Torch-facing front end of the gfx950 SSG engine.

PyTorch is used for device memory, streams and autograd plumbing only; every
number is produced by the hand-written HIP kernels in ssl_amd/csrc through the
C ABI of include/ssg_hip.h.  Tensors must live on the GPU; there is no CPU
path (a CPU tensor raises, like the reference operator refuses non-CUDA
tensors, similaritywrapper.py:60-62 -- but with an exception instead of
sys.exit()).
"""
import torch

from . import _lib
# the launch helpers under the names this module (and its tests and tools) has always used for them
from ._gpu import address_array, dense_strides, launch as _launch, need_gpu as _need_gpu, ptr as _ptr  # noqa: F401
from ._gpu import readable as _readable, stream as _stream, workspace as _workspace  # noqa: F401


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _mask_kind(mask, image_channels):
    """(mask as the C ABI reads it, kind): uint8 / bool -> kind 1 (edge pixel <=> value 1 (True), like `mask == 1`),
    float -> kind 0, None -> kind 2, the Laplacian mask of the call's GT, which must have 3 channels."""
    if mask is None:
        if image_channels != 3:
            raise ValueError("Laplacian edge mask needs a 3-channel image")
        return None, 2
    if mask.dtype == torch.uint8 or mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8), 1
    return _f32c(mask), 0


def _reduction_is_mean(name, reduction):
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"ssl_amd: {name} fuses the 'mean' and 'sum' reductions only, got {reduction!r}")
    return reduction == 'mean'


def deterministic_default():
    """The Python host asks for the bit-reproducible gradient accumulation (include/ssg_hip.h, ssg_grad_fix_bytes)
    unless SSG_DETERMINISTIC=0 is set: measured +3 % on the benchmark step (1.64 vs 1.59 ms), for gradients that
    are equal bit for bit from run to run.  Every entry point also takes `deterministic=` explicitly."""
    import os
    return os.environ.get("SSG_DETERMINISTIC", "1") not in ("", "0")


def _grad_fix(det, x):
    """Fixed-point accumulation buffer of the deterministic mode for an image batch x, or None."""
    if det is None:
        det = deterministic_default()
    if not det:
        return None
    B, C, H, W = x.shape
    return torch.empty(_lib.lib().ssg_grad_fix_bytes(B, C, H, W), dtype=torch.uint8, device=x.device)


class FwdPlan(tuple):
    """(order, rank map, plan) as the forward / backward entry points take them, plus `.ks`: the search size the plan's
    dense tiles were cut for (8-row tiles for k_s <= 25, 4-row tiles for k_s = 49).  A plan built for one tile
    height must not be walked by the kernels of the other (they would decode tile ids with their own geometry):
    `check_plan` raises before anything is launched."""

    def __new__(cls, order, rank, plan, ks):
        self = super().__new__(cls, (order, rank, plan))
        self.ks = int(ks)
        return self


def _plan_rows(ks):
    return 4 if int(ks) == 49 else 8   # dense_tile_rows() of ssl_amd/csrc/ssg_dense.hip


def check_plan(fwd, ks):
    """ValueError when `fwd` (EdgeList.fwd) was built by edge_list(ks=...) for another dense-tile height than the
    kernels of this call's k_s use."""
    built = getattr(fwd, "ks", None)
    if fwd is not None and built is not None and _plan_rows(built) != _plan_rows(ks):
        raise ValueError(f"ssl_amd: this edge list's dense/direct plan was built for k_s = {built} "
                         f"({_plan_rows(built)}-row tiles) but the call uses k_s = {ks} ({_plan_rows(ks)}-row tiles); "
                         f"build it with edge_list(..., ks={ks})")


class EdgeList(tuple):
    """(edges, counts) -- unpacks like the pair it always was -- plus `.rank`, the (B,H,W) int32
    rank map (row of `edges` holding each pixel, -1 elsewhere), and `.order`, the tile-major
    permutation of the rows that the backward kernels use as their job order, and `.plan`, the
    forward's work split between the dense-tile kernel and the direct kernels.  `.fwd` bundles
    what the forward entry points take."""

    def __new__(cls, edges, counts, rank, order, plan, ks=25):
        self = super().__new__(cls, (edges, counts))
        self.edges, self.counts, self.rank, self.order, self.plan = edges, counts, rank, order, plan
        self.ks = int(ks)
        self.fwd = FwdPlan(order, rank, plan, ks) if plan is not None else None
        return self


def edge_list(mask=None, gt=None, mask_stride=0, lap_threshold=20.0, capacity=None, ks=25, order=True, plan=True):
    """Device-side edge list of a batch.

    mask: (B,c1,H,W) float32 or uint8 (channel 0 is used) -- or None with
    gt (B,3,H,W) float32 in [0,1] to generate the reference's Laplacian mask
    on the fly.  Returns (edges (capacity,3) int32 [b,y,x], counts (B+2) int32
    on device: counts[0] = N).  No host synchronisation.  `ks` is the search size the dense/direct
    work split (`.plan`) is built for: pass the k_s the list will be used with.  order=False leaves the
    separate tile-major order out (`.order` None, three launches less) for callers whose kernels all take
    their job order from the plan (sizes with shared-term kernels: (25,9,3), (49,13,3)).  plan=False leaves the
    dense/direct plan out instead (`.plan` None, `.fwd` None: direct kernels in tile order; four launches less).
    """
    L = _lib.lib()
    if mask is not None:
        _need_gpu(mask)
        src, kind = _mask_kind(mask, None)
        B, c1, H, W = src.shape
    else:
        _need_gpu(gt)
        src = _f32c(gt)
        B, c1, H, W = src.shape
        kind = _mask_kind(None, c1)[1]
    if capacity is None:
        capacity = B * H * W
    dev = src.device
    edges = torch.empty((max(capacity, 1), 3), dtype=torch.int32, device=dev)
    counts = torch.empty(B + 2, dtype=torch.int32, device=dev)
    rank = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    order = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev) if order else None
    plan = torch.empty(L.ssg_forward_plan_bytes(B, H, W, capacity) // 4, dtype=torch.int32, device=dev) if plan else None
    scratch = torch.empty(L.ssg_edge_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    _launch(dev, L.ssg_edge_list, _ptr(src), kind, c1, B, H, W, int(mask_stride or 0), float(lap_threshold), int(ks),
            _ptr(edges), capacity, _ptr(counts), _ptr(rank), _ptr(order), _ptr(plan), _ptr(scratch))
    return EdgeList(edges, counts, rank, order, plan, ks)


def set_overlap(mode):
    """Stream assignment of the dense-tile and the direct kernel of a pass (k_s <= 25): False / 0 = every launch on the
    caller's stream (per-kernel profiling); True / 1 = dense kernel on the caller's stream, direct kernel on the side
    stream (masks with dense tiles: Laplacian edges); 2 = the other way round (masks without dense tiles: Bernoulli /
    thin strided masks, -15 % at 1 % density; +3 % at C2); 3 (default) = 1 or 2 per pass, from the shape of the last
    plan built on the device (include/ssg_hip.h).  Same results.  Returns the previous mode."""
    return _lib.lib().ssg_set_overlap(int(mode))


def set_dense_threshold(edge_pixels_per_tile):
    """Route 8x32-pixel tiles holding at least this many edge pixels through the shared-term ("dense") forward
    kernel (0 = never; default 16).  Same results either way.  Returns the previous value."""
    return _lib.lib().ssg_set_dense_threshold(int(edge_pixels_per_tile))


def set_tiny_step(on):
    """Small (11,5) fused steps (B*H*W <= 16,384 pixels, capacity <= 4,096 rows: BASELINE's C1) in two launches -- one
    workgroup per edge pixel (ssg_tiny.hip); True by default, False keeps every call on the general path.  Same results
    to rounding.  Returns the previous setting."""
    return bool(_lib.lib().ssg_set_tiny_step(int(bool(on))))


def edge_mask_laplacian(gt, lap_threshold=20.0, mask_stride=0):
    """(B,3,H,W) float32 in [0,1] -> (B,H,W) uint8 {0,1}: generate_mask.py:22-31 on device."""
    _need_gpu(gt)
    g = _f32c(gt)
    B, C, H, W = g.shape
    if C != 3:
        raise ValueError("Laplacian edge mask needs a 3-channel image")
    out = torch.empty((B, H, W), dtype=torch.uint8, device=g.device)
    _launch(g.device, _lib.lib().ssg_edge_mask_laplacian, _ptr(g), B, H, W, float(lap_threshold), int(mask_stride or 0),
            _ptr(out))
    return out


class _SSGMapFn(torch.autograd.Function):
    """SSG rows of a batch for a given edge list (loss_util.py:182-244 + autograd)."""

    @staticmethod
    def forward(ctx, img, edges, counts, n_rows, ks, kw, sigma, eps, generalization, order, fwd, det):
        x = _f32c(img)
        ctx.det = det
        f_order, f_rank, f_plan = fwd if fwd is not None else (order, None, None)
        B, C, H, W = x.shape
        ssg = torch.empty((n_rows, ks * ks), dtype=torch.float32, device=x.device)
        _launch(x.device, _lib.lib().ssg_map_forward, _ptr(x), None, B, C, H, W, _ptr(edges), _ptr(f_order), _ptr(f_rank),
                _ptr(f_plan), _ptr(counts), n_rows, ks, kw, float(sigma), float(eps), int(bool(generalization)),
                _ptr(ssg), None, None)
        ctx.save_for_backward(x, edges, counts, ssg)
        ctx.in_dtype = img.dtype
        ctx.order = order
        ctx.split = (f_rank, f_plan)
        ctx.cfg = (n_rows, ks, kw, float(sigma), int(bool(generalization)))
        return ssg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_ssg):
        x, edges, counts, ssg = ctx.saved_tensors
        n_rows, ks, kw, sigma, gen = ctx.cfg
        B, C, H, W = x.shape
        g = _f32c(grad_ssg)
        grad = torch.zeros_like(x)
        L = _lib.lib()
        rank, plan = ctx.split
        scratch = None
        if rank is not None and plan is not None:
            scratch = torch.empty(L.ssg_backward_scratch_bytes(n_rows, ks), dtype=torch.uint8, device=x.device)
        fix = _grad_fix(ctx.det, x)
        _launch(x.device, L.ssg_map_backward, _ptr(x), B, C, H, W, _ptr(edges), _ptr(ctx.order), _ptr(rank), _ptr(plan),
                _ptr(counts), n_rows, ks, kw, sigma, gen, _ptr(ssg), _ptr(g), _ptr(grad), _ptr(scratch), _ptr(fix))
        return grad.to(ctx.in_dtype), None, None, None, None, None, None, None, None, None, None, None


def ssg_map(img, edges, counts, n_rows, ks, kw, sigma, eps=1e-10, generalization=True, order=None, fwd=None,
            deterministic=None):
    """(n_rows, ks*ks) SSG rows of `img` (B,C,H,W) at `edges`; differentiable w.r.t. img.
    `order` (EdgeList.order) is the backward kernel's tile-major job order, `fwd` (EdgeList.fwd)
    the forward's (order, rank map, dense/direct plan)."""
    _need_gpu(img, edges, counts, order)
    check_plan(fwd, ks)
    return _SSGMapFn.apply(img, edges, counts, int(n_rows), int(ks), int(kw), sigma, eps, generalization, order, fwd,
                           deterministic)


class _SSGLossFn(torch.autograd.Function):
    """(l1, kl) of the caller loop realesrganssl_model.py:379-430 over a batch.

    The SSG tensors live only inside forward(): when `sr` needs a gradient, d(l1 + kl)/d sr is produced by the
    SAME launch sequence that produces the two losses (one ssg_loss_backward call) and is the only thing kept
    for backward(), which scales it by the incoming gradient.  That is exact whenever both losses receive the
    same upstream gradient (they are added into one total in every caller of the reference); if autograd hands
    two different tensors, backward() recomputes the step with them (still no host synchronisation)."""

    @staticmethod
    def _run(x, y, edges, counts, n_rows, ks, kw, sigma, eps, gen, w_l1, w_kl, order, fwd, upstream, want_grad,
             det=None):
        L = _lib.lib()
        f_order, f_rank, f_plan = fwd if fwd is not None else (order, None, None)
        B, C, H, W = x.shape
        dev = x.device
        P = ks * ks
        ssg_sr = torch.empty((max(n_rows, 1), P), dtype=torch.float32, device=dev)
        ssg_gt = torch.empty((max(n_rows, 1), P), dtype=torch.float32, device=dev)
        loss = torch.zeros(2, dtype=torch.float32, device=dev)
        grad = torch.zeros_like(x) if want_grad else None
        scratch = torch.empty(L.ssg_loss_scratch_bytes(B, H, W, n_rows, ks), dtype=torch.uint8, device=dev)
        # deferred normalisation (include/ssg_hip.h): the dense-tile forward leaves its rows un-normalised and the
        # backward's row pass rescales them -- only where that pass exists (split backward: plan + supported sizes)
        rsc = None
        if f_rank is not None and f_plan is not None and (ks, kw, C) in ((25, 9, 3), (49, 13, 3)):
            rsc = torch.empty(2 * max(n_rows, 1), dtype=torch.float64, device=dev)
        _launch(dev, L.ssg_map_forward, _ptr(x), _ptr(y), B, C, H, W, _ptr(edges), _ptr(f_order), _ptr(f_rank),
                _ptr(f_plan), _ptr(counts), n_rows, ks, kw, sigma, eps, gen, _ptr(ssg_sr), _ptr(ssg_gt), _ptr(rsc))
        fix = _grad_fix(det, x) if want_grad else None
        _launch(dev, L.ssg_loss_backward, _ptr(x), B, C, H, W, _ptr(edges), _ptr(order), _ptr(f_rank), _ptr(f_plan),
                _ptr(counts), n_rows, ks, kw, sigma, gen, _ptr(ssg_sr), _ptr(ssg_gt), w_l1, w_kl, _ptr(upstream),
                _ptr(loss), _ptr(grad), _ptr(scratch), _ptr(fix), _ptr(rsc), 1)   # (the rows die with this call: no write-back)
        return loss, grad

    @staticmethod
    def scaled_or_redone(grad, g_l1, g_kl, redo):
        """d(l1 + kl)/d sr for the upstream gradients of l1 and kl: the saved gradient scaled when both are one and the
        same scalar, else redo(device pair of the two) -- the step again with them."""
        if g_l1.data_ptr() == g_kl.data_ptr() and g_l1.numel() == 1 and g_kl.numel() == 1:
            return grad * g_l1.to(torch.float32).reshape(())
        return redo(torch.stack([g_l1.to(torch.float32).reshape(()), g_kl.to(torch.float32).reshape(())]).contiguous())

    @staticmethod
    def forward(ctx, sr, gt, edges, counts, n_rows, ks, kw, sigma, eps, generalization, w_l1, w_kl, order, fwd, det):
        x, y = _f32c(sr), _f32c(gt)
        cfg = (n_rows, ks, kw, float(sigma), float(eps), int(bool(generalization)), float(w_l1), float(w_kl))
        want_grad = bool(ctx.needs_input_grad[0])
        loss, grad = _SSGLossFn._run(x, y, edges, counts, *cfg, order, fwd, None, want_grad, det)
        ctx.cfg, ctx.order, ctx.fwd, ctx.det = cfg, order, fwd, det
        ctx.in_dtype = sr.dtype
        if want_grad:
            ctx.save_for_backward(x, y, edges, counts, grad)
        return loss[0], loss[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_l1, g_kl):
        x, y, edges, counts, grad = ctx.saved_tensors
        out = _SSGLossFn.scaled_or_redone(grad, g_l1, g_kl, lambda up: _SSGLossFn._run(
            x, y, edges, counts, *ctx.cfg, ctx.order, ctx.fwd, up, True, ctx.det)[1])
        return (out.to(ctx.in_dtype),) + (None,) * 14


def ssg_loss(sr, gt, edges, counts, n_rows, ks=25, kw=9, sigma=0.004, eps=1e-10, generalization=True, w_l1=1.0,
             w_kl=1.0, order=None, fwd=None, deterministic=None):
    """Differentiable (l1, kl) for a batch given a device edge list; n_rows bounds N."""
    _need_gpu(sr, gt, edges, counts, order)
    check_plan(fwd, ks)
    return _SSGLossFn.apply(sr, gt, edges, counts, int(n_rows), int(ks), int(kw), sigma, eps, generalization, w_l1,
                            w_kl, order, fwd, deterministic)


class _SSGFusedFn(torch.autograd.Function):
    """(l1, kl) of a batch straight from the mask: ONE C call (ssg_loss_fwd_bwd in its fused form, ssg_sr = ssg_gt =
    NULL) builds the edge list, both SSGs as scratch rows inside the workspace, the criteria and d(l1+kl)/d sr.  Only
    that gradient (and the inputs, for the rare case below) is kept for backward(), which scales it by the incoming
    gradient; if autograd hands two DIFFERENT gradients for l1 and kl the step is redone through _SSGLossFn with them.
    `counts` (B+2 int32, device) receives the edge counts of the call."""

    @staticmethod
    def forward(ctx, sr, gt, mask, counts, cap, ks, kw, sigma, eps, generalization, w_l1, w_kl, mask_stride, lap_threshold,
                det):
        L = _lib.lib()
        x, y = _f32c(sr), _f32c(gt)
        B, C, H, W = x.shape
        mp, kind = _mask_kind(mask, C)
        mc = 3 if mp is None else mp.shape[1]
        want_grad = bool(ctx.needs_input_grad[0])
        dev = x.device
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        grad = torch.empty_like(x) if want_grad else None      # (an OUTPUT of ssg_loss_step: no fill kernel)
        nb = L.ssg_loss_workspace_bytes(B, H, W, cap, ks) + L.ssg_loss_rows_bytes(cap, ks)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        fix = _grad_fix(det, x) if want_grad else None
        _launch(dev, L.ssg_loss_step, _ptr(x), _ptr(y), _ptr(mp), kind, mc, B, C, H, W, ks, kw, float(sigma), float(eps),
                int(bool(generalization)), float(w_l1), float(w_kl), int(mask_stride or 0), float(lap_threshold), cap,
                None, None, _ptr(counts), _ptr(loss), _ptr(grad), _ptr(ws), nb, _ptr(fix))
        ctx.cfg = (cap, ks, kw, sigma, eps, generalization, w_l1, w_kl, mask_stride, lap_threshold, det)
        ctx.in_dtype = sr.dtype
        ctx.has_mask = mask is not None
        if want_grad:
            ctx.save_for_backward(x, y, grad, *((mask,) if mask is not None else ()))
        return loss[0], loss[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_l1, g_kl):
        x, y, grad = ctx.saved_tensors[:3]
        mask = ctx.saved_tensors[3] if ctx.has_mask else None

        def redo(up):
            cap, ks, kw, sigma, eps, gen, w_l1, w_kl, stride, thr, det = ctx.cfg
            el = edge_list(mask=mask, gt=y if mask is None else None, mask_stride=stride, lap_threshold=thr,
                           capacity=cap, ks=ks)
            return _SSGLossFn._run(x, y, el.edges, el.counts, cap, ks, kw, float(sigma), float(eps), int(bool(gen)),
                                   float(w_l1), float(w_kl), el.order, el.fwd, up, True, det)[1]

        out = _SSGLossFn.scaled_or_redone(grad, g_l1, g_kl, redo)
        return (out.to(ctx.in_dtype),) + (None,) * 14


def ssg_loss_from_mask(sr, gt, mask, counts, capacity, ks=25, kw=9, sigma=0.004, eps=1e-10, generalization=True,
                       w_l1=1.0, w_kl=1.0, mask_stride=0, lap_threshold=20.0, deterministic=None):
    """Differentiable (l1, kl) of a batch from its mask (or from GT's Laplacian, mask=None) in one fused C call."""
    _need_gpu(sr, gt, mask, counts)
    return _SSGFusedFn.apply(sr, gt, mask, counts, int(capacity), int(ks), int(kw), sigma, eps, generalization, w_l1,
                             w_kl, mask_stride, lap_threshold, deterministic)


class LossStep:
    """The whole loss step in ONE C call (ssg_loss_step = ssg_loss_fwd_bwd with the gradient as an output): edge list, SSG(sr), SSG(gt),
    L1 + KL and d(l1+kl)/d sr, with persistent buffers sized for `capacity` edge pixels.

    This is the path bench.py times.  No host synchronisation happens inside; `counts[0]`
    (device) holds the edge-pixel count N of the last step, `loss` the two scalars.

    Memory (k_s = 49): besides the two SSG tensors (2 x capacity x k_s^2 x 4 bytes) a materialising step holds the two
    TILE-MAJOR regions the dense kernels work in (ssg_loss_tm_bytes: about the same again -- +5 GB at capacity 512 x 512),
    the fused step (materialise=False) four row regions in its workspace instead of two.  tile_major=False leaves the
    regions out of a materialising step's workspace: the row-major kernels run (C5: 8.4 instead of 7.3 ms per step).
    A step that finds more edge pixels than `capacity` returns NaN losses (it has used the first `capacity` only).
    The default capacity (every pixel, never overflows) costs the C2 step ~2 % and the C4 step ~5 % against a bound near
    the real count (bench.py: N + 1024) -- tools/r5_capacity_cost.py; the workspace grows with it.

    graph=True records the step's ~17 launches (memset, edge-list builder, two forward variants,
    backward, finalize) into a HIP graph on first use and replays it afterwards: nothing in the
    step depends on host-side values (the edge count stays on the device), so the recording is
    valid for any input CONTENT at the same addresses; a call with other tensors re-records.
    """

    def __init__(self, B, C, H, W, ks=25, kw=9, sigma=0.004, eps=1e-10, generalization=True, w_l1=1.0, w_kl=1.0,
                 mask_stride=0, lap_threshold=20.0, capacity=None, device="cuda", graph=False, deterministic=None,
                 materialise=True, tile_major=True):
        L = _lib.lib()
        self.shape = (B, C, H, W)
        self.cfg = (ks, kw, float(sigma), float(eps), int(bool(generalization)), float(w_l1), float(w_kl),
                    int(mask_stride or 0), float(lap_threshold))
        self.capacity = int(capacity if capacity is not None else B * H * W)
        P = ks * ks
        # materialise=False: the fused step of the C ABI (no SSG output) -- the rows are scratch inside the workspace
        self.materialise = bool(materialise)
        self.ssg_sr = torch.empty((self.capacity, P), dtype=torch.float32, device=device) if materialise else None
        self.ssg_gt = torch.empty((self.capacity, P), dtype=torch.float32, device=device) if materialise else None
        self.counts = torch.zeros(B + 2, dtype=torch.int32, device=device)
        self.loss = torch.zeros(2, dtype=torch.float32, device=device)
        self.grad = torch.zeros((B, C, H, W), dtype=torch.float32, device=device)
        self.ws_bytes = L.ssg_loss_workspace_bytes(B, H, W, self.capacity, ks)
        if not materialise:
            self.ws_bytes += L.ssg_loss_rows_bytes(self.capacity, ks)
        elif tile_major:   # (k_s 49: room for the tile-major regions, which a materialising call then uses as well; 0 otherwise)
            self.ws_bytes += L.ssg_loss_tm_bytes(self.capacity, ks)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.fix = _grad_fix(deterministic, self.grad)   # deterministic mode: fixed-point accumulation buffer
        self.use_graph = bool(graph)
        self._graph, self._graph_key, self._graph_refs = None, None, None

    def edges(self):
        """View of the workspace's edge list (capacity,3) int32."""
        return self.ws[: self.capacity * 12].view(torch.int32).view(self.capacity, 3)

    def __call__(self, sr, gt, mask=None):
        """mask (B,c1,H,W) float32/uint8, or None -> Laplacian mask of gt generated on device."""
        _need_gpu(sr, gt, mask)
        B, C, H, W = self.shape
        ks, kw, sigma, eps, gen, w_l1, w_kl, stride, thr = self.cfg
        assert tuple(sr.shape) == self.shape and tuple(gt.shape) == self.shape
        assert sr.dtype == torch.float32 and gt.dtype == torch.float32 and sr.is_contiguous() and gt.is_contiguous()
        if mask is None:
            kind, mc, mp = 2, 3, None
        elif mask.dtype == torch.uint8 or mask.dtype == torch.bool:
            kind, mc, mp = 1, mask.shape[1], mask.view(torch.uint8)
        else:
            kind, mc, mp = 0, mask.shape[1], mask
            assert mask.dtype == torch.float32
        if mp is not None:
            assert mp.is_contiguous()

        def launch():
            # (ssg_loss_step: the gradient is an output of the call -- no fill kernel in front of it)
            _launch(self.grad.device, _lib.lib().ssg_loss_step, _ptr(sr), _ptr(gt), _ptr(mp), kind, mc, B, C, H, W, ks, kw,
                    sigma, eps, gen, w_l1, w_kl, stride, thr, self.capacity, _ptr(self.ssg_sr), _ptr(self.ssg_gt),
                    _ptr(self.counts), _ptr(self.loss), _ptr(self.grad), _ptr(self.ws), self.ws_bytes, _ptr(self.fix))

        if not self.use_graph:
            launch()
            return self.loss, self.grad
        key = (_ptr(sr), _ptr(gt), _ptr(mp), kind, mc)
        if self._graph is None or key != self._graph_key:
            launch()                      # eager once: function attributes are set outside the recording
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launch()
            self._graph, self._graph_key, self._graph_refs = g, key, (sr, gt, mp)   # keep the recorded buffers alive
        self._graph.replay()
        return self.loss, self.grad


# ------------------------------------- the fused pixel losses: LDL, best-buddy, back-projection (ssg_pixel.hpp) ----
class _FusedLossFn(torch.autograd.Function):
    """A scalar loss whose ONE C call produces the loss and d loss / d x together: ldl_loss, bbl_loss and bp_loss.
    `call(want_grad)` runs the family's checks and its C call and returns (loss (1,) fp32, gradient or None); only the
    gradient is kept, and backward() scales it by the incoming one (the pattern of _SSGLossFn)."""

    @staticmethod
    def forward(ctx, x, call):
        loss, grad = call(bool(ctx.needs_input_grad[0]))
        if grad is not None:
            ctx.save_for_backward(grad)
        ctx.in_dtype = x.dtype
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return (grad * g.to(torch.float32).reshape(())).to(ctx.in_dtype), None


def _loss_and_grad(x, want_grad):
    """The two outputs of a fused loss call on the fp32 input x: (loss (1,), gradient like x or None)."""
    return torch.empty(1, dtype=torch.float32, device=x.device), torch.empty_like(x) if want_grad else None


# ------------------------------------------------------------------------- LDL's artifact map (ssg_ldl.hip) ----
def _ldl_prepare(output, gt, ema, ksize):
    """fp32 contiguous copies of (output, gt, ema) after the checks every LDL entry point makes."""
    _need_gpu(output, gt, ema)
    for name, t in (("gt", gt), ("ema", ema)):
        if t is not None and t.requires_grad:
            raise ValueError(f"ssl_amd: LDL's artifact map is differentiable with respect to the output only, but `{name}` "
                             "requires grad; detach it (both reference callers pass it without a gradient)")
    if output.dim() != 4 or gt.shape != output.shape or (ema is not None and ema.shape != output.shape):
        raise ValueError(f"ssl_amd: output, gt (and ema) must be (B,C,H,W) of one shape, got {tuple(output.shape)}, "
                         f"{tuple(gt.shape)}" + ("" if ema is None else f", {tuple(ema.shape)}"))
    return _f32c(output), _f32c(gt), None if ema is None else _f32c(ema), int(ksize)


class _ArtifactMapFn(torch.autograd.Function):
    """w = get_(refined_)artifact_map(gt, output, ema, k) (loss_util.py:129-161), (B,1,H,W); backward: one
    ssg_artifact_map_backward call for any upstream dL/dw."""

    @staticmethod
    def forward(ctx, output, gt, ema, k):
        x, y, z, k = _ldl_prepare(output, gt, ema, k)
        B, C, H, W = x.shape
        w = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
        ws, nb = _workspace(_lib.lib().ssg_ldl_workspace_bytes(B, H, W), x.device)
        _launch(x.device, _lib.lib().ssg_artifact_map, _ptr(x), _ptr(y), _ptr(z), B, C, H, W, k, _ptr(w), _ptr(ws), nb)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, y, z)
        ctx.k, ctx.in_dtype = k, output.dtype
        return w.to(output.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_w):
        x, y, z = ctx.saved_tensors
        B, C, H, W = x.shape
        gw = _f32c(grad_w)
        grad = torch.empty_like(x)
        ws, nb = _workspace(_lib.lib().ssg_ldl_workspace_bytes(B, H, W), x.device)
        _launch(x.device, _lib.lib().ssg_artifact_map_backward, _ptr(x), _ptr(y), _ptr(z), _ptr(gw), B, C, H, W, ctx.k,
                _ptr(grad), _ptr(ws), nb)
        return grad.to(ctx.in_dtype), None, None, None


def artifact_map(output, gt, ema=None, ksize=7):
    """LDL's artifact map (B,1,H,W) of a batch, differentiable with respect to `output`: get_refined_artifact_map with
    `ema`, get_artifact_map without.  fp16 / bf16 inputs are computed in fp32.  An image whose residual is constant
    (output == gt) gets a NaN gradient, as in the reference (its pow backward forms 0 * inf)."""
    return _ArtifactMapFn.apply(output, gt, ema, ksize)


def ldl_loss(output, gt, ema=None, ksize=7, loss_weight=1.0, reduction='mean'):
    """L1Loss(w * output, w * gt) with w = artifact_map(output, gt, ema, ksize), fused: the callers'
    ldlssl_model.py:220-224 / realesrgan_model.py:222-226 in one call.  reduction 'mean' or 'sum'."""
    mean = _reduction_is_mean("ldl_loss", reduction)

    def call(want_grad):
        x, y, z, k = _ldl_prepare(output, gt, ema, ksize)
        B, C, H, W = x.shape
        loss, grad = _loss_and_grad(x, want_grad)
        ws, nb = _workspace(_lib.lib().ssg_ldl_workspace_bytes(B, H, W), x.device)
        _launch(x.device, _lib.lib().ssg_ldl_loss, _ptr(x), _ptr(y), _ptr(z), B, C, H, W, k, float(loss_weight),
                int(mean), _ptr(loss), _ptr(grad), _ptr(ws), nb)
        return loss, grad

    return _FusedLossFn.apply(output, call)


class _LocalVarFn(torch.autograd.Function):
    """get_local_weights (loss_util.py:106-126): unbiased variance of the k x k reflect-padded window, per plane."""

    @staticmethod
    def forward(ctx, residual, k):
        _need_gpu(residual)
        if residual.dim() != 4:
            raise ValueError(f"ssl_amd: get_local_weights takes a (B,C,H,W) residual, got {tuple(residual.shape)}")
        r = _f32c(residual)
        B, C, H, W = r.shape
        v = torch.empty_like(r)
        ws, nb = _workspace(_lib.lib().ssg_ldl_workspace_bytes(B * C, H, W), r.device)
        _launch(r.device, _lib.lib().ssg_local_variance, _ptr(r), B * C, H, W, int(k), _ptr(v), None, None, _ptr(ws), nb)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(r)
        ctx.k, ctx.in_dtype = int(k), residual.dtype
        return v.to(residual.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_v):
        r, = ctx.saved_tensors
        B, C, H, W = r.shape
        gv = _f32c(grad_v)
        grad = torch.empty_like(r)
        ws, nb = _workspace(_lib.lib().ssg_ldl_workspace_bytes(B * C, H, W), r.device)
        _launch(r.device, _lib.lib().ssg_local_variance, _ptr(r), B * C, H, W, ctx.k, None, _ptr(gv), _ptr(grad), _ptr(ws),
                nb)
        return grad.to(ctx.in_dtype), None


def local_variance(residual, ksize):
    """get_local_weights(residual, ksize): (B,C,H,W) -> (B,C,H,W), differentiable with respect to `residual`."""
    return _LocalVarFn.apply(residual, ksize)


# ------------------------------------------------- BebyGAN's best-buddy loss and flat mask (ssg_bbl.hip) ----
def _bbl_prepare(x, gt, alpha, beta, ksize, stride):
    """fp32 contiguous copies of (x, gt) after the checks every best-buddy entry point makes."""
    _need_gpu(x, gt)
    if gt.requires_grad:
        raise ValueError("ssl_amd: the best-buddy loss is differentiable with respect to the output only, but `gt` "
                         "requires grad; detach it (the reference's caller passes it without a gradient)")
    if x.dim() != 4 or gt.shape != x.shape:
        raise ValueError(f"ssl_amd: x and gt must be (B,C,H,W) of one shape, got {tuple(x.shape)}, {tuple(gt.shape)}")
    ksize, stride = int(ksize), int(stride)
    if stride < ksize:
        raise NotImplementedError(f"ssl_amd: the best-buddy search needs stride >= ksize (patches that do not "
                                  f"overlap), got ksize={ksize}, stride={stride}")
    if x.shape[1] * ksize * ksize > 31:
        raise NotImplementedError(f"ssl_amd: the best-buddy search holds a patch of at most 31 elements, got "
                                  f"C*ksize^2 = {x.shape[1] * ksize * ksize}")
    if not (alpha >= 0 and beta >= 0 and alpha + beta > 0):
        raise ValueError(f"ssl_amd: the best-buddy weights must be non-negative and not both zero, got alpha={alpha}, "
                         f"beta={beta}")
    return _f32c(x), _f32c(gt), ksize, stride


def _bbl_patches(H, W, k, s):
    return ((H - k) // s + 1) * ((W - k) // s + 1)


def bbl_search(x, gt, alpha=1.0, beta=1.0, ksize=3, stride=3, want_p1=True, want_sel=True):
    """BBL.forward's search (bebyganssl_model.py:541-565) without autograd: (ind int32 (B,N), p1, sel_p2 (B,N,d));
    ind indexes cat[p2, unfold(gt_2), unfold(gt_4)], the lowest index among equal fp32 scores."""
    xs, gs, k, s = _bbl_prepare(x, gt, alpha, beta, ksize, stride)
    B, C, H, W = xs.shape
    ws, nb = _workspace(_lib.lib().ssg_bbl_workspace_bytes(B, C, H, W, k, s), xs.device)
    N, d = max(_bbl_patches(H, W, k, s), 0), C * k * k
    ind = torch.empty((B, N), dtype=torch.int32, device=xs.device)
    p1 = torch.empty((B, N, d), dtype=torch.float32, device=xs.device) if want_p1 else None
    sel = torch.empty((B, N, d), dtype=torch.float32, device=xs.device) if want_sel else None
    _launch(xs.device, _lib.lib().ssg_bbl_search, _ptr(xs), _ptr(gs), B, C, H, W, k, s, float(alpha), float(beta),
            _ptr(ind), _ptr(p1), _ptr(sel), _ptr(ws), nb)
    return ind, p1, sel


class _BBLPatchesFn(torch.autograd.Function):
    """(p1, sel_p2) of BBL.forward.  p1 = unfold(x) is differentiable with respect to x: with stride >= ksize its
    backward, the fold, moves every patch element to the one pixel it came from (no sums).  sel_p2 carries none (the
    reference's comes from gt alone; min passes no gradient through its indices)."""

    @staticmethod
    def forward(ctx, x, gt, alpha, beta, k, s):
        _, p1, sel = bbl_search(x, gt, alpha, beta, k, s)
        ctx.geom = (tuple(x.shape), int(k), int(s))
        ctx.in_dtype = x.dtype
        ctx.mark_non_differentiable(sel)
        return p1.to(x.dtype), sel.to(x.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_p1, g_sel):
        (B, C, H, W), k, s = ctx.geom
        g = torch.nn.functional.fold(g_p1.to(torch.float32).permute(0, 2, 1), (H, W), kernel_size=k, stride=s)
        return g.to(ctx.in_dtype), None, None, None, None, None


def bbl_patches(x, gt, alpha=1.0, beta=1.0, ksize=3, stride=3):
    """BBL(alpha, beta, ksize, 0, stride).forward(x, gt) -> (p1, sel_p2), both (B,N,d)."""
    return _BBLPatchesFn.apply(x, gt, alpha, beta, ksize, stride)


def bbl_loss(x, gt, alpha=1.0, beta=1.0, ksize=3, stride=3, loss_weight=1.0, reduction='mean'):
    """L1Loss(*BBL(alpha, beta, ksize, 0, stride).forward(x, gt)), fused: the caller's bebyganssl_model.py:723-724 in
    one call.  reduction 'mean' or 'sum'."""
    mean = _reduction_is_mean("bbl_loss", reduction)

    def call(want_grad):
        xs, gs, k, s = _bbl_prepare(x, gt, alpha, beta, ksize, stride)
        B, C, H, W = xs.shape
        loss, grad = _loss_and_grad(xs, want_grad)
        ws, nb = _workspace(_lib.lib().ssg_bbl_workspace_bytes(B, C, H, W, k, s), xs.device)
        _launch(xs.device, _lib.lib().ssg_bbl_loss, _ptr(xs), _ptr(gs), B, C, H, W, k, s, float(alpha), float(beta),
                float(loss_weight), int(mean), _ptr(loss), _ptr(grad), None, _ptr(ws), nb)
        return loss, grad

    return _FusedLossFn.apply(x, call)


def flat_mask(img, kernel_size=11, std_thresh=0.025):
    """get_flat_mask(img, kernel_size, std_thresh, scale=1) (bebyganssl_model.py:93-104): (B,3,H,W) -> (B,1,H,W) of
    0.0 / 1.0, no gradient."""
    _need_gpu(img)
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"ssl_amd: get_flat_mask takes a (B,3,H,W) image, got {tuple(img.shape)}")
    x = _f32c(img)
    B, _, H, W = x.shape
    mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, _lib.lib().ssg_flat_mask, _ptr(x), B, H, W, int(kernel_size), float(std_thresh), _ptr(mask))
    return mask.to(img.dtype)


# ------------------------------------------- BebyGAN's back-projection loss and its imresize (ssg_bp.hip) ----
def _bp_pad(s):
    """Pixels of symmetric padding per side at factor s: (K - s) // 2 with K = 4s (s even) or 4s - 1 (s odd)."""
    return ((4 * s if s % 2 == 0 else 4 * s - 1) - s) // 2


def _bp_prepare(x, lq, s):
    """The fp32 contiguous copy of x (and of lq) after the checks every back-projection entry point makes; x is
    (..., H, W) with any number of leading plane dimensions."""
    _need_gpu(x, lq)
    s = int(s)
    if s not in (2, 3, 4):
        raise NotImplementedError(f"ssl_amd: the antialiased bicubic downsampling runs the integer factors 2, 3 and 4 "
                                  f"only, got {s}")
    if x.dim() < 2 or not x.dtype.is_floating_point:
        raise ValueError(f"ssl_amd: expected a floating tensor of at least two dimensions, got {tuple(x.shape)} "
                         f"{x.dtype}")
    H, W = x.shape[-2:]
    if x.numel() == 0:
        raise ValueError(f"ssl_amd: an empty tensor of shape {tuple(x.shape)} holds no image to downsample")
    if min(H, W) < _bp_pad(s):
        raise ValueError(f"ssl_amd: an image of {H} x {W} is smaller than the {_bp_pad(s)} pixels of symmetric padding "
                         f"at factor {s} (the reference's padding loop raises IndexError)")
    if lq is not None:
        if lq.requires_grad:
            raise ValueError("ssl_amd: the back-projection loss is differentiable with respect to the output only, "
                             "but `lq` requires grad; detach it (the reference's caller passes it without a gradient)")
        if tuple(lq.shape) != tuple(x.shape[:-2]) + (H // s, W // s):
            raise ValueError(f"ssl_amd: lq must be {tuple(x.shape[:-2]) + (H // s, W // s)} for an output of "
                             f"{tuple(x.shape)} at factor {s}, got {tuple(lq.shape)}")
        lq = _f32c(lq)
    return _f32c(x), lq, s


class _BPDownsampleFn(torch.autograd.Function):
    """y = imresize(x, 1 / s) on the discrete-kernel path; backward: one ssg_bp_downsample_backward call (the exact
    adjoint of symmetric padding + strided correlation) for any upstream dL/dy."""

    @staticmethod
    def forward(ctx, x, s):
        xs, _, s = _bp_prepare(x, None, s)
        H, W = xs.shape[-2:]
        P = xs.numel() // (H * W)
        y = torch.empty(tuple(xs.shape[:-2]) + (H // s, W // s), dtype=torch.float32, device=xs.device)
        _launch(xs.device, _lib.lib().ssg_bp_downsample, _ptr(xs), P, H, W, s, _ptr(y))
        ctx.geom, ctx.in_dtype = (tuple(xs.shape), P, s), x.dtype
        return y.to(x.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        shape, P, s = ctx.geom
        gy = _f32c(grad_y)
        grad = torch.empty(shape, dtype=torch.float32, device=gy.device)
        _launch(gy.device, _lib.lib().ssg_bp_downsample_backward, _ptr(gy), P, shape[-2], shape[-1], s, _ptr(grad))
        return grad.to(ctx.in_dtype), None


def bp_downsample(x, s):
    """MATLAB's antialiased bicubic 1/s of (..., H, W) -> (..., H // s, W // s), s in {2, 3, 4}: the reference's
    imresize(x, scale=1 / s) (bebyganssl_model.py:375-469), differentiable with respect to x.  Computed in fp32
    whatever the floating dtype of x, and cast back."""
    return _BPDownsampleFn.apply(x, s)


def bp_loss(x, lq, s=4, loss_weight=1.0, reduction='mean'):
    """L1Loss(imresize(x, scale=1 / s), lq), fused: the caller's bebyganssl_model.py:727-731 in one call.  reduction
    'mean' or 'sum'."""
    mean = _reduction_is_mean("bp_loss", reduction)

    def call(want_grad):
        xs, ls, f = _bp_prepare(x, lq, s)
        H, W = xs.shape[-2:]
        P = xs.numel() // (H * W)
        loss, grad = _loss_and_grad(xs, want_grad)
        ws, nb = _workspace(_lib.lib().ssg_bp_workspace_bytes(P, H, W, f), xs.device)
        _launch(xs.device, _lib.lib().ssg_bp_loss, _ptr(xs), _ptr(ls), P, H, W, f, float(loss_weight), int(mean),
                _ptr(loss), _ptr(grad), None, _ptr(ws), nb)
        return loss, grad

    return _FusedLossFn.apply(x, call)


# --------------------------------------------------------------------- KAIR's SSIM criterion (ssg_ssim.hip) ----
SSIM_MAX_WINDOW = 11


def _ssim_sums(x, y, window_size, want_grad):
    """One ssg_ssim_loss call: (sums (B + 1,) fp64 -- the map summed per image, then over the batch -- and
    d sums[B] / d x or None)."""
    B, C, H, W = x.shape
    sums = torch.empty(B + 1, dtype=torch.float64, device=x.device)
    grad = torch.empty_like(x) if want_grad else None
    ws, nb = _workspace(_lib.lib().ssg_ssim_workspace_bytes(B, C, H, W), x.device)
    _launch(x.device, _lib.lib().ssg_ssim_loss, _ptr(x), _ptr(y), B, C, H, W, window_size, _ptr(grad), _ptr(sums),
            _ptr(ws), nb)
    return sums, grad


class _SSIMFn(torch.autograd.Function):
    """SSIM of (img1, img2) with the UNSCALED gradients d (sum of the map) / d img formed in the forward call: one C call
    per argument that requires grad (the second with the roles swapped -- the map is symmetric bit for bit, so its sums
    serve as well), the loss-only call when neither does.  backward() multiplies by the upstream coefficient of each map
    value."""

    @staticmethod
    def forward(ctx, img1, img2, window_size, size_average):
        x, y = _f32c(img1), _f32c(img2)
        B, C, H, W = x.shape
        need1, need2 = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        # the map is the same bits with the images exchanged, so whichever call runs supplies the sums: one tile pass per
        # gradient wanted, the loss-only pass when none is
        g1 = g2 = None
        if need1 or not need2:
            sums, g1 = _ssim_sums(x, y, window_size, need1)
        if need2:
            swapped, g2 = _ssim_sums(y, x, window_size, True)
            sums = sums if need1 else swapped
        ctx.save_for_backward(*(g for g in (g1, g2) if g is not None))
        ctx.has, ctx.size_average, ctx.dtypes = (need1, need2), bool(size_average), (img1.dtype, img2.dtype)
        if size_average:
            return (sums[B] / float(B * C * H * W)).to(torch.float32)
        return (sums[:B] / float(C * H * W)).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        saved = list(ctx.saved_tensors)
        ref = saved[0]
        B, C, H, W = ref.shape
        gout = gout.to(torch.float32)
        coef = gout.reshape(()) / float(B * C * H * W) if ctx.size_average else gout.reshape(B, 1, 1, 1) / float(C * H * W)
        out = [None, None]
        for i in (0, 1):
            if ctx.has[i]:
                out[i] = (saved.pop(0) * coef).to(ctx.dtypes[i])
        return out[0], out[1], None, None


def ssim_loss(img1, img2, window_size=11, size_average=True):
    """loss_ssim.py's ssim(img1, img2, window_size, size_average): the mean of the SSIM map under the window_size^2
    Gaussian window ('same', zero padding), a scalar, or (B,) per-image means with size_average=False; fp32 whatever the
    floating dtype of the inputs, differentiable once with respect to either image or both."""
    _need_gpu(img1, img2)
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError(f"ssl_amd: ssim takes two (B,C,H,W) images of one shape, got {tuple(img1.shape)} and "
                         f"{tuple(img2.shape)}")
    if not img1.dtype.is_floating_point or not img2.dtype.is_floating_point:
        raise ValueError(f"ssl_amd: ssim takes floating tensors, got {img1.dtype} and {img2.dtype}")
    if img1.numel() == 0:
        raise ValueError(f"ssl_amd: an empty tensor of shape {tuple(img1.shape)} holds no image")
    return _SSIMFn.apply(img1, img2, check_ssim_window(window_size), size_average)


def check_ssim_window(window_size):
    """The window sizes the kernels run: odd, 1 .. 11 (a smaller window is the 11-tap kernel with zero taps)."""
    if window_size != int(window_size) or int(window_size) < 1:
        raise ValueError(f"ssl_amd: window_size must be a positive integer, got {window_size!r}")
    window_size = int(window_size)
    if window_size % 2 == 0:
        raise ValueError(f"ssl_amd: SSIM runs odd window sizes up to {SSIM_MAX_WINDOW} only, got {window_size} (the "
                         "reference's even sizes change the output shape)")
    if window_size > SSIM_MAX_WINDOW:
        raise ValueError(f"ssl_amd: SSIM runs odd window sizes up to {SSIM_MAX_WINDOW} only, got {window_size}")
    return window_size


# ----------------------------------- SPSR's gradient map and the pixel criteria on it (ssg_spsr.hip, section (R)) ----
PIXEL_KINDS = {name: _lib.CONSTANTS["SSG_PIX_" + name.upper()] for name in ("l1", "mse", "charbonnier")}


def _pixel_kind(kind, eps, kinds=PIXEL_KINDS):
    if kind not in kinds:
        raise ValueError(f"ssl_amd: criterion must be one of {sorted(kinds)}, got {kind!r}")
    eps = float(eps)
    if not 0.0 <= eps < float("inf"):
        raise ValueError(f"ssl_amd: eps must be finite and not negative, got {eps!r}")
    return kinds[kind], eps


def _planes(name, x, *same):
    """(planes, H, W) of the (B,C,H,W) tensor x after the checks every entry point of the family makes."""
    _need_gpu(x, *same)
    if x.dim() != 4 or x.numel() == 0 or any(t.shape != x.shape for t in same):
        raise ValueError(f"ssl_amd: {name} takes non-empty (B,C,H,W) tensors of one shape, got "
                         + ", ".join(str(tuple(t.shape)) for t in (x,) + same))
    if not all(t.dtype.is_floating_point for t in (x,) + same):
        raise ValueError(f"ssl_amd: {name} takes floating tensors, got " + ", ".join(str(t.dtype) for t in (x,) + same))
    if x.numel() >= 2 ** 31:
        raise ValueError(f"ssl_amd: {name} indexes a call's elements in 31 bits, got {x.numel()}")
    return x.shape[0] * x.shape[1], x.shape[2], x.shape[3]


def _no_target_grad(name, t):
    if t.requires_grad:
        raise ValueError(f"ssl_amd: {name} is differentiable with respect to its first tensor only, but the target "
                         "requires grad; detach it")


def _sum_call(dev, fn, *args):
    """One of the family's sums entry points: (..., workspace, sum_out, stream) -> the fp64 sum, (1,) on the device."""
    total = torch.empty(1, dtype=torch.float64, device=dev)
    ws, _ = _workspace(_lib.lib().ssg_spsr_workspace_bytes(), dev)
    _launch(dev, fn, *args, _ptr(ws), _ptr(total))
    return total


def _coef(g, scale, dev):
    """The device double a gradient pass multiplies crit' by: upstream x weight / n (0 where nothing flows in)."""
    if g is None:
        return torch.zeros(1, dtype=torch.float64, device=dev)
    return g.detach().to(torch.float64).reshape(1) * scale


class _GradientMapFn(torch.autograd.Function):
    """m = sqrt(v^2 + h^2 + 1e-6) per plane (spsrssl_model.py:18-84): one ssg_spsr_map launch; backward one
    ssg_spsr_map_backward launch from x alone."""

    @staticmethod
    def forward(ctx, x):
        planes, H, W = _planes("gradient_map", x)
        a = _f32c(x)
        m = torch.empty_like(a)
        _launch(a.device, _lib.lib().ssg_spsr_map, _ptr(a), planes, H, W, _ptr(m))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(a)
        ctx.in_dtype = x.dtype
        return m.to(x.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_map):
        a, = ctx.saved_tensors
        B, C, H, W = a.shape
        grad = torch.empty_like(a)
        _launch(a.device, _lib.lib().ssg_spsr_map_backward, _ptr(a), _ptr(_f32c(grad_map)), B * C, H, W, _ptr(grad))
        return grad.to(ctx.in_dtype)


def gradient_map(x):
    """SPSR's gradient map of a (B,C,H,W) batch, any C: Get_gradient(x) and Get_gradient_nopadding(x), which are the same
    arithmetic.  Differentiable once; fp16 / bf16 inputs are computed in fp32."""
    return _GradientMapFn.apply(x)


class _GradientLossFn(torch.autograd.Function):
    """scale * sum crit(G(sr) - G(gt)) in one ssg_spsr_loss launch (plus the partials' fold), G(sr) written beside it
    when asked; backward: ONE ssg_spsr_loss_backward launch for the loss's gradient and the emitted map's together."""

    @staticmethod
    def forward(ctx, sr, gt, kind, eps, scale, want_map):
        planes, H, W = _planes("gradient_loss", sr, gt)
        x, t = _f32c(sr), _f32c(gt)
        m = torch.empty_like(x) if want_map else None
        total = _sum_call(x.device, _lib.lib().ssg_spsr_loss, _ptr(x), _ptr(t), planes, H, W, kind, eps, _ptr(m))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, t)
        ctx.set_materialize_grads(False)
        ctx.call, ctx.scale, ctx.in_dtype = (planes, H, W, kind, eps), scale, sr.dtype
        loss = (total[0] * scale).to(torch.float32)
        return (loss, m.to(sr.dtype)) if want_map else loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_map=None):
        x, t = ctx.saved_tensors
        planes, H, W, kind, eps = ctx.call
        grad = torch.empty_like(x)
        gm = None if g_map is None else _f32c(g_map)
        _launch(x.device, _lib.lib().ssg_spsr_loss_backward, _ptr(x), _ptr(t), _ptr(gm),
                _ptr(_coef(g_loss, ctx.scale, x.device)), planes, H, W, kind, eps, _ptr(grad))
        return grad.to(ctx.in_dtype), None, None, None, None, None


def _scale(name, reduction, loss_weight, n):
    return float(loss_weight) / n if _reduction_is_mean(name, reduction) else float(loss_weight)


def gradient_loss(sr, gt, kind='mse', eps=1e-12, loss_weight=1.0, reduction='mean', want_map=False):
    """loss_weight * crit(gradient_map(sr), gradient_map(gt)) without either map in memory (spsrssl_model.py:363):
    kind 'l1' | 'mse' | 'charbonnier' (with its eps), reduction 'mean' | 'sum'.  want_map=True returns (loss,
    gradient_map(sr)): both are differentiable with respect to `sr`, through one backward launch."""
    kind, eps = _pixel_kind(kind, eps)
    _no_target_grad("gradient_loss", gt)
    return _GradientLossFn.apply(sr, gt, kind, eps, _scale("gradient_loss", reduction, loss_weight, sr.numel()),
                                 bool(want_map))


class _StreamLossFn(torch.autograd.Function):
    """scale * sum crit(first, second) in one streaming pass each way, the gradient going to `first` alone: the branch
    loss and the pixel criteria.  `sums(a, b)` makes the family's sums call on the fp32 tensors and returns the fp64
    (1,) sum; `grad(a, b, coef, out)` makes its gradient call (the pattern of _FusedLossFn)."""

    @staticmethod
    def forward(ctx, first, second, scale, sums, grad):
        a, b = _f32c(first), _f32c(second)
        total = sums(a, b)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(a, b)
        ctx.grad_call, ctx.scale, ctx.in_dtype = grad, scale, first.dtype
        return (total[0] * scale).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        out = torch.empty_like(a)
        ctx.grad_call(a, b, _ptr(_coef(g, ctx.scale, a.device)), _ptr(out))
        return out.to(ctx.in_dtype), None, None, None, None


def gradient_branch_loss(branch, gt, kind='l1', eps=1e-12, loss_weight=1.0, reduction='mean'):
    """loss_weight * crit(branch, gradient_map(gt)) (spsrssl_model.py:368), the map formed on the fly; the gradient goes
    to `branch` only."""
    kind, eps = _pixel_kind(kind, eps)
    _no_target_grad("gradient_branch_loss", gt)
    call = _planes("gradient_branch_loss", branch, gt) + (kind, eps)
    L = _lib.lib()
    return _StreamLossFn.apply(
        branch, gt, _scale("gradient_branch_loss", reduction, loss_weight, branch.numel()),
        lambda b, t: _sum_call(b.device, L.ssg_spsr_branch_loss, _ptr(b), _ptr(t), *call),
        lambda b, t, coef, out: _launch(b.device, L.ssg_spsr_branch_grad, _ptr(b), _ptr(t), *call, coef, out))


def pixel_loss(pred, target, kind='mse', eps=1e-12, loss_weight=1.0, reduction='mean'):
    """loss_weight * crit(pred, target) of two tensors of one shape in one streaming pass each way (MSELoss,
    CharbonnierLoss); the gradient goes to `pred` only."""
    kind, eps = _pixel_kind(kind, eps)
    _need_gpu(pred, target)
    if pred.shape != target.shape or pred.numel() == 0:
        raise ValueError(f"ssl_amd: pixel_loss takes two non-empty tensors of one shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    _no_target_grad("pixel_loss", target)
    L = _lib.lib()
    return _StreamLossFn.apply(
        pred, target, _scale("pixel_loss", reduction, loss_weight, pred.numel()),
        lambda a, b: _sum_call(a.device, L.ssg_pixel_sums, _ptr(a), _ptr(b), a.numel(), kind, eps),
        lambda a, b, coef, out: _launch(a.device, L.ssg_pixel_grad, _ptr(a), _ptr(b), a.numel(), kind, eps, coef, out))


# ------------------------------ a pixel criterion over a ragged set of tensor pairs (ssg_mcrit.hip, section (U)) ----
MULTI_KINDS = dict(PIXEL_KINDS, fro=_lib.CONSTANTS["SSG_PIX_FRO"])


def multi_pair_is_native(pred, target):
    """Whether the pair can go to the kernels as it lies in memory: fp32 tensors on one GPU (_gpu.readable: whatever the
    switch says, which governs the modules) of one non-empty shape with equal dense strides (dense_strides)."""
    return (_readable(pred, target) and pred.shape == target.shape and pred.numel() > 0
            and pred.stride() == target.stride() and dense_strides(pred))


class _MultiPixelFn(torch.autograd.Function):
    """sum_k w_k S_k (fro: sum_k w_k sqrt(S_k)) over K pairs: one ssg_mcrit_sums call (one launch over all chunks and
    the fold); backward one ssg_mcrit_grad launch that writes the gradient of every pred that wants one.  The pattern
    of _StreamLossFn, over a list."""

    @staticmethod
    def forward(ctx, kind, eps, weights, K, *tensors):
        import numpy as np
        x = [t.detach() for t in tensors[:K]]
        g = [t.detach() for t in tensors[K:]]
        dev = x[0].device
        L = _lib.lib()
        px, pg = address_array([t.data_ptr() for t in x]), address_array([t.data_ptr() for t in g])
        counts, w = address_array([t.numel() for t in x]), np.asarray(weights, dtype=np.float64)
        sums = torch.empty(K + 1, dtype=torch.float64, device=dev)
        ws, nbytes = _workspace(L.ssg_mcrit_workspace_bytes(K, counts.ctypes.data), dev)
        _launch(dev, L.ssg_mcrit_sums, K, px.ctypes.data, pg.ctypes.data, counts.ctypes.data, w.ctypes.data, kind, eps,
                _ptr(ws), nbytes, _ptr(sums))
        if any(ctx.needs_input_grad[4:4 + K]):
            ctx.save_for_backward(sums, *x, *g)
        ctx.call = (kind, eps, K, px, pg, counts, w)
        ctx.mark_non_differentiable(sums)
        return sums[K].to(torch.float32), sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout, _gsums):
        kind, eps, K, px, pg, counts, w = ctx.call
        sums, x = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + K]
        dev = sums.device
        grads = [torch.empty_like(x[k]) if ctx.needs_input_grad[4 + k] else None for k in range(K)]
        pgrad = address_array([0 if t is None else t.data_ptr() for t in grads])
        _launch(dev, _lib.lib().ssg_mcrit_grad, K, px.ctypes.data, pg.ctypes.data, pgrad.ctypes.data, counts.ctypes.data,
                w.ctypes.data, kind, eps, _ptr(sums), _ptr(_coef(gout, 1.0, dev)))
        return (None, None, None, None) + tuple(grads) + (None,) * K


def multi_pixel_loss(preds, targets, weights, kind='l1', eps=1e-12, reduction='mean', return_sums=False):
    """sum_k weights[k] * crit(preds[k], targets[k]) over K pairs of any sizes in one launch each way: kind 'l1' | 'mse' |
    'charbonnier' (with its eps) under reduction 'mean' (each pair's own mean) | 'sum', or 'fro', the Frobenius norm
    of each difference (the reduction is not read).  Every pair must satisfy multi_pair_is_native; the gradient goes
    to each pred that requires it, and targets must not require grad.  return_sums=True returns (loss, the K + 1
    device doubles S_0 .. S_{K-1}, total)."""
    code, eps = _pixel_kind(kind, eps, MULTI_KINDS)
    preds, targets, weights = list(preds), list(targets), [float(v) for v in weights]
    K = len(preds)
    if K < 1 or len(targets) != K or len(weights) != K:
        raise ValueError(f"ssl_amd: multi_pixel_loss takes K >= 1 preds, targets and weights, got {K}, {len(targets)} "
                         f"and {len(weights)}")
    mean = kind != 'fro' and _reduction_is_mean("multi_pixel_loss", reduction)
    for p, t in zip(preds, targets):
        _need_gpu(p, t)
        if not multi_pair_is_native(p, t):
            raise ValueError("ssl_amd: multi_pixel_loss takes pairs of fp32 tensors of one non-empty shape with equal "
                             f"dense strides on one GPU, got {tuple(p.shape)} {p.dtype} {p.stride()} and "
                             f"{tuple(t.shape)} {t.dtype} {t.stride()}")
        if p.device != preds[0].device:
            raise ValueError("ssl_amd: multi_pixel_loss takes the pairs of one GPU")
        _no_target_grad("multi_pixel_loss", t)
    if any(v != v for v in weights):
        raise ValueError("ssl_amd: multi_pixel_loss takes weights that are numbers, got a NaN")
    scaled = [v / p.numel() if mean else v for v, p in zip(weights, preds)]
    loss, sums = _MultiPixelFn.apply(code, eps, scaled, K, *preds, *targets)
    return (loss, sums) if return_sums else loss
