"""An fp64 reference of LDL's artifact map, its loss and both backwards (contract: ssl_amd/csrc/ssg_ldl.hip, header
comment), on CPU tensors.  A plain helper module: test_cpu_ldl.py holds it to the reference's own outputs (fixture
F18) on every run without a GPU, test_gpu_ldl.py and test_gpu_lds_poison.py hold the HIP kernels to it.

Two things in the contract are fp32 decisions and are taken in fp32 here as well:
  * the mask r < r_e: r = sum_c |g - o| in numpy fp32, channels added in order c = 0, 1, ...  Every step is one
    correctly rounded IEEE operation, so r, r_e and the mask are bit-defined and equal to what
    torch.sum(torch.abs(g - o), 1) and the kernel's resid() produce;
  * the sign of w*o - w*g with both products rounded separately: when the two rounded products are within rounding of
    each other, a correct implementation may see +, - or 0.  Such pixels are reported as `undecided`, not answered.
Everything else is float64 through torch.autograd with the mask held fixed."""
import numpy as np
import torch
import torch.nn.functional as F

TIE = 4e-7      # |w o - w g| <= TIE |w o|: the two fp32 products are within rounding of each other


def residual32(o, g):
    """r = sum_c |g - o| in numpy fp32, channels in order: (B,1,H,W) float32 ndarray."""
    on, gn = (t.detach().cpu().contiguous().numpy().astype(np.float32, copy=False) for t in (o, g))
    r = np.abs(gn[:, 0] - on[:, 0])
    for c in range(1, on.shape[1]):
        r = r + np.abs(gn[:, c] - on[:, c])
    assert r.dtype == np.float32
    return r[:, None]


def mask32(o, g, e):
    """The boolean mask r < r_e (B,1,H,W) as a torch tensor, decided in fp32; all False without an EMA output."""
    r = residual32(o, g)
    if e is None:
        return torch.zeros(r.shape, dtype=torch.bool)
    return torch.from_numpy(r < residual32(e, g))


def _window_var(r, k):
    pad = (k - 1) // 2
    win = F.pad(r, [pad, pad, pad, pad], mode='reflect').unfold(2, k, 1).unfold(3, k, 1)
    return torch.var(win, dim=(-1, -2), unbiased=True)


def local_variance64(residual, k, upstream=None):
    """get_local_weights alone in fp64 on any residual (B,C,H,W): (V, d sum(V * upstream) / d residual or None)."""
    x = residual.detach().cpu().double().requires_grad_(upstream is not None)
    V = _window_var(x, k)
    if upstream is None:
        return V.detach(), None
    (V * upstream.detach().cpu().double()).sum().backward()
    return V.detach(), x.grad


def reference64(o, g, e, k, lam=1.0, reduction='mean', upstream=None):
    """(loss, gradient, w, undecided) in float64 for CPU tensors o = output, g = GT, e = EMA output or None.
    loss = lam * mean (or sum) |w*o - w*g| and gradient = d loss / d o; with `upstream` (B,1,H,W) the gradient is
    d sum(w * upstream) / d o instead (the map's backward) and loss is None.  `undecided` (B,1,H,W) bool marks the
    pixels whose L1 sign fp32 does not decide (module docstring); pixels with o == g are decided (sgn(0) = 0)."""
    o, g = o.detach().cpu().float(), g.detach().cpu().float()
    e = None if e is None else e.detach().cpu().float()
    masked = mask32(o, g, e)
    x = o.double().requires_grad_(True)
    gd = g.double()
    r = torch.sum(torch.abs(gd - x), 1, keepdim=True)
    P = torch.var(r, dim=(1, 2, 3), unbiased=True, keepdim=True) ** (1 / 5)
    w = P * _window_var(r, k)
    w = torch.where(masked, torch.zeros_like(w), w)
    if upstream is not None:
        (w * upstream.detach().cpu().double()).sum().backward()
        loss = None
    else:
        d = torch.abs(w * x - w * gd)
        loss = lam * (d.mean() if reduction == 'mean' else d.sum())
        loss.backward()
        loss = loss.detach()
    wf = w.detach().float()
    po, pg = wf * o, wf * g
    undecided = (((po - pg).abs() <= TIE * po.abs()) & (o != g) & (wf > 0)).any(1, keepdim=True)
    return loss, x.grad, w.detach(), undecided
