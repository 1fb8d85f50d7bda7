"""fp64 restatement of SPSR's gradient map and the pixel criteria on it (ssl_amd/csrc/ssg_spsr.hip, include/ssg_hip.h
section (R)): the map, its adjoint, the three criteria, the two fused losses with their gradients, and the error bound
an fp32 evaluation is held to.  torch on the CPU, nothing of ssl_amd.

Contract, per H x W plane (any leading dimensions), zeros outside the plane:
    v = x[i+1,j] - x[i-1,j],  h = x[i,j+1] - x[i,j-1],  m = sqrt(v^2 + h^2 + E),  E = fl32(1e-6)
    adjoint of w:  dx[i,j] = a[i-1,j] - a[i+1,j] + b[i,j-1] - b[i,j+1],  a = w v / m,  b = w h / m
    criteria on d = p - q:   l1 |d|, l' = sign(d), sign(0) = 0;   mse d^2, l' = 2 d;
                             charbonnier sqrt(d^2 + eps), l' = d / sqrt(d^2 + eps), eps = fl32(eps)
    pixel loss     L = s sum l(p - q)                     dL/dp = c l'(p - q),              c = upstream s
    gradient loss  L = s sum l(G(x) - G(t))               dL/dx = adjoint of (c l'(G(x) - G(t)) + g_map)
    branch loss    L = s sum l(branch - G(gt))            dL/dbranch = c l'(branch - G(gt))
with s = loss_weight / n ('mean') or loss_weight ('sum').  Everything is evaluated in fp64 from the fp32 inputs.

The bound (first order, u = 2^-24; every fp32 operation rounds once, relative to the value it rounds):
  map       the two subtractions (u on v and on h), the two squares (2 u from their argument and u of their own: 3 u on
            v^2 and on h^2), their sum (u more: 4 u (v^2 + h^2)), the sum with E (u more: 5 u s at most, because v^2 +
            h^2 <= s), the square root (half of that, 2.5 u, and u of its own): MAP_U = 3.5 roundings on m.  s >= 1e-6,
            so a square that underflows (below 2^-126) is 25 orders below u s and is not counted.
  adjoint   one gathered term a = (w v) / m: v (u), m (3.5 u), the product and the quotient (u each): TERM_U = 6.5
            roundings on |a| -- autograd's own order, (w / (2 m)) (2 v), counts the same --; the three additions that
            join the four terms round a partial sum that never exceeds the sum of the four magnitudes: 3 u of it.
            ADJ_U = TERM_U + 3 = 9.5 roundings on sum|terms|, the same for each of the four gathered terms.  A product
            w v below the normal range may be flushed (2^-126) before it is divided by m >= 1e-3: ADJ_TINY = (4 * 1001 +
            1) 2^-126 for the four terms and the result.
  d         the difference the criterion sees: the errors of what it subtracts, 3.5 u per map value, and the
            subtraction's own u |d|.
  criteria  l1: |.| is 1-Lipschitz, the error of d.  mse: (2 |d| + e) e for an error e of d (the second-order term
            matters where d = 0) and u of the square.  charbonnier: 1-Lipschitz in d, and the square, the sum with eps
            and the root round to 2 u l (u d^2 + u s under a root, u of its own).
            l1': a step: 2 where |d| does not exceed its error (the sign is then undecided), else exact.  mse': 2 e.
            charbonnier': e times the largest second derivative within e of d, eps / ((|d| - e)^2 + eps)^1.5, capped
            at 2, and three roundings (2 u of the root, u of the quotient) on |l'|; with eps = 0 it is l1's step.
  w         the weight that reaches a map value, c l' + g_map: |c| times the error of l' and at most W_U = 4 roundings
            (the reference's chain: the upstream's product with the loss weight, the division by n, the product with
            l', and the sum with g_map; the kernels' (float)(c l') + g_map has two) on |c l'| + |g_map|.
  loss      |s| sum of the element bounds + 3 u |L| (the scale, the weight, the cast).  The kernels add in fp64; the
            reference's recorded loss comes from torch's fp32 cascade sum, n_sum = 4 ceil(log2 n) + 64 additions on one
            element's path: + |s| n_sum u sum|l| where that loss is compared (reference_sum=True).
  gradient  pixel and branch: |c| (error of l') + W_U u |grad| + 2^-126.
            gradient loss: sum over the four gathered terms of (error of w) |v| / m, + ADJ_U u sum|terms| + ADJ_TINY.

This is a worst-case envelope that catches structural errors (a wrong sign, neighbour, plane boundary, coefficient or a
dropped element); the shares the reference's fp32 results and the kernels use are recorded in profiles/spsr_parity.txt.
"""
import math
from types import SimpleNamespace as Result

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126
MAP_U = 3.5
TERM_U = 6.5
ADJ_U = TERM_U + 3
ADJ_TINY = (4 * 1001 + 1) * TINY
W_U = 4
RES_U = 3
D = torch.float64
E = float(np.float32(1e-6))

KINDS = ("l1", "mse", "charbonnier")


def _t(a):
    return torch.as_tensor(a).detach().to(D)


def fl32(v):
    return float(np.float32(v))


def n_sum(n):
    return 4 * math.ceil(math.log2(max(n, 2))) + 64


def shift(t, di, dj):
    """s[..., i, j] = t[..., i + di, j + dj], 0 outside the plane (|di|, |dj| <= 1)."""
    H, W = t.shape[-2:]
    p = F.pad(t, (1, 1, 1, 1))
    return p[..., 1 + di:1 + di + H, 1 + dj:1 + dj + W]


def vh(x):
    x = _t(x)
    return shift(x, 1, 0) - shift(x, -1, 0), shift(x, 0, 1) - shift(x, 0, -1)


def gmap(x):
    v, h = vh(x)
    return torch.sqrt(v * v + h * h + E)


def jvp(x, dx):
    """The Jacobian of the map at x applied to dx."""
    v, h = vh(x)
    dv, dh = vh(dx)
    return (v * dv + h * dh) / gmap(x)


def _gather(a, b):
    return shift(a, -1, 0), shift(a, 1, 0), shift(b, 0, -1), shift(b, 0, 1)


def adjoint(x, w):
    """(the transposed Jacobian applied to w, the sum of the magnitudes of its four gathered terms)."""
    v, h = vh(x)
    m = gmap(x)
    au, ad, bl, br = _gather(_t(w) * v / m, _t(w) * h / m)
    return au - ad + bl - br, au.abs() + ad.abs() + bl.abs() + br.abs()


def map_bound(x):
    return MAP_U * U * gmap(x)


def adjoint_bound(x, w, w_err=None):
    """The bound of the adjoint of w at x; w_err: what w itself may be off by, element by element."""
    v, h = vh(x)
    m = gmap(x)
    bound = ADJ_U * U * adjoint(x, w)[1] + ADJ_TINY
    if w_err is not None:
        bound = bound + sum(_gather(w_err * v.abs() / m, w_err * h.abs() / m))
    return bound


def crit(kind, d, eps=0.0):
    if kind == "l1":
        return d.abs()
    if kind == "mse":
        return d * d
    return torch.sqrt(d * d + fl32(eps))


def dcrit(kind, d, eps=0.0):
    if kind == "l1":
        return torch.sign(d)
    if kind == "mse":
        return 2 * d
    return d / torch.sqrt(d * d + fl32(eps))          # (eps = 0 and d = 0: 0 / 0, a NaN, as the torch expression gives)


def crit_err(kind, d, e, eps=0.0):
    """What l(d) of an fp32 evaluation may be off by when its d is off by e."""
    if kind == "l1":
        return e
    if kind == "mse":
        return (2 * d.abs() + e) * e + U * (d.abs() + e) ** 2
    return e + 2 * U * crit(kind, d.abs() + e, eps)


def dcrit_err(kind, d, e, eps=0.0):
    step = 2.0 * (d.abs() <= e).to(D)
    if kind == "l1" or (kind == "charbonnier" and fl32(eps) == 0.0):
        return step
    if kind == "mse":
        return 2 * e
    near = (d.abs() - e).clamp(min=0)
    curve = fl32(eps) / (near * near + fl32(eps)) ** 1.5
    return torch.minimum(e * curve, torch.full_like(d, 2.0)) + 3 * U * dcrit(kind, d, eps).abs()


def scale_of(reduction, loss_weight, n):
    return loss_weight / n if reduction == "mean" else loss_weight


def _loss_bound(kind, d, e, eps, s, L, reference_sum):
    b = abs(s) * float(crit_err(kind, d, e, eps).sum()) + RES_U * U * abs(float(L))
    if reference_sum:
        b += abs(s) * n_sum(d.numel()) * U * float(crit(kind, d, eps).sum())
    return b


# ---- the streaming pixel criteria ----
def pixel(p, q, kind, eps=0.0, s=1.0, c=None):
    """Result: .loss, .grad (dL/dp), .loss_bound(reference_sum=False), .grad_bound; c: upstream * s (default s)."""
    c = s if c is None else c
    d = _t(p) - _t(q)
    L = s * crit(kind, d, eps).sum()
    g = c * dcrit(kind, d, eps)
    e = U * d.abs()
    return Result(loss=L, grad=g, grad_bound=abs(c) * dcrit_err(kind, d, e, eps) + W_U * U * g.abs() + TINY,
                  loss_bound=lambda reference_sum=False: _loss_bound(kind, d, e, eps, s, L, reference_sum))


# ---- crit(branch, G(gt)) ----
def branch_loss(branch, gt, kind, eps=0.0, s=1.0, c=None):
    c = s if c is None else c
    m = gmap(gt)
    d = _t(branch) - m
    L = s * crit(kind, d, eps).sum()
    g = c * dcrit(kind, d, eps)
    e = MAP_U * U * m + U * d.abs()
    return Result(loss=L, grad=g, grad_bound=abs(c) * dcrit_err(kind, d, e, eps) + W_U * U * g.abs() + TINY,
                  loss_bound=lambda reference_sum=False: _loss_bound(kind, d, e, eps, s, L, reference_sum))


# ---- crit(G(x), G(t)) ----
def gradient_loss(x, t, kind, eps=0.0, s=1.0, c=None, g_map=None):
    """Result: .loss, .map (G(x)), .grad (dL/dx with the path through the emitted map's upstream gradient g_map added),
    .loss_bound(reference_sum=False), .grad_bound."""
    c = s if c is None else c
    mx, mt = gmap(x), gmap(t)
    d = mx - mt
    L = s * crit(kind, d, eps).sum()
    e = MAP_U * U * (mx + mt) + U * d.abs()
    direct = c * dcrit(kind, d, eps)
    extra = torch.zeros_like(d) if g_map is None else _t(g_map)
    w = direct + extra
    w_err = abs(c) * dcrit_err(kind, d, e, eps) + W_U * U * (direct.abs() + extra.abs())
    # (the magnitudes of the gathered terms are taken at |c l'| + |g_map|, which is at least |w|)
    bound = adjoint_bound(x, direct.abs() + extra.abs(), w_err)
    return Result(loss=L, map=mx, grad=adjoint(x, w)[0], grad_bound=bound,
                  loss_bound=lambda reference_sum=False: _loss_bound(kind, d, e, eps, s, L, reference_sum))


def share(got, want, bound):
    """The largest share of the bound a result uses (0 / 0 counts as 0; anything / 0 as inf; a NaN as inf)."""
    d = (_t(got) - _t(want)).abs()
    b = _t(bound).expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


# ---- the fixture (tests/golden/make_golden_spsr.py writes it, tests/test_cpu_spsr.py reads it) ----
FIXTURE_SHAPE = (2, 3, 9, 11)
W_GRADSR, W_BRANCH = 1e-2, 5e-1      # pixel_gradSR_opt (MSELoss) and pixel_gradBranch_opt (L1Loss) of the training file
PIXEL_CASES = tuple((name, reduction, weighted) for name in ("MSELoss", "CharbonnierLoss", "L1Loss")
                    for reduction, weighted in (("mean", False), ("sum", False), ("none", False), ("mean", True)))
PIXEL_KIND = {"MSELoss": "mse", "CharbonnierLoss": "charbonnier", "L1Loss": "l1"}
PIXEL_WEIGHT, PIXEL_EPS = 0.7, 1e-12


def fixture_inputs():
    """sr, gt: images in [0, 1]; branch: what the gradient branch puts out, near G(gt); cot: a cotangent for the map;
    weight: an element-wise weight for the criteria."""
    g = torch.Generator().manual_seed(3300)
    gt = torch.rand(FIXTURE_SHAPE, generator=g, dtype=D)
    sr = (gt + 0.1 * torch.randn(FIXTURE_SHAPE, generator=g, dtype=D)).clamp(0, 1)
    branch = gmap(gt.to(torch.float32)) + 0.05 * torch.randn(FIXTURE_SHAPE, generator=g, dtype=D)
    cot = torch.randn(FIXTURE_SHAPE, generator=g, dtype=D)
    weight = torch.rand(FIXTURE_SHAPE, generator=g, dtype=D)
    return {k: v.to(torch.float32) for k, v in dict(sr=sr, gt=gt, branch=branch, cot=cot, weight=weight).items()}
