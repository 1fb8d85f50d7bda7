"""fp64 restatement of the perceptual loss's criterion over K feature pairs (ssl_amd/csrc/ssg_mcrit.hip, include/ssg_hip.h
section (U); GAN-Based-SR/basicsr/losses/basic_loss.py:226-251, train_BSGRAN/models/loss.py:122-130) and of its gradient,
with the two error bounds fp32 evaluations are held to.  torch on the CPU, nothing of ssl_amd.

Contract, for the pairs (x_k, g_k) of n_k elements with the weights w_k, d = x_k - g_k:
    l1    term_k = mean |d|            mse  term_k = mean d^2          charbonnier  term_k = mean sqrt(d^2 + eps)
    fro   term_k = sqrt(S_k), S_k = sum d^2                            ('sum' reduction: the sums instead of the means)
    L = sum_k w_k term_k               dL/dx_k = c_k l'(d), c_k = upstream w_k / n_k (fro: upstream w_k / sqrt(S_k), 0
                                       where S_k = 0), l' = sign(d), 2 d, d / sqrt(d^2 + eps), and d for fro
Everything is evaluated in fp64 from the fp32 inputs.

The kernel's bound (first order; u = 2^-24 an fp32 rounding, v = 2^-53 an fp64 rounding; nothing here is measured):
  d       one fp32 subtraction: e = u |d|.  Its sign and its being 0 are exact, so l1's l' is exact.
  l       l1: |.| is exact, e.  mse: the square of a d that is off by e, (2 |d| + e) e, and the square's own u.
          charbonnier: 1-Lipschitz in d, e, and the square, the sum with eps and the root, 2 u l.  (ssg_pixel's element
          functions: tests/spsr_reference.py counts the same roundings.)
  S_k     the sum of the element bounds; the fp32 l are widened and added in fp64: n_k v sum l.
  term    fro: the root halves the relative error of S_k and rounds once, v.  Otherwise S_k itself.
  L       sum_k |s_k| (bound of term_k), s_k = w_k / n_k formed on the host in fp64 (v); the K products and K additions
          of the fold in fp64: (2 K + 1) v sum_k |s_k term_k|; the cast of the result to fp32: u |L|.
  grad    |c_k| times the error of l' (mse: 2 e; fro: e; charbonnier: e times the largest second derivative within e of
          d, eps / ((|d| - e)^2 + eps)^1.5, capped at 2, and 3 u |l'| for the root's two roundings and the quotient's
          one), the error of c_k (two fp64 products, and for fro the relative error of sqrt(S_k) and a division: the
          relative bound of S_k halved, + 4 v), the product in fp64 (v) and ONE cast to fp32 (u), + 2^-126 for a
          result below the normal range.
Torch's bound (the reference's loop of fp32 operations, any summation order) is wider:
  S_k     + (n_k - 1) u sum l for a sum of n_k fp32 terms added in an order that is torch's own.
  term    the division by n_k and the product with w_k: 2 u each term; fro: the root's u.
  L       the K additions of the Python loop and the product with the loss weight: (K + 1) u sum |w_k term_k|.
  grad    the chain upstream -> loss weight -> w_k -> 1 / n_k -> l' rounds once per link: TORCH_GRAD_U = 6 roundings on
          |grad| instead of one; fro: the relative error of torch's norm, ((n_k - 1) u + the bound of S_k / S_k) / 2.
The shares of both bounds that the results use are recorded in profiles/perceptual_parity.txt.
"""
from types import SimpleNamespace as Result

import numpy as np
import torch

U = 2.0 ** -24
V = 2.0 ** -53
TINY = 2.0 ** -126
TORCH_GRAD_U = 6
D = torch.float64
KINDS = ("l1", "mse", "charbonnier", "fro")


def _t(a):
    if not isinstance(a, torch.Tensor):
        return torch.as_tensor(a, dtype=D)               # (a Python float keeps its 53 bits)
    return a.detach().to(D).cpu()


def fl32(v):
    return float(np.float32(v))


def crit(kind, d, eps=0.0):
    if kind == "l1":
        return d.abs()
    if kind in ("mse", "fro"):
        return d * d
    return torch.sqrt(d * d + fl32(eps))


def dcrit(kind, d, eps=0.0):
    if kind == "l1":
        return torch.sign(d)
    if kind == "mse":
        return 2 * d
    if kind == "fro":
        return d
    return d / torch.sqrt(d * d + fl32(eps))


def crit_err(kind, d, e, eps=0.0):
    if kind == "l1":
        return e
    if kind in ("mse", "fro"):
        return (2 * d.abs() + e) * e + U * (d.abs() + e) ** 2 + TINY
    return e + 2 * U * crit(kind, d.abs() + e, eps)


def dcrit_err(kind, d, e, eps=0.0):
    if kind == "l1":
        return torch.zeros_like(d)
    if kind == "mse":
        return 2 * e
    if kind == "fro":
        return e
    if fl32(eps) == 0.0:
        return torch.zeros_like(d)
    near = (d.abs() - e).clamp(min=0)
    curve = fl32(eps) / (near * near + fl32(eps)) ** 1.5
    return torch.minimum(e * curve, torch.full_like(d, 2.0)) + 3 * U * dcrit(kind, d, eps).abs()


def criterion(xs, gs, ws, kind, eps=0.0, reduction="mean", upstream=1.0):
    """Result over the K pairs: .S (fp64 sums), .terms, .total, .grads (dL/dx_k for d total = upstream), and the
    bounds .S_bound, .total_bound, .grad_bound of the kernels and .torch_total_bound, .torch_grad_bound of the
    reference's fp32 loop.  Lists have one entry per pair."""
    K = len(xs)
    S, terms, grads, S_b, term_b, grad_b, t_term_b, t_grad_b, scales = [], [], [], [], [], [], [], [], []
    for x, g, w in zip(xs, gs, ws):
        d = _t(x) - _t(g)
        n = d.numel()
        e = U * d.abs()
        l = crit(kind, d, eps)
        Sk = float(l.sum())
        elem = float(crit_err(kind, d, e, eps).sum())
        Sb = elem + n * V * float(l.abs().sum())
        tSb = Sb + (n - 1) * U * float(l.abs().sum())
        if kind == "fro":
            s = float(w)
            term = Sk ** 0.5
            rel, trel = (Sb / Sk, tSb / Sk) if Sk > 0 else (0.0, 0.0)
            tb, ttb = term * (rel / 2 + V), term * (trel / 2 + U)
            c = upstream * s / term if Sk > 0 else 0.0
            c_rel, tc_rel = rel / 2 + 4 * V, trel / 2 + 2 * U
        else:
            s = float(w) / n if reduction == "mean" else float(w)
            term, tb, ttb = Sk, Sb, tSb + 2 * U * abs(Sk)
            c = upstream * s
            c_rel, tc_rel = 2 * V, 0.0
        gk = c * dcrit(kind, d, eps)
        core = abs(c) * dcrit_err(kind, d, e, eps)
        S.append(Sk), terms.append(term), grads.append(gk), S_b.append(Sb), scales.append(s)
        term_b.append(tb), t_term_b.append(ttb)
        grad_b.append(core + (c_rel + V + U) * gk.abs() + TINY)
        t_grad_b.append(core + (tc_rel + TORCH_GRAD_U * U) * gk.abs() + TINY)
    total = sum(s * t for s, t in zip(scales, terms))
    mass = sum(abs(s * t) for s, t in zip(scales, terms))
    total_b = sum(abs(s) * b for s, b in zip(scales, term_b)) + (2 * K + 2) * V * mass + U * abs(total)
    t_total_b = sum(abs(s) * b for s, b in zip(scales, t_term_b)) + (K + 1) * U * mass + U * abs(total)
    return Result(S=S, terms=terms, total=total, grads=grads, S_bound=S_b, total_bound=total_b, grad_bound=grad_b,
                  torch_total_bound=t_total_b, torch_grad_bound=t_grad_b)


def torch_loop(xs, gs, ws, kind, weight=1.0):
    """The reference's criterion lines in torch operations, on whatever device and dtype the tensors have: the live
    oracle of the fallback (its bits) and the subject of the torch bound."""
    import torch.nn.functional as F
    loss = 0
    for x, g, w in zip(xs, gs, ws):
        if kind == "fro":
            loss += torch.norm(x - g, p="fro") * w
        else:
            loss += (F.l1_loss(x, g) if kind == "l1" else F.mse_loss(x, g)) * w
    loss *= weight
    return loss


def share(got, want, bound):
    """The largest share of the bound a result uses (0 / 0 counts as 0; anything / 0 as inf; a NaN as inf)."""
    d = (_t(got) - _t(want)).abs()
    b = _t(bound).expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())
