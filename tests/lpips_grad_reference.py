"""numpy fp64 restatement of the LPIPS criterion's GRADIENT with respect to both feature maps
(ssg_lpips_layers_backward, ssl_amd/csrc/ssg_featmetric.hip, include/ssg_hip.h section (V)), written from the
definition by the chain rule, with the two per-element error bounds that the kernel and the package's fp32 torch lines
are held to.  numpy alone, nothing of ssl_amd.

Layer k with maps f0, f1 (N,C,H,W), the 1x1 convolution w (C,) and the upstream gradient coef (N,) of the value:
    n = sqrt(sum_c f^2);  i = 1 / (n + 1e-10);  a = f0 i0;  b = f1 i1;  d = sum_c w_c (a_c - b_c)^2;  s = coef / (H W)
    u_c = 2 w_c (a_c - b_c)                                           (the derivative of d with respect to a_c; -u_c for b_c)
    da_c / df0_m = [c = m] i0 - f0_c i0^2 (f0_m / n0)                 (di0 / df0_m = -i0^2 f0_m / n0)
    g0_m = s (u_m i0 - i0^2 (f0_m / n0) sum_c u_c f0_c)
    g1_m = s (-u_m i1 + i1^2 (f1_m / n1) sum_c u_c f1_c)
It is the derivative of the UNCLAMPED d.  A pixel whose own vector is all zero has n = 0: f / n = 0 / 0, and the whole
side's C elements of that pixel are NaN here, in the kernel (0 * inf) and in torch's autograd (0 * inf in sqrt's
backward); `.nan0`, `.nan1` are those masks read off the inputs.

The kernel's bound (v = 2^-53, u = 2^-24; nothing here is measured).  Both terms of g are sums whose summands have the
absolute values
    M0_m = |s| i0 (2 |w_m| (|a_m| + |b_m|) + (i0 / n0) |f0_m| sum_c 2 |w_c| (|a_c| + |b_c|) |f0_c|)
(M1 likewise), so |g| / M is the cancellation left.  The kernel forms the five sums of C products, (C + 1) v each, the
two inverse norms, (C / 2 + 3) v each and each at most three times in a term, the six scalars' products, quotient and
difference, and five operations per element: at most (2.5 C + 24) v M.  The restatement's own error on the same
element: the norms (C / 2 + 3) v, the sum over C of three-factor products (C + 3) v, eight operations: at most
(2 C + 20) v M.  Together (4.5 C + 44) v M, and ONE cast of the result to fp32: u |g| + 2^-149 (the cast is exact
below the subnormal step only up to that step).
The wider bound of the package's fp32 lines with torch's autograd counts u in place of v and their own roundings:
a and b carry (C / 2 + 5) u each (featmetric_reference.py); the backward of the quotient, of the root and of the sum
forms the norm's gradient as a sum over C in fp32 in any order, C u, of products of three factors that each carry a's
error, and divides by 2 n and (n + eps)^2 again, (C / 2 + 6) u; the remaining element-wise products, the spatial mean's
division and the difference: 10 u.  At most (2 C + 32) u M, plus u |g| + 2^-149 for the stored fp32 result.
The shares of both bounds that the kernel and torch's fp32 lines use are recorded in profiles/lpips_grad_parity.txt.
"""
from types import SimpleNamespace as Result

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
EPS = 1e-10
TINY = 2.0 ** -149


def _f(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def lpips_grad(feats0, feats1, lins, coef):
    """A list over the layers of Result(g0, g1 (N,C,H,W fp64), bound0, bound1 (the kernel's), fp64_bound0, fp64_bound1
    (their fp64 term alone: what another fp64 evaluation is held to), torch_bound0, torch_bound1 (the fp32 lines'),
    nan0, nan1 (N,1,H,W bool: the pixels whose own vector is all zero))."""
    coef = _f(coef).reshape(-1)
    out = []
    for f0, f1, w in zip(feats0, feats1, lins):
        f0, f1, w = _f(f0), _f(f1), _f(w).reshape(1, -1, 1, 1)
        N, C, H, W = f0.shape
        s = (coef / (H * W)).reshape(N, 1, 1, 1)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            n0 = np.sqrt(np.sum(f0 ** 2, axis=1, keepdims=True))
            n1 = np.sqrt(np.sum(f1 ** 2, axis=1, keepdims=True))
            i0, i1 = 1 / (n0 + EPS), 1 / (n1 + EPS)
            a, b = f0 * i0, f1 * i1
            u = 2 * w * (a - b)
            g0 = s * (u * i0 - i0 ** 2 * (f0 / n0) * np.sum(u * f0, axis=1, keepdims=True))
            g1 = s * (-u * i1 + i1 ** 2 * (f1 / n1) * np.sum(u * f1, axis=1, keepdims=True))
            m = 2 * np.abs(w) * (np.abs(a) + np.abs(b))
            M0 = np.abs(s) * i0 * (m + (i0 / n0) * np.abs(f0) * np.sum(m * np.abs(f0), axis=1, keepdims=True))
            M1 = np.abs(s) * i1 * (m + (i1 / n1) * np.abs(f1) * np.sum(m * np.abs(f1), axis=1, keepdims=True))
        kc, tc = (4.5 * C + 44) * V, (2 * C + 32) * U
        out.append(Result(g0=g0, g1=g1, nan0=n0 == 0, nan1=n1 == 0, fp64_bound0=kc * M0, fp64_bound1=kc * M1,
                          bound0=kc * M0 + U * np.abs(g0) + TINY, bound1=kc * M1 + U * np.abs(g1) + TINY,
                          torch_bound0=tc * M0 + U * np.abs(g0) + TINY, torch_bound1=tc * M1 + U * np.abs(g1) + TINY))
    return out


def share(got, want, bound, skip=None):
    """The largest share of the bound a result uses over the elements outside `skip` (0 / 0 counts as 0, a NaN as inf)."""
    got, want, bound = np.broadcast_arrays(_f(got), _f(want), _f(bound))
    keep = np.ones(got.shape, bool) if skip is None else ~np.broadcast_to(skip, got.shape)
    if not keep.any():
        return 0.0
    d = np.abs(got[keep] - want[keep])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound[keep])
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def nan_pattern(g):
    """the NaN mask of a gradient (N,C,H,W) as a bool array"""
    return np.isnan(_f(g))
