"""numpy fp64 restatement of the LPIPS (v0.1) and DISTS criteria behind their networks (ssl_amd/csrc/ssg_featmetric.hip,
include/ssg_hip.h section (V)), written literally from the packages' definitions, with the two first-order error bounds
that fp64 kernels and the packages' fp32 torch lines are held to.  numpy alone, nothing of ssl_amd.

No `lpips` or `DISTS_pytorch` package is available to the tests: that these definitions ARE the packages' is supposed,
not verified (README).

LPIPS, layer k with maps f0, f1 (N,C,H,W) and the 1x1 convolution w (C,):
    n = sqrt(sum_c f^2);  fn = f / (n + 1e-10);  d = sum_c w_c (fn0_c - fn1_c)^2 per pixel;  layer = mean_hw d;
    value = sum_k layer_k
DISTS, layer k with maps x, y and alpha, beta over all channels (two-pass variance, the package's one-pass covariance):
    mx = mean x;  vx = mean (x - mx)^2;  cov = mean(x y) - mx my
    S1 = (2 mx my + c1) / (mx^2 + my^2 + c1);  S2 = (2 cov + c2) / (vx + vy + c2);  c1 = c2 = 1e-6
    score = 1 - sum_c (alpha_c S1 + beta_c S2) / (sum alpha + sum beta)

The kernel's bound (v = 2^-53; nothing here is measured).  The kernels have fp64 error sources only.
  LPIPS   per pixel, with T = sum_c |w_c| (|fn0_c| + |fn1_c|)^2 (the size of the expansion's terms A i0^2 + 2 |B| i0 i1 +
          Cc i1^2, so T / d is the cancellation factor):  the five sums of C terms, (C + 1) v each; the two inverse norms,
          (C / 2 + 3) v each, twice in a term; the term's products and the two additions, 4 v: (2 C + 12) v T.  The
          restatement's own error on the same pixel, 2 |fn0 - fn1| (C / 2 + 4) v (|fn0| + |fn1|) per channel, is at most
          (C + 8) v T.  Together (3 C + 20) v T.  (Weights are not negative, as v0.1's are: the true d is not, and the
          kernel's clamp at 0 can only bring its result closer.)  The spatial mean: HW additions in any order and the
          division, (HW + 1) v mean d.  The sum of the K layers: K v sum |layer|.
  DISTS   a plane's sums of HW terms in any order, the division and the restatement's own error of the same size:
          q = (4 HW + 12) v on E|x|, E x^2, E|x y|.  vx = E x^2 - mx^2 cancels: its error is q E x^2 whatever vx is, and
          E x^2 / (vx + vy + c2) is the cancellation factor; cov likewise with E|x y| + |mx my|, twice (the restatement
          forms it the same way).  S1 and S2 by the quotient rule with the denominators reduced by their own error (inf
          where nothing is left).  The sum over n_ch channels and the normalisation: (2 n_ch + 8) v sum (|a S1| + |b S2|).
The wider bound of the packages' fp32 lines counts u = 2^-24 in place of v, plus their own extra roundings:
  LPIPS   fn: square, sum of C, root, + eps, quotient: (C / 2 + 5) u |fn|; the difference, its square, the weight's
          product and the sum of C: per pixel sum_c |w_c| 2 |fn0 - fn1| (C / 2 + 5) u (|fn0| + |fn1|) + (C + 3) u sum_c
          |w_c| (fn0 - fn1)^2; the mean of HW terms (HW + 1) u; the K additions K u.
  DISTS   q32 = (HW + 4) u: the means; the two-pass variance is q32 vx + (error of the mean)^2; the ONE-PASS covariance
          cancels in fp32, q32 (E|x y| + |mx my|) + the means' errors -- where that exceeds the denominator the bound is
          inf: torch's fp32 lines decide nothing there.  alpha / w_sum and c1, c2 in fp32: (n_ch + 4) u more on the sum.
The shares of both bounds that the kernels and torch's fp32 lines use are recorded in profiles/featmetric_parity.txt.
"""
from types import SimpleNamespace as Result

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
EPS = 1e-10
C1 = C2 = 1e-6


def _f(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def lpips(feats0, feats1, lins):
    """.layers (N,K), .value (N,), and the bounds .layers_bound, .value_bound (kernels), .torch_layers_bound,
    .torch_value_bound (the package's fp32 lines)."""
    layers, kb, tb = [], [], []
    for f0, f1, w in zip(feats0, feats1, lins):
        f0, f1, w = _f(f0), _f(f1), _f(w).reshape(1, -1, 1, 1)
        N, C, H, W = f0.shape
        HW = H * W
        with np.errstate(invalid="ignore"):
            a = f0 / (np.sqrt(np.sum(f0 ** 2, axis=1, keepdims=True)) + EPS)
            b = f1 / (np.sqrt(np.sum(f1 ** 2, axis=1, keepdims=True)) + EPS)
            diff = (a - b) ** 2
            d = np.sum(w * diff, axis=1)                                   # (N,H,W)
            layer = d.mean(axis=(1, 2))
            T = np.sum(np.abs(w) * (np.abs(a) + np.abs(b)) ** 2, axis=1)
            cross = np.sum(np.abs(w) * 2 * np.abs(a - b) * (np.abs(a) + np.abs(b)), axis=1)
            dbar = np.sum(np.abs(w) * diff, axis=1)
        layers.append(layer)
        kb.append(((3 * C + 20) * V * T).mean(axis=(1, 2)) + (HW + 1) * V * dbar.mean(axis=(1, 2)))
        tb.append(((C / 2 + 5) * U * cross + (C + 3) * U * dbar).mean(axis=(1, 2)) + (HW + 1) * U * dbar.mean(axis=(1, 2)))
    layers, kb, tb = (np.stack(v, axis=1) for v in (layers, kb, tb))
    K = layers.shape[1]
    mass = np.abs(layers).sum(axis=1)
    return Result(layers=layers, value=layers.sum(axis=1), layers_bound=kb, value_bound=kb.sum(axis=1) + K * V * mass,
                  torch_layers_bound=tb, torch_value_bound=tb.sum(axis=1) + (K + 1) * U * mass)


def _quotient_err(num, e_num, den, e_den, r):
    """first-order error of num / den, the denominator reduced by its own error; inf where nothing of it is left"""
    left = np.abs(den) - e_den
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (e_num + np.abs(num / den) * e_den) / left + r * np.abs(num / den)
    return np.where(left > 0, out, np.inf)


def dists(feats0, feats1, alpha, beta):
    """.score (N,), .structure, .texture (the two shares, (N,)), .S1, .S2 (lists of (N,C)), and the bounds .score_bound
    (kernels) and .torch_score_bound (the package's fp32 lines)."""
    alpha, beta = _f(alpha).reshape(-1), _f(beta).reshape(-1)
    w_sum = alpha.sum() + beta.sum()
    n_ch = alpha.size
    s1 = s2 = kb = tb = mass = 0.0
    S1s, S2s, at = [], [], 0
    for x, y in zip(feats0, feats1):
        x, y = _f(x), _f(y)
        N, C, H, W = x.shape
        HW = H * W
        a, b = alpha[at:at + C] / w_sum, beta[at:at + C] / w_sum
        at += C
        ax = (2, 3)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mx, my = x.mean(axis=ax), y.mean(axis=ax)
            vx = ((x - mx[..., None, None]) ** 2).mean(axis=ax)
            vy = ((y - my[..., None, None]) ** 2).mean(axis=ax)
            cov = (x * y).mean(axis=ax) - mx * my
            n1, d1 = 2 * mx * my + C1, mx ** 2 + my ** 2 + C1
            n2, d2 = 2 * cov + C2, vx + vy + C2
            S1, S2 = n1 / d1, n2 / d2
            ex, ey = np.abs(x).mean(axis=ax), np.abs(y).mean(axis=ax)
            exx, eyy, exy = (x * x).mean(axis=ax), (y * y).mean(axis=ax), np.abs(x * y).mean(axis=ax)
            for r, q, bounds in ((V, (4 * HW + 12) * V, "k"), (U, (HW + 4) * U, "t")):
                e_mx, e_my = q * ex, q * ey
                if bounds == "k":
                    e_vx, e_vy = q * exx, q * eyy
                    e_cov = 2 * q * (exy + np.abs(mx * my))
                else:
                    e_vx, e_vy = q * vx + e_mx ** 2, q * vy + e_my ** 2
                    e_cov = q * (exy + np.abs(mx * my)) + np.abs(mx) * e_my + np.abs(my) * e_mx
                e_n1 = 2 * (np.abs(mx) * e_my + np.abs(my) * e_mx) + 3 * r * np.abs(n1)
                e_d1 = 2 * (np.abs(mx) * e_mx + np.abs(my) * e_my) + 3 * r * np.abs(d1)
                e_S1 = _quotient_err(n1, e_n1, d1, e_d1, r)
                e_S2 = _quotient_err(n2, 2 * e_cov + 2 * r * np.abs(n2), d2, e_vx + e_vy + 2 * r * np.abs(d2), r)
                e = (np.abs(a) * e_S1 + np.abs(b) * e_S2).sum(axis=1)
                if bounds == "k":
                    kb = kb + e
                else:
                    tb = tb + e
            s1 = s1 + (a * S1).sum(axis=1)
            s2 = s2 + (b * S2).sum(axis=1)
            mass = mass + (np.abs(a * S1) + np.abs(b * S2)).sum(axis=1)
        S1s.append(S1), S2s.append(S2)
    return Result(score=1 - (s1 + s2), structure=s1, texture=s2, S1=S1s, S2=S2s,
                  score_bound=kb + (2 * n_ch + 8) * V * mass + V,
                  torch_score_bound=tb + (3 * n_ch + 12) * U * mass + U)


def lpips_second(feats0, feats1, lins):
    """LPIPS a second, independent way (N,K): d = sum_c w_c (fn0_c^2 + fn1_c^2) - 2 sum_c w_c fn0_c fn1_c with the
    normalised maps formed through the cosine's pieces, pixel sums by einsum, in long double."""
    out = []
    for f0, f1, w in zip(feats0, feats1, lins):
        f0, f1, w = (np.asarray(_f(t), dtype=np.longdouble) for t in (f0, f1, w))
        w = w.reshape(-1)
        i0 = 1 / (np.sqrt(np.einsum("nchw,nchw->nhw", f0, f0)) + np.longdouble(EPS))
        i1 = 1 / (np.sqrt(np.einsum("nchw,nchw->nhw", f1, f1)) + np.longdouble(EPS))
        A = np.einsum("c,nchw,nchw->nhw", w, f0, f0)
        B = np.einsum("c,nchw,nchw->nhw", w, f0, f1)
        Cc = np.einsum("c,nchw,nchw->nhw", w, f1, f1)
        d = A * i0 * i0 - 2 * B * i0 * i1 + Cc * i1 * i1
        out.append(np.asarray(d.mean(axis=(1, 2)), dtype=np.float64))
    return np.stack(out, axis=1)


def dists_second(feats0, feats1, alpha, beta):
    """DISTS a second, independent way (N,): one-pass moments E x^2 - (E x)^2 from plane sums in long double."""
    alpha, beta = (np.asarray(_f(t), dtype=np.longdouble).reshape(-1) for t in (alpha, beta))
    w_sum = alpha.sum() + beta.sum()
    total, at = 0, 0
    for x, y in zip(feats0, feats1):
        x, y = (np.asarray(_f(t), dtype=np.longdouble) for t in (x, y))
        N, C, H, W = x.shape
        hw = np.longdouble(H * W)
        sx, sy = x.sum(axis=(2, 3)), y.sum(axis=(2, 3))
        sxx, syy, sxy = (x * x).sum(axis=(2, 3)), (y * y).sum(axis=(2, 3)), (x * y).sum(axis=(2, 3))
        mx, my = sx / hw, sy / hw
        vx, vy, cov = sxx / hw - mx * mx, syy / hw - my * my, sxy / hw - mx * my
        S1 = (2 * mx * my + C1) / (mx * mx + my * my + C1)
        S2 = (2 * cov + C2) / (vx + vy + C2)
        total = total + (alpha[at:at + C] * S1 + beta[at:at + C] * S2).sum(axis=1)
        at += C
    return np.asarray(1 - total / w_sum, dtype=np.float64)


def share(got, want, bound):
    """The largest share of the bound a result uses (0 / 0 counts as 0; a NaN as inf; anything under an inf bound 0)."""
    got, want, bound = np.broadcast_arrays(_f(got), _f(want), _f(bound))
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    r = np.where(np.isinf(bound) & np.isfinite(d), 0.0, r)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())
