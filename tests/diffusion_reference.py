"""Oracles of the diffusion kernels (ssl_amd/csrc/ssg_diffusion.hip, include/ssg_hip.h section (W)), written from the
definitions of Diffusion-Based-SR/ldm/models/diffusion/ddpm.py and ddpmssl.py.  torch on the CPU, nothing of ssl_amd.

Sections 1, 2 and 4 (schedule, per-sample combinations, p_sample, canvas gather and stitch) are IEEE multiplications and
additions on given tables: the torch expressions below, on the CPU in fp32, are a BIT-FOR-BIT oracle.

Section 3 (the training criterion) is restated in fp64 with autograd, and an fp32 evaluation is held to a first-order
bound (u = 2^-24) around it.  TWO bounds, as tests/perceptual_reference.py keeps two: the kernels' own, which counts only
the roundings the kernels make, and a wider one for torch's fp32 lines.

The P2 weight is the reference's: `weight = extract_into_tensor(1 / (p2_k + snr) ** p2_gamma, t, target.shape)` is
(B, 1, 1, 1) and multiplies the (B,) loss_simple, so `loss` is (B, 1, 1, B), element [i, j] = w_i m_j / e_j + lv_j, and its
mean is mean_j(wbar m_j / e_j + lv_j) with wbar = mean_i w_i: every sample is weighted by the BATCH MEAN of the P2 weights.
criterion64 forms the (B, B) array as written; the kernels use wbar.

The kernels' roundings (criterion_bounds(..., torch32=False)):
  element   d = target - pred is ONE fp32 subtraction (u |d|); l1's |d| adds nothing, l2's d d one more rounding on a
            value whose relative error is already 2 u: K = 1 (l1), 3 (l2) roundings on l.
  sums      every l is widened and added in fp64: (n + chunks) additions of non-negative terms and one division, at most
            (n + 2) 2^-53 relative on a mean.  R_m = K u + (n + 2) 2^-53.
  scalars   formed in fp64 from the means (a handful of operations and one exp: F64 = 2^-44 relative to the sum of the
            terms' magnitudes, which also covers the second-order terms u^2 = 2^-48 of this first-order count), then ONE
            cast to fp32: u |scalar|.
  gradient  an element is rounded twice: the fp32 l'(d) (2 d of an fp32 d: u; exact for l1) and the cast of c_b l'
            formed in fp64: K' = 1 (l1), 2 (l2) on the criterion's term; with the x0 path the product rb gx0 (u on
            its own value) and the subtraction (u on the result).  dloss / dlogvar is formed in fp64 (F64) from the
            means (R_m on w m / e) and cast once.
  tiny      one absolute 2^-126 per element: values below the normal range may lose bits.
torch's fp32 lines (torch32=True) round more: the per-sample mean is a cascade of blocks (n_sum(n) = 4 ceil(log2 n) + 64
additions on an element's path) and a division, R_m = (K + n_sum(n) + 1) u; the P2 product, exp (2 u: an fp32 libm result
within an ulp), the quotient and the sum are 4 u on w m / e and u on l_b, then a mean over B (B B elements with P2:
n_sum + 2 roundings) and, for the loss, the two weights and their sum (3 u); autograd forms c_b in fp32 through the chain
g / B, the weights' products and sum, 1 / e, w and 1 / n: CHAIN = 8 roundings more on the criterion's term.
Both are worst-case envelopes; the shares the kernels and torch's fp32 lines use of their own bounds are recorded in
profiles/diffusion_parity.txt.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
CHAIN = 8
F64 = 2.0 ** -44
D = torch.float64


def extract(a, t, ndim):
    return a.gather(-1, t).reshape(t.shape[0], *((1,) * (ndim - 1)))


# -------------------------------------------------------------------------------------------- section 1, bit for bit ---
def beta_schedule(name, T, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """fp64 betas of the four named schedules (torch's fp64 linspace / cos, as the reference takes them)."""
    if name == "cosine":
        f = torch.cos((torch.arange(T + 1, dtype=D) / T + cosine_s) / (1 + cosine_s) * np.pi / 2).pow(2)
        f = f / f[0]
        return np.clip((1 - f[1:] / f[:-1]).numpy(), 0, 0.999)
    lo, hi, power = {"linear": (linear_start ** 0.5, linear_end ** 0.5, 2), "sqrt_linear": (linear_start, linear_end, 1),
                     "sqrt": (linear_start, linear_end, 0.5)}[name]
    line = torch.linspace(lo, hi, T, dtype=D)
    return (line if power == 1 else line ** power).numpy()


def schedule_tables(betas, parameterization="eps", v_posterior=0.):
    """register_schedule's thirteen buffers from an array of betas, in the array's own precision (fp64, or fp32 after a
    respacing; the shifted cumulative product is fp64 either way, since it is built around a Python 1.0), cast to
    float32 at the end; lvlb_weights in torch from the float32 buffers."""
    betas = np.asarray(betas)
    a = 1. - betas
    c = np.cumprod(a, axis=0)
    cp = np.append(1., c[:-1])
    var = (1 - v_posterior) * betas * (1. - cp) / (1. - c) + v_posterior * betas
    raw = dict(betas=betas, alphas_cumprod=c, alphas_cumprod_prev=cp, sqrt_alphas_cumprod=np.sqrt(c),
               sqrt_one_minus_alphas_cumprod=np.sqrt(1. - c), log_one_minus_alphas_cumprod=np.log(1. - c),
               sqrt_recip_alphas_cumprod=np.sqrt(1. / c), sqrt_recipm1_alphas_cumprod=np.sqrt(1. / c - 1),
               posterior_variance=var, posterior_log_variance_clipped=np.log(np.maximum(var, 1e-20)),
               posterior_mean_coef1=betas * np.sqrt(cp) / (1. - c), posterior_mean_coef2=(1. - cp) * np.sqrt(a) / (1. - c))
    tab = {k: torch.tensor(v, dtype=torch.float32) for k, v in raw.items()}
    if parameterization == "x0":
        c32 = torch.tensor(c, dtype=torch.float32)
        w = 0.5 * torch.sqrt(c32) / (2. - c32)
    else:
        w = tab["betas"] ** 2 / (2 * tab["posterior_variance"] * torch.tensor(a, dtype=torch.float32) * (1 - tab["alphas_cumprod"]))
        w = torch.ones_like(w) if parameterization == "v" else w
    w[0] = w[1]
    tab["lvlb_weights"] = w
    return tab


def respaced_betas(alphas_cumprod32, keep):
    """The float32 betas of a respacing: 1 - a_i / a_previous over the kept steps (the first against 1.0), in float32."""
    a = alphas_cumprod32[sorted(keep)]
    return (1 - a / torch.cat([torch.ones(1), a[:-1]])).numpy()


# -------------------------------------------------------------------------------------------- section 2, bit for bit ---
def combine(A, x, Bt, y, t, subtract, clamp=None):
    a, b = extract(A, t, x.dim()) * x, extract(Bt, t, x.dim()) * y
    out = a - b if subtract else a + b
    return out if clamp is None else out.clamp(*clamp)


def p_sample(tab, x, model_out, t, noise, parameterization, clip, return_x0=False):
    """tab: the schedule's buffers by name (fp32, CPU) and `sigma`."""
    if parameterization == "eps":
        rec = combine(tab["sqrt_recip_alphas_cumprod"], x, tab["sqrt_recipm1_alphas_cumprod"], model_out, t, True)
    elif parameterization == "x0":
        rec = model_out.clone()
    else:
        rec = combine(tab["sqrt_alphas_cumprod"], x, tab["sqrt_one_minus_alphas_cumprod"], model_out, t, True)
    if clip:
        rec = rec.clamp(-1., 1.)
    mean = combine(tab["posterior_mean_coef1"], rec, tab["posterior_mean_coef2"], x, t, False)
    mask = (1 - (t == 0).float()).reshape(x.shape[0], *((1,) * (x.dim() - 1)))
    out = mean + mask * extract(tab["sigma"], t, x.dim()) * noise
    return (out, rec) if return_x0 else out


def same_bits(got, want):
    """The number of elements that differ: bits where the oracle is finite or infinite, NaN-ness where it is a NaN."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    nan = torch.isnan(want)
    view = torch.int32 if want.dtype == torch.float32 else torch.int64
    differ = torch.where(nan, ~torch.isnan(got), got.view(view) != want.view(view))
    return int(differ.sum())


# ------------------------------------------------------------------------------------------------ section 3, fp64 ---
def n_sum(n):
    return 4 * math.ceil(math.log2(max(n, 2))) + 64


def criterion64(pred, target, x_noisy, t, tab, logvar, loss_type, lsw, elbo, p2=None, upstream=1.0, grad_x0=None):
    """The criterion in fp64 with autograd: the four scalars, the per-sample means and S_b, x0, and the gradients of
    upstream loss + <grad_x0, x0> to pred and logvar.  With P2 the loss is the reference's (B, B) broadcast."""
    p = pred.detach().to(D).requires_grad_(True)
    lv = logvar.detach().to(D).requires_grad_(True)
    d = target.detach().to(D) - p
    ell = d.abs() if loss_type == "l1" else d * d
    n = ell[0].numel()
    S = ell.flatten(1).sum(1)
    m = S / n
    lvt = lv[t]
    if p2 is None:
        w = torch.ones_like(m)
        gamma = (m / torch.exp(lvt) + lvt).mean()
    else:
        wi = p2.to(D)[t]
        w = wi.mean().expand_as(m)
        gamma = (wi[:, None] * m[None, :] / torch.exp(lvt)[None, :] + lvt[None, :]).mean()      # [i, j]
    lb = w * m / torch.exp(lvt) + lvt
    vw = tab["lvlb_weights"].to(D)[t]
    vlb = (vw * m).mean()
    loss = lsw * gamma + elbo * vlb
    ra = extract(tab["sqrt_recip_alphas_cumprod"].to(D), t, p.dim())
    rb = extract(tab["sqrt_recipm1_alphas_cumprod"].to(D), t, p.dim())
    x0 = ra * x_noisy.detach().to(D) - rb * p
    total = upstream * loss
    if grad_x0 is not None:
        total = total + (grad_x0.detach().to(D) * x0).sum()
    gp, glv = torch.autograd.grad(total, (p, lv), allow_unused=True)
    return dict(S=S.detach(), m=m.detach(), w=w.detach(), e=torch.exp(lvt).detach(), lb=lb.detach(), vw=vw, rb=rb,
                scalars=torch.stack([m.mean(), gamma, vlb, loss]).detach(), x0=x0.detach(), grad_pred=gp,
                grad_logvar=torch.zeros_like(lv) if glv is None else glv, d=d.detach(), n=n, p2=p2 is not None,
                crit_grad=None if grad_x0 is None else gp + rb * grad_x0.detach().to(D))


def criterion_bounds(r, loss_type, lsw, elbo, upstream=1.0, grad_x0=None, torch32=False):
    """(bounds on the four scalars, per-element bound on grad_pred, per-sample terms of the bound on grad_logvar (see
    logvar_bound), relative bound on S_b) for the result r of criterion64: the kernels' bound, or with torch32 the one
    for torch's fp32 lines."""
    K = 1 if loss_type == "l1" else 3
    B, n = r["m"].numel(), r["n"]
    m, w, e, lb, vw = r["m"], r["w"], r["e"], r["lb"], r["vw"]
    term = (w * m / e).abs()
    simple, gamma, vlb, loss = (float(v) for v in r["scalars"])
    crit = r["grad_pred"] if grad_x0 is None else r["crit_grad"]
    back = None if grad_x0 is None else (r["rb"] * grad_x0.detach().to(D)).abs()
    if torch32:
        Rm = (K + n_sum(n) + 1) * U
        over = (n_sum(B * B if r["p2"] else B) + 2) * U
        b_simple = Rm * simple + (n_sum(B) + 2) * U * simple
        b_gamma = float((term * (Rm + 4 * U) + U * lb.abs()).mean()) + over * float((term + r["lb"].abs()).mean())
        b_vlb = float((vw.abs() * m * (Rm + U)).mean()) + (n_sum(B) + 2) * U * float((vw.abs() * m).mean())
        b_loss = abs(lsw) * b_gamma + abs(elbo) * b_vlb + 3 * U * (abs(lsw * gamma) + abs(elbo * vlb))
        b_grad = (2 + CHAIN) * U * crit.abs() + U * r["grad_pred"].abs() + TINY
        if back is not None:
            b_grad = b_grad + 2 * U * back
        per = abs(upstream * lsw) / B * (term * (Rm + 4 * U) + (2 + CHAIN) * U * (1 + term))
        return [b_simple, b_gamma, b_vlb, b_loss], b_grad, per, Rm
    Rm = K * U + (n + 2) * 2.0 ** -53
    mag_gamma, mag_vlb = float((term + (lb - w * m / e).abs()).mean()), float((vw.abs() * m).mean())
    pre_gamma = Rm * float(term.mean()) + F64 * mag_gamma
    pre_vlb = (Rm + F64) * mag_vlb
    b_simple = (Rm + F64) * simple + U * simple
    b_gamma = pre_gamma + U * abs(gamma)
    b_vlb = pre_vlb + U * abs(vlb)
    b_loss = abs(lsw) * pre_gamma + abs(elbo) * pre_vlb + F64 * (abs(lsw) * mag_gamma + abs(elbo) * mag_vlb) + U * abs(loss)
    b_grad = ((K + 1) // 2 * U + F64) * crit.abs() + TINY       # K' = 1 (l1), 2 (l2)
    if back is not None:
        b_grad = b_grad + U * back + U * r["grad_pred"].abs()
    per = abs(upstream * lsw) / B * (term * Rm + F64 * (1 + term))
    return [b_simple, b_gamma, b_vlb, b_loss], b_grad, per, Rm


def share(got, want, bound):
    """The largest share of the bound a result uses (0 / 0 counts as 0; anything / 0 as inf)."""
    got, want = torch.as_tensor(got).detach().cpu().to(D), torch.as_tensor(want).detach().cpu().to(D)
    d = (got - want).abs()
    b = torch.as_tensor(bound, dtype=D).expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    return float(r.max()) if r.numel() else 0.0


def logvar_bound(per, t, T, want=None):
    """The per-sample terms of criterion_bounds scattered to the (T,) entries, + the one fp32 cast of the entry (`want`,
    the exact gradient) + TINY."""
    out = torch.zeros(T, dtype=D)
    out.index_add_(0, t, per)
    return out + TINY + (0 if want is None else U * want.detach().abs())


def criterion_torch32(pred, target, x_noisy, t, tab, logvar, loss_type, lsw, elbo, p2=None, grad_x0=None):
    """The reference's own fp32 lines (ddpmssl.py:391-417) with autograd, on the CPU: what the bound must hold as well."""
    p = pred.detach().clone().requires_grad_(True)
    lv = logvar.detach().clone().requires_grad_(True)
    diff = target - p
    per = (diff.abs() if loss_type == "l1" else torch.nn.functional.mse_loss(target, p, reduction="none")).mean([1, 2, 3])
    simple = per.mean()
    ls = per if p2 is None else extract(p2, t, 4) * per      # the reference's own line: (B, 1, 1, 1) x (B,) -> (B, 1, 1, B)
    lvt = lv[t]
    loss = ls / torch.exp(lvt) + lvt
    gamma = loss.mean()
    loss = lsw * loss.mean()
    vlb = (tab["lvlb_weights"][t] * per).mean()
    loss = loss + elbo * vlb
    x0 = (extract(tab["sqrt_recip_alphas_cumprod"], t, p.dim()) * x_noisy -
          extract(tab["sqrt_recipm1_alphas_cumprod"], t, p.dim()) * p)
    total = loss if grad_x0 is None else loss + (grad_x0 * x0).sum()
    gp, glv = torch.autograd.grad(total, (p, lv))
    return dict(scalars=torch.stack([simple, gamma, vlb, loss]).detach(), x0=x0.detach(), grad_pred=gp, grad_logvar=glv)


# -------------------------------------------------------------------------------------------- section 4, bit for bit ---
def canvas_tiles(h, w, ts, overlap):
    """[(oy, ox)] in the loop order of p_mean_variance_canvas and (grid_rows, grid_cols): rows step along the width."""
    def offsets(extent):
        out = []
        while not out or out[-1] + ts < extent:
            out.append(max(len(out) * ts - overlap * len(out), 0))
        out[-1] = extent - ts
        return out
    xs, ys = offsets(w), offsets(h)
    return [(oy, ox) for ox in xs for oy in ys], (len(xs), len(ys))


def canvas_gather(x, tiles, ts):
    return torch.cat([x[:, :, oy:oy + ts, ox:ox + ts] for oy, ox in tiles], dim=0)


def canvas_stitch(preds, tiles, shape, weights, sources=None, order=None):
    """torch's own in-place lines: out[window] += pred * w (an fp64 product added into an fp32 tensor), cnt[window] += w,
    out /= cnt.  sources[k]: the slice of preds tile k takes (default: its B samples); order: the tiles' order."""
    B = shape[0]
    ts = preds.shape[-1]
    out, cnt = torch.zeros(shape), torch.zeros(shape)
    for k in (range(len(tiles)) if order is None else order):
        oy, ox = tiles[k]
        p = preds[k * B:(k + 1) * B] if sources is None else preds[sources[k]]
        out[:, :, oy:oy + ts, ox:ox + ts] += p * weights if weights is not None else p
        cnt[:, :, oy:oy + ts, ox:ox + ts] += weights if weights is not None else 1
    out /= cnt
    return out


def reference_sources(grid, B):
    """Which entries of the concatenated predictions the reference's stitch reads for tile (row, col): it appends every
    sample of a tile batch to the row's list and then takes entry `col`, one (1, C, ts, ts) tile for all samples."""
    rows, cols = grid
    return [slice(r * cols * B + c, r * cols * B + c + 1) for r in range(rows) for c in range(cols)]


def gaussian_weights(tw, th):
    var = 0.01
    # (numpy's exp and sqrt, as there: numpy's vectorised exp need not be libm's to the last bit)
    def probs(n, mid):
        return [np.exp(-(i - mid) * (i - mid) / (n * n) / (2 * var)) / np.sqrt(2 * np.pi * var) for i in range(n)]
    xs, ys = probs(tw, (tw - 1) / 2), probs(th, th / 2)
    return torch.tensor(ys, dtype=D)[:, None] * torch.tensor(xs, dtype=D)[None, :]


def splitter_starts(length, patch, stride):
    if length <= patch:
        return [0]
    out = []
    for s in range(0, length, stride):
        s = min(s, length - patch)
        if s not in out:
            out.append(s)
    return out


def splitter_windows(h, w, patch, stride, sf):
    """[(h_start, h_end, w_start, w_end)] in the class's order: the width index is the outer one."""
    return [(y * sf, (y + patch) * sf, x * sf, (x + patch) * sf)
            for x in splitter_starts(w, patch, stride) for y in splitter_starts(h, patch, stride)]
