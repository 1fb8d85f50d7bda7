"""The best-buddy contract (ssl_amd/csrc/ssg_bbl.hip, header comment) restated in torch, evaluated in fp64.

Plain and slow on purpose: the dense (B,N,M) score matrix is formed, which is what the kernels avoid.  Used by
test_cpu_bbl.py (against the reference's own outputs, tests/golden/f19_bbl.npz) and by test_gpu_bbl.py (against the
kernels, at sizes no fixture covers).  Everything takes and returns CPU tensors; inputs are promoted to fp64.
"""
import numpy as np
import torch
import torch.nn.functional as F

TAPS = (-0.09375, 0.59375, 0.59375, -0.09375)   # cubic convolution, A = -0.75, at fraction 0.5


def half_or_quarter(t, shift):
    """Bicubic 1/2 (shift 1) or 1/4 (shift 2) of (B,C,H,W): align_corners=False, no antialias, output side
    floor(side / 2^shift); every output sample sits at fraction 0.5, taps at 2y-1..2y+2 or 4y..4y+3, clamped."""
    t = t.double()
    H, W = t.shape[-2:]
    Ho, Wo = H >> shift, W >> shift
    off = -1 if shift == 1 else 0
    ys = torch.arange(Ho) * (1 << shift) + off
    xs = torch.arange(Wo) * (1 << shift) + off
    rows = sum(w * t[..., (ys + r).clamp(0, H - 1), :] for r, w in enumerate(TAPS))
    return sum(w * rows[..., :, (xs + c).clamp(0, W - 1)] for c, w in enumerate(TAPS))


def unfold(t, k, s):
    """(B,C,H,W) -> (B, n, C k^2): F.unfold(t, k, stride=s).permute(0, 2, 1)."""
    return F.unfold(t.double(), k, padding=0, stride=s).permute(0, 2, 1).contiguous()


def candidates(gt, k=3, s=3):
    """cat[p2, u(gt_2), u(gt_4)] (B,M,d) and the three level sizes."""
    levels = [unfold(gt, k, s), unfold(half_or_quarter(gt, 1), k, s), unfold(half_or_quarter(gt, 2), k, s)]
    return torch.cat(levels, 1), [l.shape[1] for l in levels]


def scores(x, gt, alpha=1.0, beta=1.0, k=3, s=3, rows=None):
    """score_ij = alpha |p1_i - cand_j|^2 + beta |p2_i - cand_j|^2 as differences (no expansion), fp64.
    rows: optional index tensor of the rows to evaluate.  Returns (score (B,n,M), p1 (B,n,d), cand)."""
    p1, p2 = unfold(x, k, s), unfold(gt, k, s)
    cand, _ = candidates(gt, k, s)
    if rows is not None:
        p1, p2 = p1[:, rows], p2[:, rows]
    sc = alpha * torch.cdist(p1, cand, compute_mode='donot_use_mm_for_euclid_dist') ** 2
    if beta != 0:
        sc = sc + beta * torch.cdist(p2, cand, compute_mode='donot_use_mm_for_euclid_dist') ** 2
    return sc, p1, cand


def argmin_lowest(sc):
    """argmin over the last axis, the lowest index among equal values."""
    M = sc.shape[-1]
    mn = sc.min(-1, keepdim=True).values
    return torch.where(sc == mn, torch.arange(M).expand_as(sc), torch.full_like(sc, M, dtype=torch.long)).min(-1).values


def gap_to_distinct(sc, cand, best, chunk=256):
    """For every row the fp64 score distance from the best candidate to the best candidate of DIFFERENT content
    (identical patches tie exactly and are not a decision).  sc (B,n,M), cand (B,M,d), best (B,n)."""
    B, n, M = sc.shape
    out = torch.empty(B, n, dtype=torch.float64)
    for b in range(B):
        for i0 in range(0, n, chunk):
            sl = slice(i0, min(i0 + chunk, n))
            same = (cand[b][None, :, :] == cand[b][best[b, sl]][:, None, :]).all(-1)
            rest = sc[b, sl].masked_fill(same, float('inf')).min(-1).values
            out[b, sl] = rest - sc[b, sl].gather(1, best[b, sl][:, None])[:, 0]
    return out


def tau(d, alpha, beta, x, gt):
    """fp32 evaluation bound of the expanded score, doubled because two scores are compared:
    2 * 128 * 2^-24 * d * (alpha + beta) * max(|x|, |gt|)^2."""
    m = max(float(x.abs().max()), float(gt.abs().max()))
    return 2 * 128 * 2.0 ** -24 * d * (alpha + beta) * m * m


def loss_and_grad(x, cand, ind, k=3, s=3, loss_weight=1.0, reduction='mean'):
    """loss_weight * mean (or sum) |p1 - cand[ind]| and its gradient with respect to x (B,C,H,W), fp64, at the
    given indices; sgn(0) = 0, zero outside the patch grid.  Also returns p1 - sel."""
    x = x.double()
    B, C, H, W = x.shape
    p1 = unfold(x, k, s)
    sel = cand.gather(1, ind.long()[..., None].expand(-1, -1, cand.shape[-1]))
    diff = p1 - sel
    scale = loss_weight / diff.numel() if reduction == 'mean' else loss_weight
    loss = scale * diff.abs().sum()
    grad = F.fold((scale * torch.sign(diff)).permute(0, 2, 1), (H, W), kernel_size=k, stride=s)
    return loss, grad, diff


def flat_std(img, k=11):
    """Unbiased standard deviation of the k x k window of L = (0.2989 r + 0.587 g) + 0.114 b, reflect-padded by
    k // 2: (B,1,H,W) fp64."""
    img = img.double()
    lum = ((0.2989 * img[:, 0] + 0.587 * img[:, 1]) + 0.114 * img[:, 2])[:, None]
    win = F.pad(lum, [k // 2] * 4, mode='reflect').unfold(2, k, 1).unfold(3, k, 1)
    return win.var(dim=(-1, -2), unbiased=True).sqrt()


# ----------------------------------------------------------------------------------------------- test inputs ----
def smooth_noise(rng, shape, sigma):
    """Gaussian-filtered white noise, stretched to [0, 1] per image."""
    r = int(3 * sigma)
    t = torch.arange(-r, r + 1, dtype=torch.float64)
    g = torch.exp(-t * t / (2 * sigma * sigma))
    g = (g / g.sum())
    z = torch.from_numpy(rng.standard_normal(shape))
    B, C, H, W = shape
    z = F.pad(z.reshape(B * C, 1, H, W), [r] * 4, mode='reflect')
    z = F.conv2d(F.conv2d(z, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1)).reshape(shape)
    lo, hi = z.amin((1, 2, 3), keepdim=True), z.amax((1, 2, 3), keepdim=True)
    return (z - lo) / (hi - lo)


def textured_gt(rng, shape):
    """Sinusoids of several orientations plus smooth noise, in [0, 1]: patches repeat approximately across the image
    and across scales, so that searches land on other patches and on the coarser levels."""
    B, C, H, W = shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    img = torch.empty(shape, dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            fx, fy, ph = rng.uniform(0.15, 0.6), rng.uniform(0.15, 0.6), rng.uniform(0, 6.28)
            img[b, c] = 0.5 + 0.25 * torch.sin(fx * xx + fy * yy + ph) * torch.cos(0.07 * xx - 0.05 * yy + c)
    img = 0.7 * img + 0.3 * smooth_noise(rng, shape, 2.0)
    return img.clamp(0, 1).float()


def box_blur(t, radius):
    k = 2 * radius + 1
    B, C, H, W = t.shape
    p = F.pad(t.reshape(B * C, 1, H, W), [radius] * 4, mode='replicate')
    return F.avg_pool2d(p, k, stride=1).reshape(B, C, H, W)


def degraded(rng, gt, radius, noise):
    """Box blur of the GT plus Gaussian noise: an output whose patches are nearer other patches than their own."""
    x = box_blur(gt.double(), radius) if radius else gt.double().clone()
    if noise:
        x = x + noise * torch.from_numpy(rng.standard_normal(tuple(gt.shape)))
    return x.float()


def natural_like_u8(rng, B, H, W):
    """An 8-bit-quantised image (B,3,H,W) in [0, 1] with smooth shading, texture and exactly flat regions."""
    img = 0.6 * smooth_noise(rng, (B, 3, H, W), 6.0) + 0.4 * smooth_noise(rng, (B, 3, H, W), 1.0)
    img[:, :, : H // 3, : W // 2] = torch.from_numpy(rng.random((B, 3, 1, 1)))
    img[:, :, H // 2:, W // 2:] = 0.25
    return (torch.round(img * 255) / 255).float()
