"""numpy fp64 restatement of the NIQE contract (include/ssg_hip.h section (K), ssl_amd/csrc/ssg_niqe.hip's header):
the rounded plane, the block-multiple crop, the MSCN planes under the 7 x 7 window with 'nearest' borders, MATLAB's
antialiased bicubic half, the 18 AGGD features per block and scale (vectorised over blocks), and the multivariate
Gaussian fit.  Everything from the integer plane on is float64; the reference (basicsr/metrics/niqe.py) keeps float32
planes, which is what tests/test_cpu_niqe.py measures against its recorded outputs.

Images are (H,W,C) / (C,H,W) BGR arrays holding 0 .. 255, or an (H,W) plane, as calculate_niqe receives them."""
import math

import numpy as np

import metrics_reference as MR

BS = 96
NF = 36
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
GAM = np.arange(0.2, 10.001, 0.001)          # 9,801 grid values of alpha


def window():
    """fspecial('gaussian', 7, 7/6) in closed form, (7,7), sum 1."""
    i = np.arange(7, dtype=np.float64) - 3
    d2 = i[:, None] ** 2 + i[None, :] ** 2
    g = np.exp(-d2 / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def resize_taps():
    """The 8 weights of MATLAB's antialiased bicubic at scale 1/2: Keys' kernel (a = -0.5) stretched by 2, tap t at
    distance 3.5 - t input pixels from the output's centre; normalised to sum 1."""
    x = np.abs(0.5 * (3.5 - np.arange(8, dtype=np.float64)))
    w = 0.5 * np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2)
    return w / w.sum()


_TABLE = None


def table():
    """(4, 9801): gam, r(gam) = G(2/g)^2 / (G(1/g) G(3/g)), G(1/g) / G(3/g), G(2/g) / G(1/g), by math.gamma."""
    global _TABLE
    if _TABLE is None:
        t = np.empty((4, GAM.size))
        for i, g in enumerate(GAM):
            rec = 1.0 / g
            t[0, i] = g
            t[1, i] = math.gamma(rec * 2) ** 2 / (math.gamma(rec) * math.gamma(rec * 3))
            t[2, i] = math.gamma(1 / g) / math.gamma(3 / g)
            t[3, i] = math.gamma(2 / g) / math.gamma(1 / g)
        _TABLE = t
    return _TABLE


# ------------------------------------------------------------------------------------------------------ planes ---
def plane1(img, crop_border=0, input_order='HWC', convert_to='y'):
    """The rounded plane cropped to whole blocks, float64 holding integers: (96 nbh, 96 nbw)."""
    img = np.asarray(img)
    if input_order == 'HW':
        p = np.rint(img.astype(np.float32))
    else:
        if input_order == 'CHW':
            img = img.transpose(1, 2, 0)
        elif img.ndim == 2:
            img = img[..., None]
        q = np.ascontiguousarray(np.rint(img).astype(np.uint8))
        if convert_to == 'y':
            p = np.rint(MR.planes(q, 0, True)[0])
        elif convert_to == 'gray':
            v = q.astype(np.float32) / np.float32(255.0)
            gray = (np.float32(0.114) * v[..., 0] + np.float32(0.587) * v[..., 1]) + np.float32(0.299) * v[..., 2]
            p = np.rint(gray * np.float32(255.0))
        else:
            raise ValueError(convert_to)
    p = MR.crop(p, crop_border)
    nbh, nbw = p.shape[0] // BS, p.shape[1] // BS
    return np.ascontiguousarray(p[:nbh * BS, :nbw * BS]).astype(np.float64)


def _half_axis0(v, w):
    n = v.shape[0]
    out = np.zeros((n // 2,) + v.shape[1:])
    o = np.arange(n // 2)
    for t in range(8):
        idx = 2 * o - 3 + t
        idx = np.where(idx < 0, -1 - idx, idx)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
        out = out + w[t] * v[idx]
    return out


def plane2(p1):
    """imresize(p1 / 255, 0.5) * 255: rows first, then columns, taps in index order."""
    w = resize_taps()
    v = _half_axis0(np.asarray(p1, np.float64) / 255.0, w)
    v = _half_axis0(v.T, w).T
    return np.ascontiguousarray(v * 255.0)


def mscn(p):
    """(I - mu) / (sigma + 1) with the window's 49 taps in row-major order and indices clamped at the plane's border."""
    p = np.asarray(p, np.float64)
    H, W = p.shape
    pad = np.pad(p, 3, mode='edge')
    g = window()
    mu = np.zeros_like(p)
    e2 = np.zeros_like(p)
    for i in range(7):
        for j in range(7):
            v = pad[i:i + H, j:j + W]
            mu = mu + g[i, j] * v
            e2 = e2 + g[i, j] * (v * v)
    sigma = np.sqrt(np.abs(e2 - mu * mu))
    return (p - mu) / (sigma + 1.0)


# ---------------------------------------------------------------------------------------------------- features ---
def _blocks(n, bs):
    """(nblk, bs, bs), blocks in column-major order (block column outer)."""
    nbh, nbw = n.shape[0] // bs, n.shape[1] // bs
    b = n.reshape(nbh, bs, nbw, bs).transpose(2, 0, 1, 3)
    return b.reshape(nbh * nbw, bs, bs)


def aggd(x):
    """x (nblk, N).  Returns alpha's table index, l, r, t (rhatnorm) per block; empty sides give NaN and index 0."""
    tab = table()
    with np.errstate(all='ignore'):
        sq = x * x
        neg, pos = x < 0, x > 0
        left = np.sqrt(np.where(neg, sq, 0.0).sum(1) / neg.sum(1))
        right = np.sqrt(np.where(pos, sq, 0.0).sum(1) / pos.sum(1))
        gh = left / right
        rhat = np.abs(x).mean(1) ** 2 / sq.mean(1)
        t = (rhat * (gh * gh * gh + 1) * (gh + 1)) / ((gh * gh + 1) * (gh * gh + 1))
        idx = np.array([0 if np.isnan(v) else int(np.argmin((tab[1] - v) ** 2)) for v in t])
    return idx, left, right, t


def features(n, bs):
    """(nblk, 18) features of one scale's MSCN plane, and (nblk, 5) of the fits' t (rhatnorm)."""
    tab = table()
    b = _blocks(n, bs)
    nblk = b.shape[0]
    out = np.empty((nblk, 18))
    ts = np.empty((nblk, 5))
    for k in range(5):
        m = b if k == 0 else b * np.roll(b, SHIFTS[k - 1], axis=(1, 2))
        idx, left, right, t = aggd(m.reshape(nblk, -1))
        sc = np.sqrt(tab[2, idx])
        bl, br = left * sc, right * sc
        ts[:, k] = t
        if k == 0:
            out[:, 0] = tab[0, idx]
            out[:, 1] = (bl + br) / 2
        else:
            o = 2 + 4 * (k - 1)
            out[:, o] = tab[0, idx]
            out[:, o + 1] = (br - bl) * tab[3, idx]
            out[:, o + 2] = bl
            out[:, o + 3] = br
    return out, ts


ALPHA_COLUMNS = (0, 2, 6, 10, 14)            # within one scale's 18


def midpoint_margin(t):
    """Relative distance of t to the nearest midpoint of adjacent r(gam) entries (where the argmin changes); inf for NaN."""
    r = table()[1]
    mid = 0.5 * (r[1:] + r[:-1])
    t = np.asarray(t, np.float64)
    out = np.full(t.shape, np.inf)
    ok = ~np.isnan(t)
    j = np.clip(np.searchsorted(mid, t[ok]), 1, mid.size - 1)
    out[ok] = np.minimum(np.abs(mid[j] - t[ok]), np.abs(mid[j - 1] - t[ok])) / np.abs(t[ok])
    return out


def features_from_planes(p1, p2):
    """(nblk, 36) and the (nblk, 10) t values from the two planes."""
    f1, t1 = features(mscn(p1), BS)
    f2, t2 = features(mscn(p2), BS // 2)
    return np.concatenate([f1, f2], 1), np.concatenate([t1, t2], 1)


# --------------------------------------------------------------------------------------------------------- fit ---
def fit(feat, mu_pris, cov_pris):
    """The score, its square, Sigma, d, and Sigma's condition number and eigenvalue ratio (NaN where Sigma is not
    finite)."""
    feat = np.asarray(feat, np.float64)
    mu_pris = np.asarray(mu_pris, np.float64).reshape(-1)
    cov_pris = np.asarray(cov_pris, np.float64)
    nan = dict(score=float('nan'), q2=float('nan'), cond=float('nan'), ratio=float('nan'))
    with np.errstate(all='ignore'):
        cnt = (~np.isnan(feat)).sum(0)
        mean = np.where(np.isnan(feat), 0.0, feat).sum(0) / cnt
    good = feat[~np.isnan(feat).any(1)]
    if good.shape[0] < 2 or np.isnan(mean).any():
        return nan
    c = good - good.mean(0)
    cov = c.T @ c / (good.shape[0] - 1)
    sigma = (cov_pris + cov) / 2
    d = mu_pris - mean
    ev = np.linalg.eigvalsh((sigma + sigma.T) / 2)
    q2 = float(d @ np.linalg.solve(sigma, d))
    return dict(score=math.sqrt(q2), q2=q2, cond=float(ev[-1] / ev[0]), ratio=float(ev[0] / ev[-1]), sigma=sigma, d=d)


def fit_by_numpy(feat, mu_pris, cov_pris):
    """q^2 once more by the library calls the metric is defined with: np.nanmean of the columns, np.cov of the rows
    without a NaN, np.linalg.pinv.  Another order of every sum than fit's, and an SVD instead of an LU solve."""
    feat = np.asarray(feat, np.float64)
    mu = np.nanmean(feat, axis=0)
    cov = np.cov(feat[~np.isnan(feat).any(axis=1)], rowvar=False)
    d = np.asarray(mu_pris, np.float64).reshape(1, -1) - mu.reshape(1, -1)
    return float((d @ np.linalg.pinv((np.asarray(cov_pris, np.float64) + cov) / 2) @ d.T)[0, 0])


# ----------------------------------------------------------------------------------------------- the comparisons ---
# What tests/test_gpu_niqe_blocks.py holds the kernels to, as functions of arrays, so that tests/test_cpu_niqe_blocks.py
# can show that they refuse wrong outputs.  Each returns the measured share of its bound and raises AssertionError.
ALPHA = [c + 18 * s for s in (0, 1) for c in ALPHA_COLUMNS]
OTHER = [c for c in range(NF) if c not in ALPHA]
PLANE2_BOUND = 255 * 2.0 ** -44            # derived in test_gpu_niqe.test_planes
FEATURE_BOUND = 1e-10


def score_bound(rfit):
    """|q2 - q2_restatement| may reach 64 cond(Sigma) 2.2e-16 q2 (absolute).

    Where the 64 comes from: q2 = d' Sigma^-1 d moves by at most cond(Sigma) |dSigma| / |Sigma| (to first order, plus
    twice the relative error of d, which the factor cond dwarfs) when Sigma is perturbed.  Two correct fp64 fits differ
    in Sigma by the rounding of their sums and of their solves: a 36 x 36 factorisation and substitution has a backward
    error of about 36 u in the worst case, and a sum of n products in some order errs by n u in the worst case and by
    sqrt(n) u typically.  64 u allows the solve's 36 u and 28 u for the sums: a worst-case allowance up to 28 rows, a
    typical-case one (sqrt(n) <= 28) up to 784 rows, which covers the 294 rows of a 2040 x 1356 image.  It has no
    row-count term, and needs none at the sizes tested: two orders of summation (fit against fit_by_numpy) use 1.4e-5 of
    it at 258 rows and 3.3e-6 at 8 (tests/test_cpu_niqe_blocks.py asserts less than 1 % and prints the shares), because
    the factor cond(Sigma) is reached only by a d along Sigma's smallest eigenvector, which no image's d is."""
    return 64 * rfit["cond"] * 2.2e-16 * rfit["q2"]


def compare_planes(p1, p2, want_p1):
    """Plane 1 (float32) bit-equal to want_p1; plane 2 within PLANE2_BOUND of the restatement on plane 1."""
    want_p1 = np.asarray(want_p1)
    assert p1.dtype == np.float32 and p1.shape == want_p1.shape, (p1.dtype, p1.shape, want_p1.shape)
    assert np.array_equal(p1.view(np.uint32), want_p1.astype(np.float32).view(np.uint32)), "plane 1"
    want_p2 = plane2(p1.astype(np.float64))
    assert p2.dtype == np.float64 and p2.shape == want_p2.shape, (p2.dtype, p2.shape, want_p2.shape)
    dev = float(np.abs(p2 - want_p2).max())
    assert dev <= PLANE2_BOUND, ("plane 2", dev)
    return dev / PLANE2_BOUND


def compare_features(got, want, t):
    """got against the restatement's rows `want` with their fits' rhatnorm `t`: the NaN pattern and every alpha equal
    (which rests on no t lying within 1e-9 of a midpoint: asserted), the rest within FEATURE_BOUND relative."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape, got.dtype)
    differ = np.argwhere(np.isnan(got) != np.isnan(want))
    assert differ.size == 0, ("NaN pattern at (row, column)", differ[:8].tolist())
    assert midpoint_margin(t).min() > 1e-9, "a fit within 1e-9 of a midpoint"
    differ = np.argwhere(got[:, ALPHA] != want[:, ALPHA])
    assert differ.size == 0, ("alpha at (row, fit)", differ[:8].tolist())
    a, b = got[:, OTHER], want[:, OTHER]
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    rel = float((np.abs(a - b)[ok] / np.abs(b[ok])).max())
    assert rel <= FEATURE_BOUND, ("features", rel)
    return rel / FEATURE_BOUND


def compare_score(score, rfit):
    """A score against the restatement's fit: both NaN, or q2 within score_bound."""
    if np.isnan(rfit["score"]):
        assert np.isnan(score), ("a score where the restatement has none", score)
        return 0.0
    assert np.isfinite(score), score
    dev, bound = abs(score * score - rfit["q2"]), score_bound(rfit)
    assert dev <= bound, ("score", score, rfit["score"], dev / bound)
    return dev / bound


def niqe(img, crop_border, mu_pris, cov_pris, input_order='HWC', convert_to='y'):
    p1 = plane1(img, crop_border, input_order, convert_to)
    p2 = plane2(p1)
    feat, ts = features_from_planes(p1, p2)
    out = fit(feat, mu_pris, cov_pris)
    out.update(plane1=p1, plane2=p2, feat=feat, t=ts)
    return out


def calculate_niqe(img, crop_border, input_order='HWC', convert_to='y', niqe_pris_params=None, **kwargs):
    return niqe(img, crop_border, niqe_pris_params['mu_pris_param'], niqe_pris_params['cov_pris_param'], input_order,
                convert_to)['score']
