"""numpy fp64 restatement of the validation metrics' contract (include/ssg_hip.h section (J)): basicsr's tensor2img
quantisation, crop, to_y_channel / bgr2ycbcr(y_only=True), calculate_psnr and calculate_ssim, with the 'valid' 11 x 11
Gaussian moments summed both as one 2-D window (filter2D's order) and separably (the kernel's order), and an error bound
for SSIM that is derived, not fitted.

Images here are uint8 (H,W,C) arrays in BGR order, as the reference's metric functions receive them."""
import numpy as np

U = 2.0 ** -53
C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2
KSIZE, RADIUS = 11, 5


def taps():
    i = np.arange(KSIZE, dtype=np.float64) - RADIUS
    g = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def quantise(x):
    """tensor2img on a float (C,H,W) RGB tensor given as an array: clamp, * 255.0f in fp32, round half to even, uint8,
    BGR, (H,W,C)."""
    x = np.clip(np.asarray(x).astype(np.float32), np.float32(0), np.float32(1))
    q = np.rint(x * np.float32(255.0)).astype(np.uint8)
    return np.ascontiguousarray(q[::-1].transpose(1, 2, 0))


def crop(q, border):
    return q[border:q.shape[0] - border, border:q.shape[1] - border] if border else q


def planes(q, border=0, y_channel=False):
    """The float32 planes (P,Hc,Wc) the metrics are computed on."""
    q = crop(np.asarray(q), border)
    if q.ndim == 2:
        q = q[..., None]
    assert q.dtype == np.uint8
    if not y_channel:
        return np.ascontiguousarray(q.transpose(2, 0, 1)).astype(np.float32)
    v = q.astype(np.float32) / np.float32(255.0)
    if q.shape[2] == 3:
        w = v.astype(np.float64)
        t = ((24.966 * w[..., 0] + 128.553 * w[..., 1]) + 65.481 * w[..., 2]) + 16.0
        v = (t / 255.0).astype(np.float32)[..., None]
    return np.ascontiguousarray((v * np.float32(255.0)).transpose(2, 0, 1))


def y_by_dot(q):
    """to_y_channel's own arithmetic on (..., 3) uint8 BGR, np.dot included (metric_util.py:32-45, color_util.py:60-67,
    129-183)."""
    img = q.astype(np.float32) / 255.
    out = np.dot(img, [24.966, 128.553, 65.481]) + 16.0
    out /= 255.
    return out.astype(np.float32) * 255.


def squared_differences(pa, pb):
    """(the fp64 sum as the reference's np.mean forms it times N, the exact integer sum or None, N)"""
    d = pa.astype(np.float64) - pb.astype(np.float64)
    n = d.size
    exact = None
    if np.all(pa == np.rint(pa)) and np.all(pb == np.rint(pb)):
        di = pa.astype(np.int64) - pb.astype(np.int64)
        exact = int((di * di).sum())
    return float(np.mean(d ** 2)) * n, exact, n


def psnr(pa, pb):
    d = pa.astype(np.float64) - pb.astype(np.float64)
    mse = np.mean(d ** 2)
    return float("inf") if mse == 0 else float(10. * np.log10(255. * 255. / mse))


def _moments_2d(x, w2):
    hm, wm = x.shape[0] - 2 * RADIUS, x.shape[1] - 2 * RADIUS
    acc = np.zeros((hm, wm))
    for i in range(KSIZE):
        for j in range(KSIZE):
            acc += w2[i, j] * x[i:i + hm, j:j + wm]
    return acc


def _moments_sep(x, g):
    hm, wm = x.shape[0] - 2 * RADIUS, x.shape[1] - 2 * RADIUS
    row = np.zeros((x.shape[0], wm))
    for j in range(KSIZE):
        row += g[j] * x[:, j:j + wm]
    acc = np.zeros((hm, wm))
    for i in range(KSIZE):
        acc += g[i] * row[i:i + hm]
    return acc


def _five(x, y, order):
    g = taps()
    if order == "2d":
        w2 = np.outer(g, g)
        f = lambda z: _moments_2d(z, w2)
    else:
        f = lambda z: _moments_sep(z, g)
    return f(x), f(y), f(x * x), f(y * y), f(x * y)


def ssim_map(x, y, order="2d"):
    """_ssim's map of one fp64 plane pair (psnr_ssim.py:170-198)."""
    mu1, mu2, exx, eyy, exy = _five(x, y, order)
    mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1, s2, s12 = exx - mu1_sq, eyy - mu2_sq, exy - mu12
    return ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def ssim(pa, pb, order="2d"):
    """calculate_ssim on planes (P,Hc,Wc): the mean over each plane's map, then over the planes."""
    return float(np.array([ssim_map(a.astype(np.float64), b.astype(np.float64), order).mean()
                           for a, b in zip(pa, pb)]).mean())


def ssim_bound(pa, pb):
    """A bound on |S' - S''| for any two fp64 evaluations S', S'' of calculate_ssim on these planes that differ only in
    the order of their sums (2-D window or separable passes, any order of the mean).

    The planes are non-negative, so each moment is a sum of 121 non-negative terms w_ij z_ij; formed in any order (a
    separable pass rounds its 11-term rows and then 11 products and sums of them, fewer operations per path than the 121
    of the 2-D window), its relative error is at most gamma = 124 u, u = 2^-53.  The absolute errors are carried
    through _ssim's expression operation by operation (each operation adds u |result|): the squares and the product of
    the means, the differences E[x^2] - mu^2 (where the moments' errors do NOT shrink with the difference: this is the
    cancellation of a flat plane), the two numerator and denominator factors, their products and the quotient, with the
    actual denominator less its own error (it is at least c1 c2, the variances being non-negative).  One evaluation is
    within e of the exact map value, two evaluations within 2 e of each other; the mean of n map values in any order adds
    (n + 3) u mean|map| per evaluation."""
    gam = 124 * U
    total, count = 0.0, 0
    for a, b in zip(pa, pb):
        x, y = a.astype(np.float64), b.astype(np.float64)
        mu1, mu2, exx, eyy, exy = _five(x, y, "2d")
        e1, e2, exx_e, eyy_e, exy_e = gam * mu1, gam * mu2, gam * exx, gam * eyy, gam * exy
        mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
        mu1_sq_e = 2 * mu1 * e1 + e1 ** 2 + U * mu1_sq
        mu2_sq_e = 2 * mu2 * e2 + e2 ** 2 + U * mu2_sq
        mu12_e = mu1 * e2 + mu2 * e1 + e1 * e2 + U * mu12
        s1, s2, s12 = exx - mu1_sq, eyy - mu2_sq, exy - mu12
        s1_e = exx_e + mu1_sq_e + U * np.abs(s1)
        s2_e = eyy_e + mu2_sq_e + U * np.abs(s2)
        s12_e = exy_e + mu12_e + U * np.abs(s12)
        a1, a2 = 2 * mu12 + C1, 2 * s12 + C2
        b1, b2 = mu1_sq + mu2_sq + C1, s1 + s2 + C2
        a1_e = 2 * mu12_e + U * np.abs(a1)
        a2_e = 2 * s12_e + U * np.abs(a2)
        b1_e = mu1_sq_e + mu2_sq_e + 2 * U * np.abs(b1)
        b2_e = s1_e + s2_e + 2 * U * np.abs(b2)
        num, den = a1 * a2, b1 * b2
        num_e = np.abs(a1) * a2_e + np.abs(a2) * a1_e + a1_e * a2_e + U * np.abs(num)
        den_e = np.abs(b1) * b2_e + np.abs(b2) * b1_e + b1_e * b2_e + U * np.abs(den)
        m = num / den
        assert np.all(den - den_e > 0)
        m_e = (num_e + np.abs(m) * den_e) / (den - den_e) + U * np.abs(m)
        n = m.size
        total += float((2 * m_e).mean() + 2 * (n + 3) * U * np.abs(m).mean())
        count += 1
    return total / count


def metrics(a, b, border=0, y_channel=False):
    """Everything at once for two uint8 (H,W,C) BGR images."""
    pa, pb = planes(a, border, y_channel), planes(b, border, y_channel)
    sq, exact, n = squared_differences(pa, pb)
    return dict(planes_a=pa, planes_b=pb, psnr=psnr(pa, pb), ssim=ssim(pa, pb, "2d"), ssim_sep=ssim(pa, pb, "sep"),
                sq_sum=sq, sq_exact=exact, n=n, bound=ssim_bound(pa, pb))


# ---- the reference's two public functions on numpy arrays (what the offline tool's CPU test patches in) ----
def _reorder(img, input_order):
    if input_order not in ['HWC', 'CHW']:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    if input_order == 'CHW':
        img = img.transpose(1, 2, 0)
    return np.ascontiguousarray(img).astype(np.uint8)


def calculate_psnr(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    assert img.shape == img2.shape, (f'Image shapes are different: {img.shape}, {img2.shape}.')
    a, b = _reorder(img, input_order), _reorder(img2, input_order)
    return psnr(planes(a, crop_border, test_y_channel), planes(b, crop_border, test_y_channel))


def calculate_ssim(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    assert img.shape == img2.shape, (f'Image shapes are different: {img.shape}, {img2.shape}.')
    a, b = _reorder(img, input_order), _reorder(img2, input_order)
    return ssim(planes(a, crop_border, test_y_channel), planes(b, crop_border, test_y_channel))
