"""fp64 restatement of the ragged degradation kernels (ssl_amd/csrc/ssg_blindsr.hip, include/ssg_hip.h section (T)),
written from the rules of the header, and the first-order bounds an fp32 evaluation is held to.  numpy only, nothing of
ssl_amd.  Images are planar (C, h, w).

conv     scipy.ndimage.convolve(img, k[:, :, None], mode='mirror')[0::s, 0::s]: out[y, x] = sum_ij k[i, j] in[fold(y s + r -
         i), fold(x s + r - j)], fold the reflection of period 2 (n - 1).
         Bound: the kernel rounds every tap to fp32 (u |k|) and adds one fmaf per tap (the partial sums never exceed
         S = sum |k_ij| |x_ij|; k^2 of them): (k^2 + 1) u S; CONV_U = k^2 + 2 leaves one for the restatement's own sum.
resize   per axis a list of (source index, weight) per destination index (`axis_taps`), out = sum_y wy sum_x wx in[iy, ix].
         OpenCV forms the coordinate in fp64, casts it to float and computes the WEIGHTS IN FLOAT; that is part of the
         rule, so the restatement forms the same float weights operation by operation (numpy float32, no fused
         operation) and sums in fp64.  Bound: a source value passes its product with wx, at most Tx - 1 additions of the
         row, the product with wy and at most Ty - 1 additions of the rows: (Tx + Ty) u S, S = sum |wy| |wx| |x|; the
         integer box adds its sy sx values first and multiplies by float(1 / (sy sx)) (one rounding of the constant, one
         of the product): (sy sx + 1) u S.
         Against an oracle that forms the coordinate or the weights differently (torch's interpolate: fp64 throughout,
         or float throughout), `coordinate_slack` adds what a perturbation df of the fraction moves the result by.
noise    numpy float32 transcriptions of add_Gaussian_noise, add_speckle_noise and add_Poisson_noise given their
         fields: the kernels are held to them bit for bit.
"""
import numpy as np

U = 2.0 ** -24
LINEAR, CUBIC, AREA = 1, 2, 3
F32 = np.float32


def fold(i, n):
    p = 2 * (n - 1)
    if p == 0:
        return np.zeros_like(i)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


# ------------------------------------------------------------------ conv ----
def conv_u(k):
    return k * k + 2


def conv(x, kernel, stride=1, clip=False):
    """(result, bound) in fp64 of planar x (C, h, w) and a (k, k) kernel"""
    x = np.asarray(x, dtype=np.float64)
    kernel = np.asarray(kernel, dtype=np.float64)
    k = kernel.shape[0]
    r = k // 2
    C, h, w = x.shape
    oy, ox = np.arange(0, h, stride), np.arange(0, w, stride)
    out = np.zeros((C, len(oy), len(ox)))
    mag = np.zeros_like(out)
    for i in range(k):
        yy = fold(oy + r - i, h)
        for j in range(k):
            xx = fold(ox + r - j, w)
            g = x[:, yy][:, :, xx]
            out += kernel[i, j] * g
            mag += abs(kernel[i, j]) * np.abs(g)
    if clip:
        out = np.clip(out, 0.0, 1.0)
    return out, conv_u(k) * U * mag


# ------------------------------------------------------------------ resize ----
def _cubic_weights(f):
    """OpenCV's interpolateCubic in float, A = -0.75, operation by operation"""
    A, one = F32(-0.75), F32(1)
    t = f + one
    w0 = ((A * t - F32(5) * A) * t + F32(8) * A) * t - F32(4) * A
    w1 = ((A + F32(2)) * f - (A + F32(3))) * f * f + one
    g = one - f
    w2 = ((A + F32(2)) * g - (A + F32(3))) * g * g + one
    w3 = one - w0 - w1 - w2
    return np.stack([w0, w1, w2, w3], 1)


def axis_taps(n, m, mode):
    """(indices (m, T) int64, weights (m, T) float32 as OpenCV forms them, zero-padded) of one axis n -> m"""
    d = np.arange(m, dtype=np.float64)
    s = np.float64(n) / np.float64(m)
    if mode == "box":
        q = n // m
        return (np.arange(m)[:, None] * q + np.arange(q)[None, :]), np.full((m, q), 1.0 / q)   # (weights: see resize)
    if mode == "table":
        f1 = d * s
        f2 = f1 + s
        cw = np.minimum(s, n - f1)
        a, b = np.ceil(f1).astype(np.int64), np.floor(f2).astype(np.int64)
        b = np.minimum(b, n - 1)
        a = np.minimum(a, b)
        T = int((b - a).max()) + 2
        idx, wgt = np.zeros((m, T), np.int64), np.zeros((m, T), F32)
        for q in range(m):
            ii, ww = [], []
            if a[q] - f1[q] > 1e-3:
                ii.append(a[q] - 1), ww.append(F32((a[q] - f1[q]) / cw[q]))
            for sx in range(a[q], b[q]):
                ii.append(sx), ww.append(F32(1.0 / cw[q]))
            if f2[q] - b[q] > 1e-3:
                ii.append(b[q]), ww.append(F32(min(min(f2[q] - b[q], 1.0), cw[q]) / cw[q]))
            idx[q, :len(ii)], wgt[q, :len(ii)] = ii, ww
        return np.clip(idx, 0, n - 1), wgt
    if mode == "area_linear":
        sx = np.floor(d * s).astype(np.int64)
        f = ((d + 1) - (sx + 1) / s).astype(F32)
        f = np.where(f <= 0, F32(0), f - np.floor(f)).astype(F32)
    else:
        f = ((d + 0.5) * s - 0.5).astype(F32)
        sx = np.floor(f).astype(np.int64)
        f = (f - sx.astype(F32)).astype(F32)
    if mode == "cubic":
        return np.clip(sx[:, None] + np.arange(-1, 3)[None, :], 0, n - 1), _cubic_weights(f)
    low, high = sx < 0, sx >= n - 1
    f = np.where(low | high, F32(0), f).astype(F32)
    sx = np.where(low, 0, np.where(high, n - 1, sx))
    return np.stack([sx, np.minimum(sx + 1, n - 1)], 1), np.stack([F32(1) - f, f], 1).astype(F32)


def resize(x, oh, ow, interp, clip=False):
    """(result, bound) in fp64 of cv2.resize's rules on planar x (C, h, w)"""
    x = np.asarray(x, dtype=np.float64)
    C, h, w = x.shape
    reduce_both = h >= oh and w >= ow
    box = interp == AREA and reduce_both and h % oh == 0 and w % ow == 0
    if interp == AREA and reduce_both:
        my = mx = "box" if box else "table"
    else:
        my = mx = {LINEAR: "linear", CUBIC: "cubic", AREA: "area_linear"}[interp]
    iy, wy = axis_taps(h, oh, my)
    ix, wx = axis_taps(w, ow, mx)
    wy, wx = wy.astype(np.float64), wx.astype(np.float64)
    g = x[:, iy][:, :, :, ix]                                   # (C, oh, Ty, ow, Tx)
    out = np.einsum("cytxs,yt,xs->cyx", g, wy, wx)
    mag = np.einsum("cytxs,yt,xs->cyx", np.abs(g), np.abs(wy), np.abs(wx))
    if box:
        area = (h // oh) * (w // ow)
        scale = np.float64(F32(1.0 / area))                     # the kernel's constant
        out, mag = out * area * scale, mag * area * scale
        rounds = area + 1
    else:
        rounds = wy.shape[1] + wx.shape[1]
    if clip:
        out = np.clip(out, 0.0, 1.0)
    return out, rounds * U * mag


def coordinate_slack(x, oh, ow, interp, df_y, df_x):
    """What a perturbation of the fraction by df (per axis) moves a LINEAR or CUBIC result by at most, to first order:
    |dw / df| <= 1 for the two linear weights and <= 1.5 for the cubic ones (the derivative of the A = -0.75 kernel), on
    the taps' magnitudes."""
    x = np.asarray(x, dtype=np.float64)
    C, h, w = x.shape
    mode = {LINEAR: "linear", CUBIC: "cubic"}[interp]
    iy, wy = axis_taps(h, oh, mode)
    ix, wx = axis_taps(w, ow, mode)
    g = np.abs(x[:, iy][:, :, :, ix])
    lip = 1.0 if interp == LINEAR else 1.5
    ones_y, ones_x = np.ones_like(wy, dtype=np.float64), np.ones_like(wx, dtype=np.float64)
    return lip * (df_y * np.einsum("cytxs,yt,xs->cyx", g, ones_y, np.abs(wx).astype(np.float64)) +
                  df_x * np.einsum("cytxs,yt,xs->cyx", g, np.abs(wy).astype(np.float64), ones_x))


# ------------------------------------------------------------------ noise: numpy float32, the reference's expressions ----
def _clip(v):
    return np.clip(v, 0.0, 1.0)


def correlated(z, M):
    """n_c = (M[c][0] z_0 + M[c][1] z_1) + M[c][2] z_2 in float32: the kernel's order"""
    z, M = np.asarray(z, F32), np.asarray(M, dtype=np.float64).astype(F32)
    return np.stack([(M[c, 0] * z[0] + M[c, 1] * z[1]) + M[c, 2] * z[2] for c in range(3)]).astype(F32)


def gaussian(x, field, scale=1.0, mode="color", matrix=None, speckle=False, clip=True):
    """add_Gaussian_noise / add_speckle_noise (utils_blindsr.py:363-395) given the field: float32 (C, h, w) in and out.
    field: (C, h, w) for 'color' and 'corr' (a standard-normal field under `matrix`), (1, h, w) for 'gray'."""
    x, field = np.asarray(x, F32), np.asarray(field, F32)
    n = correlated(field, matrix) if mode == "corr" else field
    n = (n * F32(scale)).astype(F32)
    if speckle:
        x = _clip(x)
        y = x + x * n
    else:
        y = x + n
    return (_clip(y) if clip else y).astype(F32)


def quantise(x):
    return (np.clip((np.asarray(x, F32) * F32(255.0)).round(), 0, 255) / F32(255.)).astype(F32)


def luminance(q):
    """np.dot(img[..., :3], [0.299, 0.587, 0.114]) on the float32 image, as the reference calls it: the image promoted to
    fp64 and numpy's own dot, whose sum is the fused chain fma(q_2, c_2, fma(q_1, c_1, q_0 c_0)) (`luminance_fma` states
    it exactly; tests/test_cpu_blindsr.py holds the two equal)"""
    q = np.asarray(q)
    return np.dot(np.moveaxis(q, 0, -1)[..., :3], [0.299, 0.587, 0.114])


def luminance_fma(q):
    """the chain the kernel forms, evaluated exactly (rationals), rounded once per fused operation"""
    from fractions import Fraction
    q = np.asarray(q, dtype=np.float64)
    c = [0.299, 0.587, 0.114]
    fma = lambda a, b, s: float(Fraction(a) * Fraction(b) + Fraction(s))
    flat = q.reshape(3, -1)
    out = [fma(flat[2, i], c[2], fma(flat[1, i], c[1], flat[0, i] * c[0])) for i in range(flat.shape[1])]
    return np.array(out).reshape(q.shape[1:])


def gray_level(x):
    g = luminance(quantise(x))
    return np.clip((g * 255.0).round(), 0, 255) / 255.


def poisson_rates(x, vals, gray):
    """what np.random.poisson is drawn from (:402, :406), as the kernel writes it: float32"""
    if gray:
        return (gray_level(x) * np.float64(F32(vals)))[None].astype(F32)
    return (quantise(x) * F32(vals)).astype(F32)


def poisson(x, draw, vals, gray, clip=True):
    """add_Poisson_noise (:398-409) given the draw (float32, (C, h, w), or (1, h, w) for the gray form)"""
    draw, v = np.asarray(draw, F32), F32(vals)
    if gray:
        noise = (draw[0] / v).astype(np.float64) - gray_level(x)
        y = (quantise(x).astype(np.float64) + noise[None]).astype(F32)
    else:
        y = (draw / v).astype(F32)
    return (_clip(y) if clip else y).astype(F32)


# ------------------------------------------------------------------ one stage of a program ----
def stage(st, x, field=None):
    """(result fp64, bound | None for a bit-exact stage) of a conv / resize / noise / poisson Stage on planar fp32 x"""
    p = st.params
    if st.kind == "conv":
        return conv(x, p["kernel"], p["stride"], p["clip"])
    if st.kind == "resize":
        return resize(x, st.oh, st.ow, p["interp"], p["clip"])
    if st.kind == "noise":
        family, mode = p["op"].split("_")
        return gaussian(x, field, p["scale"], mode.lower(), p.get("matrix"), family == "SPECKLE", p["clip"]), None
    if st.kind == "poisson":
        return poisson(x, field, p["vals"], p["gray"]), None
    raise ValueError(st.kind)
