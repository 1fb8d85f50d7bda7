"""A numpy restatement of the Diffusion fork's colour correction (scripts/wavelet_color_fix.py), in fp64 or in the
dtype of its input, and the two error bounds the kernels of ssl_amd/csrc/ssg_colorfix.hip are held to.

The restatement keeps the reference's structure: the nine-term 3 x 3 sum on clamped indices (replicate padding by
`radius`, then a convolution dilated by `radius`, is a gather at clamped coordinates), the per-level accumulation of
`high`, two decompositions per reconstruction, torch's unbiased variance.  `wavelet_reconstruction_linear` is the form the
kernel uses, content + low(style - content).

Arrays are (B,C,H,W); `dtype=None` keeps the input's dtype, so a float32 input is evaluated in float32 throughout."""
import warnings

import numpy as np

U = 2.0 ** -24                      # the unit roundoff of float32
WEIGHTS = ((0.0625, 0.125, 0.0625), (0.125, 0.25, 0.125), (0.0625, 0.125, 0.0625))
EPS = 1e-5


def _as(a, dtype):
    a = np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def wavelet_blur(image, radius, dtype=None):
    x = _as(image, dtype)
    H, W = x.shape[-2:]
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros_like(x)
    for i, dy in enumerate((-radius, 0, radius)):
        yy = np.clip(ys + dy, 0, H - 1)
        for j, dx in enumerate((-radius, 0, radius)):
            xx = np.clip(xs + dx, 0, W - 1)
            out += x.dtype.type(WEIGHTS[i][j]) * x[..., yy[:, None], xx[None, :]]
    return out


def wavelet_decomposition(image, levels=5, dtype=None):
    x = _as(image, dtype)
    high = np.zeros_like(x)
    low = x
    for i in range(levels):
        low = wavelet_blur(x, 2 ** i)
        high += x - low
        x = low
    return high, low


def wavelet_reconstruction(content, style, levels=5, dtype=None):
    high, _ = wavelet_decomposition(content, levels, dtype)
    _, low = wavelet_decomposition(style, levels, dtype)
    return high + low


def wavelet_reconstruction_linear(content, style, levels=5, dtype=None):
    c, s = _as(content, dtype), _as(style, dtype)
    return c + wavelet_decomposition(s - c, levels)[1]


def calc_mean_std(feat, eps=EPS, dtype=None):
    x = _as(feat, dtype)
    b, c = x.shape[:2]
    flat = x.reshape(b, c, -1)
    with np.errstate(invalid='ignore', divide='ignore'), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        var = flat.var(axis=2, ddof=1) + x.dtype.type(eps)       # one element: 0 / 0 = NaN, as torch
    return flat.mean(axis=2).reshape(b, c, 1, 1), np.sqrt(var).reshape(b, c, 1, 1)


def adaptive_instance_normalization(content, style, dtype=None):
    c, s = _as(content, dtype), _as(style, dtype)
    sm, ss = calc_mean_std(s)
    cm, cs = calc_mean_std(c)
    return (c - cm) / cs * ss + sm


def unit(x):
    """clamp((x + 1) / 2, 0, 1), the step between the correction and the PNG."""
    return np.clip((np.asarray(x) + 1) / 2, 0, 1)


def to_tensor(img):
    """ToTensor of an 8-bit image array (H,W,C): / 255, HWC -> CHW, with a batch axis."""
    a = np.asarray(img)
    a = a[:, :, None] if a.ndim == 2 else a
    return (a.transpose(2, 0, 1).astype(np.float32) / np.float32(255))[None]


def to_image(t):
    """ToPILImage of a float (1,C,H,W) array clamped to [0, 1]: * 255, truncated, CHW -> HWC."""
    return (np.clip(t[0], 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)


def adain_color_fix(target, source):
    return to_image(adaptive_instance_normalization(to_tensor(target), to_tensor(source)))


def wavelet_color_fix(target, source):
    return to_image(wavelet_reconstruction(to_tensor(target), to_tensor(source)))


# ------------------------------------------------------------------------------------------------ error bounds ---
def wavelet_bound(content, style=None):
    """Per plane pair, (B,C,1,1): the largest distance of a float32 evaluation of wavelet_reconstruction (or of either
    band of wavelet_decomposition: style = None) from its fp64 value.

    With M = max(|content|, |style|) of the plane pair: every level is a convex combination of values bounded by M
    (2 M for the difference style - content), its taps are powers of two, so only its adds round -- at most 8 per level
    in the nine-term form, 4 in the separable one -- each by at most U times a magnitude <= 2 M.  The blur is
    non-expansive in the max norm, so an error made at one level reaches the output undamped at most.  Five levels
    (<= 5 x 8 x U M in the reference's form on magnitudes <= M; <= 5 x 4 x 2 U M in the separable form on the
    difference), the difference (2 U M), the final add (a result <= 3 M: 3 U M) and the reference's ten updates of
    `high` (partial sums <= 2 M: 2 x 10 x U M, of which the sample's five reach the output) stay under 64 U M."""
    m = np.abs(np.asarray(content, np.float64)).max(axis=(2, 3), keepdims=True)
    if style is not None:
        m = np.maximum(m, np.abs(np.asarray(style, np.float64)).max(axis=(2, 3), keepdims=True))
    return 64 * U * m


def adain_bound(content, style):
    """Per element, (B,C,H,W): the largest distance of an evaluation of (x - m_c) / s_c * s_s + m_s that keeps its
    statistics in fp64 and rounds them and its four operations to float32 from the fp64 value.

    Eight roundings, each relative U: four of the statistics, four of the operations.  A relative error in m_c moves the
    output by |m_c| s_s / s_c, one in m_s by |m_s|, one in s_c, s_s or any of the first three operations by
    |x - m_c| / s_c * s_s (the size of the scaled term), one in the last add by the size of the output, itself at most
    the scaled term plus |m_s|.  Each of the eight is covered by U times the sum of the three magnitudes."""
    c = np.asarray(content, np.float64)
    s = np.asarray(style, np.float64)
    cm, cs = calc_mean_std(c)
    sm, ss = calc_mean_std(s)
    return 8 * U * (np.abs(c - cm) / cs * ss + np.abs(cm) * ss / cs + np.abs(sm))


STATS_RTOL = 1e-12      # fp64 sums of at most a few million float32 values against numpy's fp64 mean / var


def byte_check(got_nhwc, value64, bound):
    """The uint8 epilogue against the fp64 value of the correction (`value64`, (B,C,H,W)) under an error `bound` on it
    (broadcastable): a byte must equal floor(255 u), u = unit(value64), unless 255 u lies within 255 bound / 2 + 255 U
    of an integer, where either neighbour may come out.  Returns (every decided byte right, the decided share);
    saturated values (u = 0 or 1 well inside the clamp) are decided."""
    v = np.asarray(value64, np.float64)
    t = 255.0 * unit(v)
    tol = np.broadcast_to(255.0 * np.asarray(bound, np.float64) / 2 + 255.0 * U, t.shape)
    want = np.floor(t)
    near = np.abs(t - np.rint(t)) <= tol
    sat = (v <= -1 - 2 * bound) | (v >= 1 + 2 * bound)
    undecided = near & ~sat
    got = np.asarray(got_nhwc).transpose(0, 3, 1, 2).astype(np.float64)
    lo, hi = np.floor(t - tol), np.floor(t + tol)
    ok = np.where(undecided, (got == np.clip(lo, 0, 255)) | (got == np.clip(hi, 0, 255)), got == want)
    return bool(ok.all()), 1.0 - float(undecided.mean())
