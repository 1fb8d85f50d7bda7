"""fp64 restatement of the SSIM criterion's contract (ssl_amd/csrc/ssg_ssim.hip, include/ssg_hip.h section (M)) with its
analytic gradient, and the per-element error bound an fp32 evaluation of it is held to.  torch on the CPU, nothing of
ssl_amd.

Contract: w = fl32(g_i g_j), g = e / sum(e) in fp32, e_i = fl32(exp(-(i - K//2)^2 / 4.5)); `*` the per-channel 'same'
convolution with zero padding K//2;

    mx = w*x  my = w*y  exx = w*x^2  eyy = w*y^2  exy = w*xy
    A1 = 2 mx my + C1   A2 = 2 (exy - mx my) + C2   B1 = mx^2 + my^2 + C1   B2 = (exx - mx^2) + (eyy - my^2) + C2
    S = A1 A2 / (B1 B2),  C1 = 0.01^2, C2 = 0.03^2
    P = dS/dmx = 2 my (A2 - A1) / (B1 B2) - 2 mx S (1/B1 - 1/B2),  Q = dS/dexx = -S / B2,  R = dS/dexy = 2 A1 / (B1 B2)
    L = sum_p c_p S_p:   dL/dx = w*(c P) + 2 x (w*(c Q)) + y (w*(c R));  dL/dy the same with the roles swapped.

The bound (first order, u = 2^-24), term by term:
  moments   a 121-term fp32 product sum, whatever its order, is off by at most K_ROUND u (w*|term|): 120 additions,
            the product w t, the term itself (x^2, xy) and the tap (the kernels' g_i g_j against the table's
            fl32(g_i g_j)) -- K_ROUND = 123 roundings on the path of one term.
  nodes     A1, A2, B1, B2 are formed from the moments with one rounding per operation; each rounding is relative to
            the value it rounds, so the node is off by u times the magnitudes listed in node_roundings().
  map       S, P, Q, R depend on the five moments and four nodes AT THE SAME PIXEL, so fp64 autograd of the restatement
            gives their partials; the errors above are pushed through their absolute values, plus POINT_ROUND u times
            the magnitude of the addends the value is accumulated from (S: itself; Q, R: themselves; P: the four
            addends 2 my A2 D, 2 my A1 D, 2 mx S / B1, 2 mx S / B2 that an autograd replay accumulates separately).
            POINT_ROUND = 12: no addend's product chain has more than ten roundings (S has three, 1 / (B1 B2) two), and
            at most two additions accumulate them.
  gradient  the three output convolutions carry the map's errors through |c|, |x|, |y|, add their own K_ROUND u on
            w*|c P|, 2 |x| w*|c Q| and |y| w*|c R|, and OUT_ROUND = 6 more roundings on the three terms' magnitudes (the
            coefficient c, the products with 2x and y, the accumulation).
  loss      the mean of the map's errors, plus the summation: a cascade in blocks of 16 (torch's CPU reduction) puts at
            most 4 ceil(log2 N) + 64 additions on one element's path; the kernels sum in fp64 and round once.

This is a worst-case envelope: the reference's own fp32 results and the kernels use a few per cent of it at most.  It
catches structural errors; changes of a few ulp are the business of the bit-for-bit tests in test_gpu_ssim.py.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
K_ROUND = 123
POINT_ROUND = 12
OUT_ROUND = 6
C1, C2 = 0.01 ** 2, 0.03 ** 2
D = torch.float64


def gaussian(window_size, sigma=1.5):
    """The contract's fp32 taps: fp64 exponentials rounded once, normalised in fp32."""
    offset = torch.arange(window_size, dtype=D) - window_size // 2
    e = torch.exp(-offset.square() / (2.0 * sigma * sigma)).to(torch.float32)
    return e / e.sum()


def window(window_size):
    """The reference's fp32 window (K, K), as fp64."""
    g = gaussian(window_size)
    return torch.outer(g, g).to(D)


def _t(a):
    return torch.as_tensor(a).detach().to(D)


def conv(t, w):
    c = t.shape[1]
    return F.conv2d(t, w.expand(c, 1, *w.shape).contiguous(), padding=w.shape[0] // 2, groups=c)


def moments(x, y, w):
    return [conv(x, w), conv(y, w), conv(x * x, w), conv(y * y, w), conv(x * y, w)]


def nodes(m):
    mx, my, exx, eyy, exy = m
    return [2 * mx * my + C1, 2 * (exy - mx * my) + C2, mx * mx + my * my + C1, (exx - mx * mx) + (eyy - my * my) + C2]


def node_roundings(m):
    """What one unit roundoff at every operation that forms A1, A2, B1, B2 amounts to."""
    mx, my, exx, eyy, exy = m
    A1, A2, B1, B2 = nodes(m)
    mxy, mxx, myy = (mx * my).abs(), mx * mx, my * my
    return [2 * mxy + A1.abs(),
            2 * mxy + 2 * (exy - mx * my).abs() + A2.abs(),
            2 * (mxx + myy) + B1.abs(),
            (mxx + myy) + 2 * ((exx - mxx).abs() + (eyy - myy).abs()) + B2.abs()]


def point(m, n):
    """S, P (with respect to mx), P' (with respect to my), Q, R from the moments and the nodes."""
    mx, my = m[0], m[1]
    A1, A2, B1, B2 = n
    Dn = 1 / (B1 * B2)
    S = A1 * A2 * Dn
    P = 2 * my * (A2 - A1) * Dn - 2 * mx * S * (1 / B1 - 1 / B2)
    Py = 2 * mx * (A2 - A1) * Dn - 2 * my * S * (1 / B1 - 1 / B2)
    return S, P, Py, -S / B2, 2 * A1 * Dn


def _coef(c, shape):
    B = shape[0]
    if c is None:
        return torch.full((B, 1, 1, 1), 1.0 / (shape[0] * shape[1] * shape[2] * shape[3]), dtype=D)
    c = _t(c)
    return c.reshape(()).expand(B).reshape(B, 1, 1, 1) if c.numel() == 1 else c.reshape(B, 1, 1, 1)


def ssim_map(x, y, window_size=11):
    x, y = _t(x), _t(y)
    m = moments(x, y, window(window_size))
    return point(m, nodes(m))[0]


def ssim(x, y, window_size=11, size_average=True):
    S = ssim_map(x, y, window_size)
    return S.mean() if size_average else S.mean(dim=(1, 2, 3))


def gradients(x, y, window_size=11, coef=None):
    """(dL/dx, dL/dy) of L = sum_p c_p S_p; c per image (B,) or a scalar, default 1 / (B C H W): the scalar mean."""
    x, y = _t(x), _t(y)
    w = window(window_size)
    c = _coef(coef, x.shape)
    m = moments(x, y, w)
    S, P, Py, Q, R = point(m, nodes(m))
    cq, cr = conv(c * Q, w), conv(c * R, w)
    return conv(c * P, w) + 2 * x * cq + y * cr, conv(c * Py, w) + 2 * y * cq + x * cr


def term_scale(x, y, window_size=11, coef=None):
    """max over the elements of |w*(cP)| + 2 |x| |w*(cQ)| + |y| |w*(cR)|: the size of the gradient's three terms.  Where
    x == y they cancel to zero analytically and max|grad| is rounding noise; this is what a gap is measured against
    there."""
    x, y = _t(x), _t(y)
    w = window(window_size)
    c = _coef(coef, x.shape)
    m = moments(x, y, w)
    S, P, Py, Q, R = point(m, nodes(m))
    return float((conv(c * P, w).abs() + 2 * x.abs() * conv(c * Q, w).abs() + y.abs() * conv(c * R, w).abs()).max())


def bounds(x, y, window_size=11, coef=None):
    """(loss_bound (B,): on each image's mean of S -- the scalar mean's bound is their mean;
    grad_x bound, grad_y bound: per element, for L = sum_p c_p S_p).  See the module docstring."""
    x, y = _t(x), _t(y)
    w = window(window_size)
    c = _coef(coef, x.shape).abs()
    m = moments(x, y, w)
    dm = [K_ROUND * U * t for t in moments(x.abs(), y.abs(), w)]          # w*|x|, w*|y|, w*x^2, w*y^2, w*|xy|
    dn = [U * t for t in node_roundings(m)]
    leaves = [t.clone().requires_grad_(True) for t in m]
    eps = [torch.zeros_like(m[0], requires_grad=True) for _ in range(4)]
    n = [a + e for a, e in zip(nodes(leaves), eps)]
    S, P, Py, Q, R = point(leaves, n)
    A1, A2, B1, B2 = [t.detach() for t in n]
    Sd, Dn, mx, my = S.detach(), 1 / (B1 * B2), m[0], m[1]
    mag = {"S": Sd.abs(), "Q": Q.detach().abs(), "R": R.detach().abs(),
           "P": (2 * my * Dn).abs() * (A2.abs() + A1.abs()) + (2 * mx * Sd).abs() * (1 / B1.abs() + 1 / B2.abs()),
           "Py": (2 * mx * Dn).abs() * (A2.abs() + A1.abs()) + (2 * my * Sd).abs() * (1 / B1.abs() + 1 / B2.abs())}
    err = {}
    for name, v in (("S", S), ("P", P), ("Py", Py), ("Q", Q), ("R", R)):
        part = torch.autograd.grad(v.sum(), leaves + eps, retain_graph=True, allow_unused=True)
        err[name] = sum(p.abs() * d for p, d in zip(part, dm + dn) if p is not None) + POINT_ROUND * U * mag[name]
    N = x.shape[1] * x.shape[2] * x.shape[3]
    n_sum = 4 * math.ceil(math.log2(max(N * x.shape[0], 2))) + 64
    loss = (err["S"] + n_sum * U * mag["S"]).mean(dim=(1, 2, 3))
    ax, ay = x.abs(), y.abs()

    def grad_bound(p, a, b):
        # a: the image the gradient is taken for (2 a w*(cQ)), b the other (b w*(cR))
        carried = conv(c * err[p], w) + 2 * a * conv(c * err["Q"], w) + b * conv(c * err["R"], w)
        own = conv(c * mag[p], w) + 2 * a * conv(c * mag["Q"], w) + b * conv(c * mag["R"], w)
        return carried + (K_ROUND + OUT_ROUND) * U * own

    return loss, grad_bound("P", ax, ay), grad_bound("Py", ay, ax)


def share(got, want, bound):
    """The largest share of the bound a result uses (0 / 0 counts as 0; anything / 0 as inf)."""
    d = (_t(got) - _t(want)).abs()
    b = _t(bound).expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    return float(r.max())


# ---- contents (shared by the fixture generator and the GPU tests; seeded) ----
CONTENTS = ("uniform01", "uniform11", "smooth", "flat_noise", "step", "equal", "zero")


def content(name, shape, seed=0):
    """An (x, y) fp32 pair of `shape`, |values| <= 1."""
    g = torch.Generator().manual_seed(1000 + seed)
    B, C, H, W = shape
    rnd = lambda: torch.rand(shape, generator=g, dtype=D)     # noqa: E731
    if name == "uniform01":
        x, y = rnd(), rnd()
    elif name == "uniform11":
        x, y = 2 * rnd() - 1, 2 * rnd() - 1
    elif name == "smooth":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=D), torch.arange(W, dtype=D), indexing="ij")
        x = (0.5 + 0.4 * torch.sin(xx / 7.0 + 0.3) * torch.cos(yy / 5.0)).expand(shape).clone()
        y = (0.5 + 0.35 * torch.sin(xx / 7.0 + 0.5) * torch.cos(yy / 5.5 + 0.2)).expand(shape).clone()
        x, y = x + 0.02 * rnd(), y + 0.02 * rnd()
    elif name == "flat_noise":
        x, y = 0.5 + 1e-3 * (2 * rnd() - 1), 0.5 + 1e-3 * (2 * rnd() - 1)
    elif name == "step":
        x = torch.zeros(shape, dtype=D)
        x[..., W // 2:] = 1.0
        y = torch.zeros(shape, dtype=D)
        y[..., H // 2:, :] = 0.9
        y = y + 0.05 * rnd()
    elif name == "equal":
        x = rnd()
        y = x.clone()
    elif name == "zero":
        x, y = torch.zeros(shape, dtype=D), torch.zeros(shape, dtype=D)
    else:
        raise KeyError(name)
    return x.to(torch.float32), y.to(torch.float32)
