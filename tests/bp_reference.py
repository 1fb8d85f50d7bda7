"""The back-projection contract (ssl_amd/csrc/ssg_bp.hip, header comment) restated in torch, evaluated in fp64.

imresize on its integer-factor path is MATLAB's antialiased bicubic: Keys cubic (a = -0.5) stretched by the factor s,
K = 4s (s even) or 4s - 1 (s odd) taps, p = (K - s) // 2 pixels of symmetric padding (the edge pixel used twice), a
stride-s correlation, output sides H // s, W // s.  Used by test_cpu_bp.py (against the reference's own outputs,
tests/golden/f20_bp.npz) and by test_gpu_bp.py (against the kernels).  Everything takes and returns CPU tensors; inputs
are promoted to fp64.  The derived error bounds of the tests live here too, as functions of the input (u = 2^-24):

    forward     |y - y64|_o  <= T_o = (K^2 + 8) u A_o,  A_o = sum |w_i w_j| |x~|: a sequential fp32 sum of K^2 terms is
                within (K^2 - 1) u of the sum of the terms' magnitudes, 8 u cover the rounded taps and products
    pin         T_o + (|dk| * |x~|)_o for a tap table that differs from the closed form by dk
    loss        |L - L64|    <= lambda mean_o(T_o + 2u (|y64| + |lq|)) + 2u |L64|   (or the sum)
    gradient    |d|_h        <= 152 u (|K|^T |g|)_h: a pixel has at most 3 padded copies per axis, each inside at most
                ceil(K / s) = 4 windows, so at most 144 terms, plus 8
    ambiguous   an output with |y64 - lq| <= T_o + u |lq| has no decided sign at fp32
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GRAD_TERMS = 152


def geometry(s):
    """(K, p) of the integer factor s."""
    K = 4 * s if s % 2 == 0 else 4 * s - 1
    return K, (K - s) // 2


def keys(r, a=-0.5):
    r = r.abs()
    near = (a + 2) * r ** 3 - (a + 3) * r ** 2 + 1
    far = a * r ** 3 - 5 * a * r ** 2 + 8 * a * r - 4 * a
    return torch.where(r <= 1, near, torch.where(r <= 2, far, torch.zeros_like(r)))


def taps(s):
    """w_i = c(r_i) / sum c, r_i = (i - (K - 1) / 2) / s, fp64."""
    K, _ = geometry(s)
    c = keys((torch.arange(K, dtype=torch.float64) - (K - 1) / 2) / s)
    return c / c.sum()


def sym_index(n, p):
    """Pixel read by each of the n + 2p padded positions: -1-i -> i, n+i -> n-1-i."""
    q = torch.arange(-p, n + p)
    q = torch.where(q < 0, -1 - q, q)
    return torch.where(q >= n, 2 * n - 1 - q, q)


def _planes(x):
    x = x.double()
    return x.reshape(-1, 1, x.shape[-2], x.shape[-1])


def padded(x, s):
    """(P,1,H+2p,W+2p) of (...,H,W)."""
    _, p = geometry(s)
    x = _planes(x)
    H, W = x.shape[-2:]
    assert H >= p and W >= p, "outside the domain: the image is smaller than the padding"
    return x[..., sym_index(H, p), :][..., sym_index(W, p)]


def correlate(xp, k2, s, H, W):
    """Stride-s correlation of the padded planes with the (K,K) table k2, cropped to H // s, W // s."""
    y = F.conv2d(xp, k2[None, None].double(), stride=s)
    assert y.shape[-2:] == (H // s, W // s), (y.shape, H, W, s)
    return y


def forward(x, s, table=None):
    """y64 of (...,H,W) -> (...,H // s, W // s); `table`: a (K,K) tap table instead of the closed form."""
    w = taps(s)
    k2 = torch.outer(w, w) if table is None else table.double()
    H, W = x.shape[-2:]
    y = correlate(padded(x, s), k2, s, H, W)
    return y.reshape(tuple(x.shape[:-2]) + (H // s, W // s))


def magnitude(x, s, table=None):
    """A_o = sum |k| |x~|, the shape of forward()."""
    w = taps(s)
    k2 = (torch.outer(w, w) if table is None else table.double()).abs()
    H, W = x.shape[-2:]
    return correlate(padded(x, s).abs(), k2, s, H, W).reshape(tuple(x.shape[:-2]) + (H // s, W // s))


def forward_bound(x, s):
    K, _ = geometry(s)
    return (K * K + 8) * U * magnitude(x, s)


def pin_bound(x, s, table):
    """Bound between forward(x, s) in fp64 and an fp32 correlation with `table`."""
    w = taps(s)
    return forward_bound(x, s) + magnitude(x, s, table.double() - torch.outer(w, w))


def adjoint(g, s, H, W, absolute=False, table=None):
    """K^T g: (...,h,w) -> (...,H,W), the exact adjoint of padded() + correlate(): the transposed correlation into
    the padded domain, then every padded position added to the pixel it reads (a pixel under both mirrors collects
    all of its copies).  absolute: with |taps| (the gradient bound's magnitude); `table`: a (K,K) table instead of
    the closed form."""
    K, p = geometry(s)
    w = taps(s)
    k2 = torch.outer(w, w) if table is None else table.double()
    if absolute:
        k2 = k2.abs()
    lead = tuple(g.shape[:-2])
    g = _planes(g)
    assert g.shape[-2:] == (H // s, W // s)
    gp = F.conv_transpose2d(g, k2[None, None], stride=s)
    gp = F.pad(gp, (0, W + 2 * p - gp.shape[-1], 0, H + 2 * p - gp.shape[-2]))
    rows = torch.zeros(gp.shape[:2] + (H, gp.shape[-1]), dtype=torch.float64).index_add_(2, sym_index(H, p), gp)
    out = torch.zeros(gp.shape[:2] + (H, W), dtype=torch.float64).index_add_(3, sym_index(W, p), rows)
    return out.reshape(lead + (H, W))


def backward_bound(g, s, H, W):
    return GRAD_TERMS * U * adjoint(g.double().abs(), s, H, W, absolute=True)


def loss_and_grad(x, lq, s, loss_weight=1.0, reduction='mean'):
    """(L64, dL/dx, y64, g): g = lambda / M sgn(y64 - lq) is the upstream the gradient is the adjoint of."""
    y = forward(x, s)
    d = y - lq.double()
    scale = loss_weight / d.numel() if reduction == 'mean' else loss_weight
    g = scale * torch.sign(d)
    H, W = x.shape[-2:]
    return scale * d.abs().sum(), adjoint(g, s, H, W), y, g


def loss_bound(x, lq, s, y64, loss64, loss_weight=1.0, reduction='mean'):
    per = forward_bound(x, s) + 2 * U * (y64.abs() + lq.double().abs())
    red = per.mean() if reduction == 'mean' else per.sum()
    return abs(loss_weight) * float(red) + 2 * U * abs(float(loss64))


def ambiguous(x, lq, s, y64):
    """Outputs whose sign fp32 cannot decide, and the input pixels under their windows."""
    amb = (y64 - lq.double()).abs() <= forward_bound(x, s) + U * lq.double().abs()
    H, W = x.shape[-2:]
    return amb, adjoint(amb.double(), s, H, W, absolute=True) > 0


def smooth_field(shape, seed):
    """A smooth field in [0, 1]: products of low-frequency sinusoids, a different phase per plane."""
    g = torch.Generator().manual_seed(seed)
    H, W = shape[-2:]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    n = 1
    for d in shape[:-2]:
        n *= d
    ph = torch.rand(n, 3, generator=g, dtype=torch.float64) * 6.28
    f = 0.5 + 0.5 * torch.sin(0.11 * xx[None] + ph[:, :1, None]) * torch.cos(0.07 * yy[None] + ph[:, 1:2, None] +
                                                                              0.03 * xx[None])
    return f.reshape(shape).float()
