"""An fp64 numpy restatement of the staged contract of ssl_amd/csrc/ssg_specnorm.hip (include/ssg_hip.h section (Y)),
with first-order error bounds that are DERIVED here, not tuned.

The contract, per layer (W fp32 R x K, u fp32 R, v fp32 K), eps = 1e-12, max(x, eps) = eps where x < eps (a NaN passes):
    training:  t = W^T u;  v = f32(t / max(|t|, eps));  s = W v (from the fp32 v);  u = f32(s / max(|s|, eps))
    eval:      v, u as stored;  s = W v
    sigma = u . s (fp32 u, fp64 s);  sigma32 = f32(sigma);  W_sn = W / sigma32 (one fp32 division)
    backward:  c = <G, W_sn>;  dW = f32((G - c u v^T) / sigma32)
Products of two fp32 values are exact in fp64; sums are fp64.

The bounds.  E is the unit roundoff of the SUMS (2^-53 for the kernels and for this restatement, 2^-24 for torch's own
fp32 lines), e = 2^-24 that of an fp32 cast, TINY = 2^-149 the spacing of the fp32 subnormals (a cast that lands there is
off by at most that).  A sum of n terms x_i evaluated in any order differs from the exact sum by at most
(n + 2) E sum|x_i| (to first order; the + 2 covers the roundings of the operations around it), so two evaluations in
two orders differ by at most twice that.  Two fp32 casts of two values that differ by d differ by at most d + 2 e |x|
(each is within half a spacing, e |x|, of its own value): that is "one flipped last bit".  Everything downstream of v is
computed by each side from ITS OWN fp32 v, so a difference dv in v enters s as sum_j |W_rj| dv_j, and so on:
    dt_j   = 2 (R + 2) E sum_r |u_r W_rj|
    d|t|   = (sum_j |t_j| dt_j + (K + 2) E |t|^2) / |t| + E |t|           (max(., eps) is 1-Lipschitz)
    dv_j   = dt_j / den + |t_j| d|t| / den^2 + (2 e + 2 E) |v_j| + TINY   den = max(|t|, eps);  0 in eval mode
    ds_r   = sum_j |W_rj| dv_j + 2 (K + 2) E sum_j |W_rj v_j|
    d|s|, du_r as d|t|, dv_j
    dsig   = sum_r (du_r |s_r| + |u_r| ds_r) + 2 (R + 2) E sum_r |u_r s_r|
    dsig32 = dsig + 2 e |sigma| + TINY
    dWsn   = |W| dsig32 / sigma^2 + ROUND e |W_sn| + TINY     exactly 0 where both sides hold the same sigma32
    dc     = sum |G| dWsn + 2 (N + 2) E sum |G W_sn|
    ddW    = (dc |u_r v_j| + |c| (du_r |v_j| + |u_r| dv_j)) / |sigma| + |G - c u v| dsig32 / sigma^2
             + (ROUND e + 8 E) (|G| + |c u_r v_j|) / |sigma| + TINY
ROUND counts the fp32 roundings behind the last cast: 2 for the kernels against this restatement (one cast on either
side), `rounds` for torch's fp32 lines (each of its element-wise operations rounds once; 8 covers the quotient G /
sigma, the product G W, the quotient by sigma^2, the sign, grad_sigma u, its outer product with v, the accumulation into
the gradient and the forward's own division).  Where sigma is 0 or not finite the bounds are not finite and say nothing:
there the outputs are compared as bits (inf and NaN patterns).
"""
import numpy as np

EPS = 1e-12
E64, E32 = 2.0 ** -53, 2.0 ** -24
TINY = 2.0 ** -149


def _clamp(x):
    return np.where(x < EPS, EPS, x)          # (a NaN passes, as torch's clamp_min passes it)


def forward(W, u, v, training):
    """dict of v, u (fp32), sigma32 (fp32 scalar), out (fp32 R x K) and the fp64 intermediates t, s, sigma."""
    W = np.asarray(W, np.float32)
    W2 = W.reshape(W.shape[0], -1)
    W64 = W2.astype(np.float64)
    u, v = np.asarray(u, np.float32).reshape(-1), np.asarray(v, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        t = None
        if training:
            t = W64.T @ u.astype(np.float64)
            v = (t / _clamp(np.sqrt(np.sum(t * t)))).astype(np.float32)
        s = W64 @ v.astype(np.float64)
        if training:
            u = (s / _clamp(np.sqrt(np.sum(s * s)))).astype(np.float32)
        sigma = np.sum(u.astype(np.float64) * s)
        sigma32 = np.float32(sigma)
        out = (W2 / sigma32).astype(np.float32)
    return dict(v=v, u=u, t=t, s=s, sigma=sigma, sigma32=sigma32, out=out.reshape(W.shape))


def backward(W, fwd, G):
    """fp32 dW from the forward's own fp32 u, v, sigma32 and W_sn."""
    W2 = np.asarray(W, np.float32).reshape(W.shape[0], -1)
    G64 = np.asarray(G, np.float32).reshape(W2.shape).astype(np.float64)
    with np.errstate(all="ignore"):
        c = np.sum(G64 * fwd["out"].reshape(W2.shape).astype(np.float64))
        uv = np.outer(c * fwd["u"].astype(np.float64), fwd["v"].astype(np.float64))
        dW = ((G64 - uv) / np.float64(fwd["sigma32"])).astype(np.float32)
    return dict(c=c, dW=dW.reshape(W.shape))


def _norm_terms(x, dx, n, E):
    """(den, d norm) of max(|x|, eps) for a vector x known to dx per element."""
    nrm = np.sqrt(np.sum(x * x))
    safe = nrm if nrm > 0 else 1.0
    dn = (np.sum(np.abs(x) * dx) + (n + 2) * E * nrm * nrm) / safe + E * nrm
    return float(_clamp(nrm)), dn


def bounds(W, u0, fwd, training, G=None, bwd=None, E=E64, rounds=2):
    """Per-element bounds dv, du, dsig32 (a scalar), dout and, with G and bwd, ddW, for outputs computed by the contract
    with sums of unit roundoff E against this restatement (see the module's text).  u0 is the u the call started from."""
    W2 = np.asarray(W, np.float32).reshape(W.shape[0], -1).astype(np.float64)
    aW = np.abs(W2)
    R, K = W2.shape
    e = E32
    v, u, s = fwd["v"].astype(np.float64), fwd["u"].astype(np.float64), fwd["s"]
    with np.errstate(all="ignore"):
        if training:
            t = fwd["t"]
            dt = 2 * (R + 2) * E * (aW.T @ np.abs(np.asarray(u0, np.float64).reshape(-1)))
            den, dn = _norm_terms(t, dt, K, E)
            dv = dt / den + np.abs(t) * dn / den ** 2 + (2 * e + 2 * E) * np.abs(v) + TINY
        else:
            dv = np.zeros(K)
        ds = aW @ dv + 2 * (K + 2) * E * (aW @ np.abs(v))
        if training:
            den, dn = _norm_terms(s, ds, R, E)
            du = ds / den + np.abs(s) * dn / den ** 2 + (2 * e + 2 * E) * np.abs(u) + TINY
        else:
            du = np.zeros(R)
        sigma = np.float64(fwd["sigma32"])
        dsig = np.sum(du * np.abs(s) + np.abs(u) * ds) + 2 * (R + 2) * E * np.sum(np.abs(u * s))
        dsig32 = dsig + 2 * e * abs(fwd["sigma"]) + TINY
        out = fwd["out"].reshape(R, K).astype(np.float64)
        dout = aW * dsig32 / sigma ** 2 + rounds * e * np.abs(out) + TINY
        res = dict(dv=dv, du=du, dsig32=dsig32, dout=dout.reshape(W.shape))
        if G is not None:
            G64 = np.abs(np.asarray(G, np.float32).reshape(R, K).astype(np.float64))
            c = bwd["c"]
            dc = np.sum(G64 * dout) + 2 * (R * K + 2) * E * np.sum(G64 * np.abs(out))
            auv = np.outer(np.abs(u), np.abs(v))
            num = np.abs(bwd["dW"].reshape(R, K).astype(np.float64)) * abs(sigma)        # |G - c u v|
            ddW = ((dc * auv + abs(c) * (np.outer(du, np.abs(v)) + np.outer(np.abs(u), dv))) / abs(sigma)
                   + num * dsig32 / sigma ** 2 + (rounds * e + 8 * E) * (G64 + abs(c) * auv) / abs(sigma) + TINY)
            res["ddW"] = ddW.reshape(W.shape)
    return res


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def within(got, want, bound):
    """Element-wise: |got - want| <= bound, or the same bits, or both NaN (where the bound is not finite only the last
    two can hold).  Returns (ok array, the largest share |got - want| / bound over the finite elements)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    with np.errstate(all="ignore"):
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
        close = diff <= bound
        same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
        finite = np.isfinite(diff) & np.isfinite(bound) & (bound > 0)
        share = float(np.max(diff[finite] / bound[finite])) if finite.any() else 0.0
    return close | same, share


def check(name, got, want, bound):
    """assert `within`, with the worst element in the message; returns the share of the bound that was used."""
    ok, share = within(got, want, bound)
    if not ok.all():
        i = np.unravel_index(np.argmin(ok), ok.shape)
        raise AssertionError(f"{name}: element {i}: got {np.asarray(got)[i]!r} want {np.asarray(want)[i]!r} "
                             f"bound {np.broadcast_to(bound, ok.shape)[i]!r}; {int((~ok).sum())} of {ok.size} outside")
    return share
