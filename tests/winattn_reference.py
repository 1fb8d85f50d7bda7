"""The window attention of include/ssg_hip.h section (Z) restated in fp64 numpy from its definitions, with its adjoint
and a derived, data-dependent first-order error bound per output element.  Shared by the CPU and GPU tests.

Definitions (window 8, N = 64 tokens, C = heads d; inputs are fp32 values, everything below is fp64):
  window (wy, wx), token (iy, ix): shifted coordinate ys = 8 wy + iy, xs = 8 wx + ix, source pixel
  ((ys + shift) mod H, (xs + shift) mod W), read from and written back to.
  qs = q scale;  S_ij = qs_i . k_j + table[(iy_i - iy_j + 7) 15 + (ix_i - ix_j + 7), h] + mask_ij
  mask_ij (shift > 0) = -100 where label_i != label_j, label = 3 ly + lx, ly = (ys >= H - 8) + (ys >= H - shift)
  P = softmax_j S;  O = P v
  adjoint: dv = P^T dO, dP = dO v^T, D_i = sum_j P_ij dP_ij, dS = P (dP - D), dq = scale dS k, dk = dS^T qs,
  dtable[idx, h] = the sum of dS_ij over images, windows and the pairs of idx.

The bound counts the roundings of an fp32 evaluation, u = 2^-24, to first order, at the fp64 values:
  qs        one rounding: u |qs|
  S         a d-term sum of products of the perturbed qs: (d + 1) u A_ij, A_ij = sum_c |qs_ic k_jc|.  This holds for
            an fma chain (d roundings) and for rounded products added in ANY order (1 + (d - 1) roundings per path).
  + bias    u |s + b|;  + mask (shift > 0 only)  u |S|;  - row maximum  u |S - m| (the maximum itself is one of the
            computed scores: a shift of a whole row changes no softmax)
  exp       an fp32 libm result is within 1 ulp <= 2 u relative (EXP_U = 2: the assumption of tests/gan_reference.py,
            documented for the device library, glibc and the vectorised library torch's CPU kernels call); a result
            below the normal range may be flushed: TINY = 2^-126 absolute (the row's sum is >= 1)
  sum, /    64 positive terms in any order: 63 u relative; the quotient 2 u (one division, or a reciprocal and a
            product).  With the exp errors of numerator and denominator: REL = (2 EXP_U + 65) u relative on P.
  P         |dP_ij| <= P_ij (|dS_ij| + sum_k P_ik |dS_ik|) + REL P_ij + TINY        (softmax's derivative)
  O         sum_j EP_ij |v_jc| + 64 u sum_j P_ij |v_jc| + TINY
  backward  the same counting, term by term in `Result.bounds`: d-term and 64-term sums of products as above, one
            rounding per product, difference and scale; dtable: the sum of the dS bounds, an fp64 sum (negligible,
            counted) and the final cast.
No constant is fitted to an observed error.  The sums' bounds hold for any order of summation, so torch's fp32 lines
(BLAS products, a vectorised softmax) meet the SAME bounds for out, dqkv; torch's dtable is an fp32 sum over images,
windows and pairs in an order of torch's choosing: `table_bound_fp32` adds (n - 1) u sum |dS| for the n terms of an entry.
"""
import numpy as np

WS, N, NB = 8, 64, 225
U = 2.0 ** -24
EXP_U = 2.0
TINY = 2.0 ** -126
REL = (2 * EXP_U + 65) * U

MUTANTS = ("no_mask", "source_labels", "shift_reversed", "bias_transposed", "other_head", "scale_after_bias",
           "softmax_columns", "no_reverse_shift")


def bias_index():
    """(64, 64): the table row of (query i, key j)"""
    iy, ix = np.arange(N) // WS, np.arange(N) % WS
    return (iy[:, None] - iy[None, :] + WS - 1) * (2 * WS - 1) + (ix[:, None] - ix[None, :] + WS - 1)


def geometry(H, W, shift, labels_from_source=False, reverse=False):
    """(src, label): (nW, 64) source pixel y W + x and mask label of every token, windows in row-major order"""
    wy, wx, iy, ix = np.meshgrid(np.arange(H // WS), np.arange(W // WS), np.arange(WS), np.arange(WS), indexing="ij")
    ys, xs = WS * wy + iy, WS * wx + ix
    sy, sx = ((ys - shift) % H, (xs - shift) % W) if reverse else ((ys + shift) % H, (xs + shift) % W)
    ly, lx = (sy, sx) if labels_from_source else (ys, xs)
    label = 3 * ((ly >= H - WS).astype(int) + (ly >= H - shift)) + (lx >= W - WS).astype(int) + (lx >= W - shift)
    return (sy * W + sx).reshape(-1, N), label.reshape(-1, N)


def label_mask(H, W, shift):
    """(nW, 64, 64) of 0 / -100 by the label rule"""
    _, label = geometry(H, W, shift)
    return np.where(label[:, :, None] != label[:, None, :], -100.0, 0.0)


class Result:
    pass


def evaluate(qkv, table, heads, shift, scale, dout=None, mutant=None, bounds=True):
    """out (B, H, W, C) and, with dout, dqkv and dtable, in fp64; with `bounds` their bounds (same shapes).  `mutant`:
    one of MUTANTS, a deliberately wrong restatement (no bounds)."""
    assert mutant is None or mutant in MUTANTS
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    scale = float(np.float32(scale))
    src, label = geometry(H, W, shift, labels_from_source=mutant == "source_labels", reverse=mutant == "shift_reversed")
    nW = src.shape[0]
    tok = qkv.astype(np.float64).reshape(B, H * W, 3, heads, d)[:, src]           # (B, nW, 64, 3, heads, d)
    q, k, v = (np.moveaxis(tok[:, :, :, s], 3, 2) for s in range(3))                # (B, nW, heads, 64, d)
    idx = bias_index()
    tab = table.astype(np.float64)
    if mutant == "other_head":
        tab = np.roll(tab, 1, axis=1)
    bias = np.moveaxis(tab[idx.T if mutant == "bias_transposed" else idx], 2, 0)    # (heads, 64, 64)
    masked = shift > 0 and mutant != "no_mask"
    mask = np.where(label[:, :, None] != label[:, None, :], -100.0, 0.0)[None, :, None] if masked else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        if mutant == "scale_after_bias":
            s0 = q @ np.swapaxes(k, -1, -2)
            sb = (s0 + bias) * scale
            qs = q
        else:
            qs = q * scale
            s0 = qs @ np.swapaxes(k, -1, -2)
            sb = s0 + bias
        S = sb + mask
        axis = -2 if mutant == "softmax_columns" else -1
        m = S.max(axis=axis, keepdims=True)
        e = np.exp(S - m)
        P = e / e.sum(axis=axis, keepdims=True)
        O = P @ v                                                                  # (B, nW, heads, 64, d)

    def scatter(x, width):
        """(B, nW, heads, 64, d) -> (B, H, W, width-th part layout (heads d))"""
        flat = np.empty((B, H * W, heads, d))
        dst = geometry(H, W, 0)[0] if mutant == "no_reverse_shift" else src
        flat[:, dst] = np.moveaxis(x, 2, 3)
        return flat.reshape(B, H, W, heads * d)

    r = Result()
    r.out = scatter(O, C)
    r.P = P
    if bounds and mutant is None:
        A = np.abs(qs) @ np.swapaxes(np.abs(k), -1, -2)
        ES = (d + 1) * U * A + U * np.abs(sb) + (U * np.abs(S) if masked else 0.0) + U * np.abs(S - m)
        EP = P * (ES + (P * ES).sum(-1, keepdims=True)) + REL * P + TINY
        r.out_bound = scatter(EP @ np.abs(v) + N * U * (P @ np.abs(v)) + TINY, C)
    if dout is None:
        return r
    g = np.moveaxis(dout.astype(np.float64).reshape(B, H * W, heads, d)[:, src], 3, 2)   # (B, nW, heads, 64, d)
    with np.errstate(invalid="ignore", over="ignore"):
        dP = g @ np.swapaxes(v, -1, -2)
        t = P * dP
        Drow = t.sum(-1, keepdims=True)
        diff = dP - Drow
        dS = P * diff
        dv = np.swapaxes(P, -1, -2) @ g
        dk = np.swapaxes(dS, -1, -2) @ qs
        dq = scale * (dS @ k)
    r.dqkv = np.concatenate([scatter(x, C) for x in (dq, dk, dv)], axis=-1)
    per_head = dS.sum(axis=(0, 1))                                                 # (heads, 64, 64)
    r.dtable = np.stack([np.bincount(idx.ravel(), weights=per_head[h].ravel(), minlength=NB) for h in range(heads)], 1)
    if bounds and mutant is None:
        EdP = d * U * (np.abs(g) @ np.swapaxes(np.abs(v), -1, -2))
        Et = np.abs(dP) * EP + P * EdP + U * np.abs(t)
        ED = Et.sum(-1, keepdims=True) + (N - 1) * U * np.abs(t).sum(-1, keepdims=True)
        EdS = EP * np.abs(diff) + P * (EdP + ED + U * np.abs(diff)) + U * np.abs(dS) + TINY
        Edv = np.swapaxes(EP, -1, -2) @ np.abs(g) + N * U * (np.swapaxes(P, -1, -2) @ np.abs(g)) + TINY
        Edk = (np.swapaxes(EdS, -1, -2) @ np.abs(qs) + (N + 1) * U * (np.swapaxes(np.abs(dS), -1, -2) @ np.abs(qs))
               + TINY)
        Edq = abs(scale) * (EdS @ np.abs(k) + N * U * (np.abs(dS) @ np.abs(k))) + U * np.abs(dq) + TINY
        r.dqkv_bound = np.concatenate([scatter(x, C) for x in (Edq, Edk, Edv)], axis=-1)
        terms = B * nW * np.bincount(idx.ravel(), minlength=NB)[:, None]           # the terms of an entry's sum
        sum_E, sum_abs = (np.stack([np.bincount(idx.ravel(), weights=x.sum(axis=(0, 1))[h].ravel(), minlength=NB)
                                    for h in range(heads)], 1) for x in (EdS, np.abs(dS)))
        r.dtable_bound = sum_E + terms * 2.0 ** -53 * sum_abs + U * np.abs(r.dtable) + TINY
        r.dtable_bound_fp32 = r.dtable_bound + (terms - 1) * U * sum_abs
    return r


def share(got, want, bound):
    """The largest |got - want| / bound over the elements where `want` is a number; NaNs must coincide."""
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs"
    if nan.all():
        return 0.0
    ok = ~nan
    assert np.isfinite(bound[ok]).all() and (bound[ok] > 0).all()
    return float((np.abs(got[ok] - want[ok]) / bound[ok]).max())
