"""MATLAB's bicubic imresize restated in fp64 numpy, the yardstick of ssl_amd.prep.imresize (ssg_imresize.hip), and the
bound that holds the reference's float32 Python (basicsr/utils/matlab_functions.py:imresize) to it.

PASS ORDER: the columns are filtered first (every input row, into fp64), then the rows.  The reference filters the rows
first; in exact arithmetic the two orders give the same number and in fp64 they differ by a few 1e-16 of sum |w| |x|.

Per axis (input length n, Python-double scale s > 0, both axes share s), in doubles and in exactly this order:
  m    = math.ceil(n * s)                                    (not repaired: 50 * 1.1 = 55.00000000000001 -> 56)
  kw   = 4 / s when s < 1 and antialiasing is on, else 4;    T = ceil(kw) taps per output
  k    = 1 .. m:  u = k / s + 0.5 * (1 - 1 / s),  left = floor(u - kw / 2),  taps j = left + 1 .. left + T (1-based)
  v_j  = s * c(s * (u - j)) under antialiasing, else c(u - j);  V = ((0.0 + v_1) + v_2) + ...;  w_j = v_j / V
  c(x) = (1.5 a3 - 2.5 a2) + 1 for a <= 1, ((-0.5 a3 + 2.5 a2) - 4 a) + 2 for a <= 2, else 0, a = |x|, a2 = a a, a3 = a2 a
The reference takes P = ceil(kw) + 2 candidates left .. left + P - 1 and then drops its first and its last column.  Both
are zero in every row: u - left lies in [kw / 2, kw / 2 + 1), so the first candidate's argument is >= 2 (after the
multiplication by s where that applies) and c vanishes from 2 on; the last candidate sits at u - left - T - 1 <
kw / 2 - T <= -kw / 2.  `axis_table` asserts both.

Border: a tap outside 1 .. n is mirrored symmetrically on the index, j < 1 -> 1 - j, j > n -> 2 n + 1 - j, once.  Every
tap must satisfy 1 - n <= j <= 2 n (the reference's padding copy raises beyond that): `axis_table` raises ValueError.
The tables returned are 0-based: first = left, and the mirror is j < 0 -> -1 - j, j >= n -> 2 n - 1 - j.

Sums: y = ((0.0 + w_1 x_1) + w_2 x_2) + ..., every product rounded before it is added.  Float output: one rounding to
fp32.  Byte output: min(255, floor(y + 0.5)) for y >= 0, 0 below, y summed over the byte values 0 .. 255 themselves.

THE BOUND on |reference - restatement| (`reference_bound`), first order in e = 2^-24, per element.  The reference works
in float32 throughout; per axis and output k, with P = T + 2 candidates j, s' = s under antialiasing and 1 otherwise:
  coordinate   x / s rounds s to float32 and the quotient (2 e |k / s|), the Python-double constant 0.5 (1 - 1 / s) is
               rounded when it is added (e |const|) and the sum is rounded (e |u|):
                   du = e (2 |k / s| + |0.5 (1 - 1 / s)| + |u|)            (<~ 4 e |u| once k / s dominates)
               The distance u - j is rounded (e |u - j|) and, under antialiasing, multiplied by the rounded s (2 e |t|):
                   dt = s' (du + e |u - j|) + [aa] 2 e |t|,     t = s' (u - j)
               and reaches the weight through max |c'| = 25 / 18 (at |x| = 5 / 9).
  weights      c is evaluated in float32: each monomial carries at most three roundings and the sum two more, 5 e A(t)
               with A the sum of the monomials' magnitudes; the product by s two more:
                   dv_j = s' (25 / 18 dt + 5 e A(t)) + [aa] 2 e |v_j|
               normalisation: V is a float32 sum of P terms, the quotient is rounded:
                   dV = sum dv_j + (P - 1) e sum |v_j|,    dw_j = dv_j / V + |w_j| dV / V + e |w_j|
  dot product  each pass is a float32 matrix-vector product of T terms: T e sum |w_j| |x_j| whatever its order.
The first pass (rows, in the reference's order) gives E1 = sum (dw_j + T e |w_j|) |x_j|; the second gives
E = sum (dw_j + T e |w_j|) |t_j| + sum |w_j| E1_j with t the first pass's output.  A window that the float32 floor
shifts by one changes nothing at first order: the candidates it trades carry weights of second order (c and c' vanish
at 2).  The bound is an envelope: at dyadic scales every coordinate is exact and the reference uses a few percent of
it; at 0.3, 0.7, 1.5 and 3 the coordinate term grows with the side as the observed difference does."""
import math

import numpy as np

EPS32 = 2.0 ** -24
MAX_TAPS = 32
DYADIC = (0.125, 0.25, 0.5, 2.0, 4.0, 8.0)


def cubic(x):
    a = np.abs(np.asarray(x, np.float64))
    a2 = a * a
    a3 = a2 * a
    inner = (1.5 * a3 - 2.5 * a2) + 1.0
    outer = ((-0.5 * a3 + 2.5 * a2) - 4.0 * a) + 2.0
    return np.where(a <= 1.0, inner, np.where(a <= 2.0, outer, 0.0))


def out_size(n, s):
    return math.ceil(n * s)


def taps(s, antialiasing=True):
    return math.ceil(4 / s) if (s < 1 and antialiasing) else 4


def _axis(n, s, antialiasing):
    if not (s > 0 and math.isfinite(s)):
        raise ValueError(f"scale must be positive and finite, got {s!r}")
    if n < 1:
        raise ValueError(f"an axis of length {n}")
    aa = bool(s < 1 and antialiasing)
    kw = 4 / s if aa else 4
    T = math.ceil(kw)
    m = math.ceil(n * s)
    k = np.arange(1, m + 1, dtype=np.float64)
    u = k / s + 0.5 * (1 - 1 / s)
    left = np.floor(u - kw / 2)
    return aa, kw, T, m, u, left


def axis_table(n, s, antialiasing=True):
    """(first (m,) int64, weights (m, T) float64): 0-based first tap before the mirror, normalised fp64 weights."""
    aa, kw, T, m, u, left = _axis(n, s, antialiasing)
    if T > MAX_TAPS:
        raise NotImplementedError(f"{T} taps")
    j = left[:, None] + np.arange(0, T + 2, dtype=np.float64)[None, :]       # the reference's P candidates, 1-based
    d = u[:, None] - j
    v = s * cubic(s * d) if aa else cubic(d)
    assert not v[:, 0].any() and not v[:, -1].any(), "the two columns the reference drops are not zero"
    v = v[:, 1:-1]
    V = np.zeros(m)
    for i in range(T):
        V = V + v[:, i]
    w = v / V[:, None]
    lo, hi = left[0] + 1, left[-1] + T                                       # 1-based extremes: left never decreases
    assert (np.diff(left) >= 0).all()
    if lo < 1 - n or hi > 2 * n:
        raise ValueError(f"taps {int(lo)} .. {int(hi)} of an axis of length {n} at scale {s} leave [{1 - n}, {2 * n}]")
    return left.astype(np.int64), w


def mirror(j, n):
    """0-based symmetric mirror, one reflection."""
    j = np.where(j < 0, -1 - j, j)
    return np.where(j >= n, 2 * n - 1 - j, j)


def _indices(first, T, n):
    idx = mirror(first[:, None] + np.arange(T)[None, :], n)
    assert idx.min() >= 0 and idx.max() < n
    return idx


def resize_planes(x, s, antialiasing=True):
    """x (..., H, W) of any real dtype -> fp64 (..., h, w): columns first, then rows, sums in tap order."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    fy, wy = axis_table(H, s, antialiasing)
    fx, wx = axis_table(W, s, antialiasing)
    T = wx.shape[1]
    ix, iy = _indices(fx, T, W), _indices(fy, T, H)
    t = np.zeros(x.shape[:-1] + (len(fx),))
    for i in range(T):
        t = t + wx[:, i] * x[..., ix[:, i]]
    y = np.zeros(x.shape[:-2] + (len(fy), len(fx)))
    for i in range(T):
        y = y + wy[:, i, None] * t[..., iy[:, i], :]
    return y


def to_bytes(y):
    return np.where(y >= 0, np.minimum(255.0, np.floor(y + 0.5)), 0.0).astype(np.uint8)


def imresize_float(x, s, antialiasing=True):
    """float planes (..., H, W) -> float32, rounded once."""
    return resize_planes(x, s, antialiasing).astype(np.float32)


def imresize_bytes(a, s, antialiasing=True):
    """uint8 (H,W), (H,W,C) or (B,H,W,C) -> (bytes in the same layout, the fp64 sums y in the same layout)."""
    a = np.asarray(a)
    assert a.dtype == np.uint8
    p = a if a.ndim == 2 else np.moveaxis(a, -1, -3)
    y = resize_planes(p, s, antialiasing)
    y = y if a.ndim == 2 else np.moveaxis(y, -3, -1)
    return to_bytes(y), y


# ----------------------------------------------------------------------------------------- integer restatement ---
def dyadic_shift(s, antialiasing=True):
    """q such that every weight of the axis at a dyadic scale is an integer multiple of 2^-q."""
    assert s in DYADIC
    # c is a cubic polynomial with coefficients in halves: arguments in multiples of 2^-g give values in multiples of
    # 2^-(3 g + 1).  Upscaling by 2^e has u - j in multiples of 2^-(e + 1); antialiased downscaling by 2^-e has
    # s (u - j) in multiples of 2^-(e + 1) and the factor s = 2^-e in front; without antialiasing u - j is a half-integer
    e = int(round(abs(math.log2(s))))
    if s > 1:
        return 3 * (e + 1) + 1
    return (3 * (e + 1) + 1 + e) if antialiasing else 4


def resize_planes_int(a, s, antialiasing=True):
    """uint8 planes (..., H, W) at a dyadic scale -> (y numerator int64, total shift Q): y = numerator / 2^Q exactly."""
    a = np.asarray(a)
    assert a.dtype == np.uint8
    H, W = a.shape[-2:]
    q = dyadic_shift(s, antialiasing)
    tabs = []
    for n in (H, W):
        f, w = axis_table(n, s, antialiasing)
        wi = w * float(2 ** q)
        assert np.array_equal(wi, np.round(wi)), "a scaled weight is not an integer"
        wi = wi.astype(np.int64)
        assert (wi.sum(1) == 2 ** q).all(), "a row sum is not exactly one"
        tabs.append((_indices(f, w.shape[1], n), wi))
    (iy, wy), (ix, wx) = tabs
    x = a.astype(np.int64)
    t = sum(wx[:, i] * x[..., ix[:, i]] for i in range(wx.shape[1]))
    y = sum(wy[:, i, None] * t[..., iy[:, i], :] for i in range(wy.shape[1]))
    assert int(np.abs(y).max()) < 2 ** 52                                   # the fp64 sums are exact as well
    return y, 2 * q


def int_to_bytes(num, Q):
    """min(255, floor(y + 1 / 2)) for y >= 0, 0 below, on y = num / 2^Q: floor((num + 2^(Q-1)) / 2^Q) in integers."""
    v = (num + (1 << (Q - 1))) >> Q
    return np.clip(np.where(num >= 0, v, 0), 0, 255).astype(np.uint8)


def int_ties(num, Q):
    """where y = k + 1 / 2 exactly, 0 <= y < 255"""
    return ((num & ((1 << Q) - 1)) == (1 << (Q - 1))) & (num >= 0) & (num < (255 << Q))


def imresize_bytes_int(a, s, antialiasing=True):
    a = np.asarray(a)
    p = a if a.ndim == 2 else np.moveaxis(a, -1, -3)
    num, Q = resize_planes_int(p, s, antialiasing)
    b = int_to_bytes(num, Q)
    return b if a.ndim == 2 else np.moveaxis(b, -3, -1)


def tie_image(s, H=64, W=64, want=32, seed=0, tries=400):
    """A byte image (H,W), H == W, with at least `want` outputs that are exact ties (y = k + 1 / 2) at the dyadic scale
    s, found by search with the integer restatement.  Candidates: staircases (one to four steps of random height at
    random places, constant along the other axis, in either orientation): a step whose edge falls on the centre of an
    output's kernel gives (a + b) / 2 there, a tie for a + b odd, in every output of that line.  Returns (image, count)."""
    assert H == W
    rng = np.random.default_rng(seed)
    best, best_n = None, -1
    for t in range(tries):
        steps = int(rng.integers(1, 5))
        pos = np.sort(rng.choice(np.arange(1, W), steps, replace=False))
        levels = rng.integers(0, 256, steps + 1).astype(np.uint8)
        profile = levels[np.searchsorted(pos, np.arange(W), side="right")]
        a = np.ascontiguousarray(np.broadcast_to(profile, (H, W)))
        a = np.ascontiguousarray(a.T) if t % 2 else a
        num, Q = resize_planes_int(a, s)
        n = int(int_ties(num, Q).sum())
        if n > best_n:
            best, best_n = a, n
    assert best_n >= want, (s, best_n)
    return best, best_n


def clear_of_ties(s, shape, seed, margin=1e-9, antialiasing=True):
    """bytes of `shape` ((H,W), (H,W,C) or (B,H,W,C)) for which no fp64 sum y lies within `margin` of k + 1 / 2
    (asserted): there the byte does not depend on the last bits of y, so an implementation that sums in another order
    must give the same bytes.  Random bytes, repaired: at 1.5 and 3 some outputs sit on half-integer coordinates, their
    weights are multiples of 1 / 256 and random bytes tie there a few times per image, so the lowest bit of the input
    pixel under the middle of each such output is flipped until none is left."""
    a = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    p = np.ascontiguousarray(a if a.ndim == 2 else np.moveaxis(a, -1, -3))          # planes (..., H, W)
    H, W = p.shape[-2:]
    fy, wy = axis_table(H, s, antialiasing)
    fx, wx = axis_table(W, s, antialiasing)
    my, mx = mirror(fy + wy.shape[1] // 2, H), mirror(fx + wx.shape[1] // 2, W)
    for _ in range(50):
        y = resize_planes(p, s, antialiasing)
        near = np.argwhere(np.abs(y - np.floor(y) - 0.5) <= margin)
        if len(near) == 0:
            out = np.ascontiguousarray(p if a.ndim == 2 else np.moveaxis(p, -3, -1))
            assert np.abs(imresize_bytes(out, s, antialiasing)[1] % 1.0 - 0.5).min() > margin
            return out
        for at in near:
            p[tuple(at[:-2]) + (my[at[-2]], mx[at[-1]])] ^= 1
    raise AssertionError((s, shape, seed))


# ---------------------------------------------------------------------------------------------------- the bound ---
def _axis_errors(n, s, antialiasing):
    """(first, |w| (m,T), dw (m,T) >= 0, split (m,T,2): the coordinate's and the weights' share of dw)"""
    aa, kw, T, m, u, left = _axis(n, s, antialiasing)
    e = EPS32
    k = np.arange(1, m + 1, dtype=np.float64)
    du = e * (2 * np.abs(k / s) + abs(0.5 * (1 - 1 / s)) + np.abs(u))
    j = left[:, None] + np.arange(0, T + 2, dtype=np.float64)[None, :]      # all P candidates
    d = u[:, None] - j
    sp = s if aa else 1.0
    t = sp * d
    v = sp * cubic(t)
    a = np.minimum(np.abs(t), 2.0)
    A = np.where(np.abs(t) <= 1.0, 1.5 * a ** 3 + 2.5 * a ** 2 + 1.0, 0.5 * a ** 3 + 2.5 * a ** 2 + 4.0 * a + 2.0)
    dt = sp * (du[:, None] + e * np.abs(d)) + (2 * e * np.abs(t) if aa else 0.0)
    dv_coord = sp * (25.0 / 18.0) * dt
    dv_eval = sp * 5 * e * A + (2 * e * np.abs(v) if aa else 0.0)
    V = v.sum(1)
    w = v / V[:, None]
    P = T + 2

    def normalised(dv, with_sum):
        dV = dv.sum(1) + ((P - 1) * e * np.abs(v).sum(1) if with_sum else 0.0)
        return dv / V[:, None] + np.abs(w) * (dV / V)[:, None] + (e * np.abs(w) if with_sum else 0.0)

    dw_coord, dw_eval = normalised(dv_coord, False), normalised(dv_eval, True)
    return left.astype(np.int64), np.abs(w), dw_coord, dw_eval, P


def reference_bound(x, s, antialiasing=True):
    """x float planes (..., H, W) -> dict of per-element fp64 arrays (..., h, w): 'coordinate', 'weights', 'dot' and
    their sum 'total', the first-order envelope of |reference - restatement| derived in the module docstring."""
    x = np.abs(np.asarray(x, np.float64))
    H, W = x.shape[-2:]
    fy, wy, cy, ey, P = _axis_errors(H, s, antialiasing)
    fx, wx, cx, ex, _ = _axis_errors(W, s, antialiasing)
    T = P - 2
    iy = mirror(fy[:, None] + np.arange(P)[None, :], H).clip(0, H - 1)      # (candidates beyond the domain carry 0)
    ix = mirror(fx[:, None] + np.arange(P)[None, :], W).clip(0, W - 1)

    def rows(k, v):      # sum_j k[q][j] v[..., iy[q][j], :]
        return sum(k[:, i, None] * v[..., iy[:, i], :] for i in range(P))

    def cols(k, v):
        return sum(k[:, i] * v[..., ix[:, i]] for i in range(P))

    t1 = rows(wy, x)                                                        # sum |w| |x| of the reference's first pass
    out = {}
    for name, ky, kx in (("coordinate", cy, cx), ("weights", ey, ex), ("dot", T * EPS32 * wy, T * EPS32 * wx)):
        out[name] = cols(kx, t1) + cols(wx, rows(ky, x))
    out["total"] = out["coordinate"] + out["weights"] + out["dot"]
    return out


def modcrop(a, modulo):
    H, W = a.shape[:2]
    return a[:H - H % modulo, :W - W % modulo]


# ---------------------------------------------------------------------------------------------------- the fixture ---
SCALES = {"1_2": 1 / 2, "1_3": 1 / 3, "1_4": 1 / 4, "1_8": 1 / 8, "0.3": 0.3, "0.7": 0.7, "1.5": 1.5, "2": 2, "3": 3,
          "4": 4}
FIXTURE_INPUTS = {"small": (19, 23), "mid": (37, 101), "big": (300, 255), "far": (64, 48)}     # (H, W), 3 channels each


def case_tag(name, scale_name, aa):
    return f"{name}@{scale_name}@{'aa' if aa else 'noaa'}"


FIXTURE_CASES = ([(n, k, True) for n in ("small", "mid") for k in SCALES]
                 + [(n, k, False) for n in ("small", "mid") for k in ("1_2", "1_3")]
                 + [("big", "1_4", True), ("big", "0.7", True)])
FIXTURE_CASE_TAGS = [case_tag(*c) for c in FIXTURE_CASES]
FIXTURE_PART_B = ("mid@4@aa", "big@0.7@aa")          # the outputs kept in f30_imresize_b.npz
# what make_golden_imresize.py tries: the cases, and one the reference is known to raise on
FIXTURE_CANDIDATES = FIXTURE_CASES + [("far", "1_4", False)]


def fixture_input(b):
    """the float32 input of a fixture case from its stored bytes"""
    return np.asarray(b, np.float32) / np.float32(255)


def load_fixture(golden_dir):
    """{tag: (x float32 (3,H,W), scale, antialiasing, reference output float32 (3,h,w))} and the skipped list"""
    import os
    out = {}
    with np.load(os.path.join(golden_dir, "f30_imresize.npz")) as za, \
            np.load(os.path.join(golden_dir, "f30_imresize_b.npz")) as zb:
        in_b = set(za["part_b"].tolist())
        for tag in za["cases"].tolist():
            name, scale_name, aa = tag.split("@")
            planes = (zb if tag in in_b else za)["out_" + tag]
            y = np.ascontiguousarray(planes.transpose(1, 2, 3, 0)).view(np.float32)[..., 0]
            out[tag] = (fixture_input(za["in_" + name]), SCALES[scale_name], aa == "aa", y)
        skipped = za["skipped"].tolist()
    return out, skipped
