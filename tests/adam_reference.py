"""The Adam / AdamW step's contract (include/ssg_hip.h section (X), ssl_amd/csrc/ssg_multi.hip) three times over:

1. `restate`: numpy float32, one `.astype(float32)` per operation.  The kernel must equal it BIT FOR BIT.
2. `exact`: the same formulas in fp64 from the same fp32 inputs and the host's DOUBLE scalars.
3. `bound`: per element and data dependent, how far ANY fp32 evaluation that rounds each operation of the contract once
   (in this association, with or without a fused multiply-add, which only removes a rounding) can lie from `exact`.

Torch's own fp32 Adam is NOT the restatement's bits (its lerp_ and vectorised multiply-adds round differently in 10-40 %
of the elements), so the gate has two halves: kernel == restate bit for bit, and restate and torch each within `bound`
of `exact`.

The bound is a running error analysis, u = 2^-24.  A value computed as fl(x op y) from operands that carry errors e has
error at most E + u (|R| + E) + tiny, with R the exact result, E the operands' errors propagated through the operation
(sum: e_x + e_y; product: |X| e_y + |Y| e_x + e_x e_y; quotient: (e_x + |X / Y| e_y) / (|Y| - e_y); square root:
min(sqrt(e), e / sqrt(V))) and tiny = 2^-149 for a result in the subnormal range.  A host scalar S cast to float carries
u |S|.  Counting the roundings gives, to first order, with sg = |g| + wd |p| (NOT |g'|: g' = g + wd p cancels) and
c = 3 under L2 weight decay (the cast of wd, the product, the sum), c = 0 otherwise:
    e(g') <= c u sg
    e(m)  <= u [w1 (c sg + 3 (|g' - m|)) + |m_new|]             <= (1 + (3 + c) w1) units of u (|m| + sg)
    e(v)  <= u [2 b2 |v| + 3 w2 g'^2 + 2 w2 |g'| c sg + |v_new|]  <= 3 + 2 c units of u (|v| + sg^2) (+ e(g')^2 w2)
    e(den) from e(v) through the square root (e(v) / (2 sqrt(v))), the quotient by s2 and the sum with eps: 5 more u
    e(p)  <= u (|p'| + |p_new| + 3 |update|) + a e(m) / den + |update| e(den) / den
The error of p is not proportional to |update|: m's error enters through a e(m) / den, and e(m) is of the size of a
rounding of |m| + |g|, which the subtraction inside the lerp cancels.  `bound` evaluates the running analysis itself, not
these closed forms, so second-order terms (e(g')^2 where g' cancels to nothing) are kept.
fp32's range is modelled in `exact`: an intermediate beyond the largest float is an infinity, as the fp32 evaluation's is.
"""
import numpy as np

PLAIN, L2, DECOUPLED = 0, 1, 2        # include/ssg_hip.h: SSG_ADAM_*
U = 2.0 ** -24
TINY = 2.0 ** -149
FLT_MAX = float(np.finfo(np.float32).max)
F = np.float32


def host_scalars(lr, beta1, beta2, eps, weight_decay, decoupled, step):
    """The scalars in Python doubles, by torch's expressions (_single_tensor_adam): a dict; `mode` an int."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    mode = PLAIN if weight_decay == 0 else (DECOUPLED if decoupled else L2)
    return dict(a=lr / bias_correction1, w1=1 - beta1, b2=beta2, w2=1 - beta2, s2=bias_correction2 ** 0.5, eps=eps,
                wd=weight_decay if mode == L2 else 0.0, cwd=1 - lr * weight_decay if mode == DECOUPLED else 1.0, mode=mode)


def restate(p, g, m, v, s):
    """(p, m, v) after one step: the contract in float32, every operation rounded on its own.  s: host_scalars()."""
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    a, w1, b2, w2, s2, eps, wd, cwd = (F(s[k]) for k in ("a", "w1", "b2", "w2", "s2", "eps", "wd", "cwd"))
    with np.errstate(all="ignore"):
        q = p
        if s["mode"] == L2:
            decay = (wd * p).astype(F)
            g = (g + decay).astype(F)
        if s["mode"] == DECOUPLED:
            q = (p * cwd).astype(F)
        diff = (g - m).astype(F)
        lerp = (w1 * diff).astype(F)
        m = (m + lerp).astype(F)
        kept = (v * b2).astype(F)
        sq = (g * g).astype(F)
        added = (w2 * sq).astype(F)
        v = (kept + added).astype(F)
        root = np.sqrt(v).astype(F)
        scaled = (root / s2).astype(F)
        den = (scaled + eps).astype(F)
        ratio = (m / den).astype(F)
        step = (a * ratio).astype(F)
        p = (q - step).astype(F)
    return p, m, v


def _ranged(x):
    """fp32's range on an fp64 intermediate: beyond the largest float it is an infinity."""
    return np.where(np.abs(x) > FLT_MAX, np.copysign(np.inf, x), x)


class _V:
    """An exact (fp64) value with the error bound of its fp32 counterpart."""

    def __init__(self, x, e=0.0):
        self.x = np.asarray(x, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.x.shape)

    def rounded(self, ulps=0.5):
        """One fp32 rounding of the result (correct rounding: half an ulp, u relative)."""
        x = _ranged(self.x)
        return _V(x, self.e + 2 * ulps * U * (np.abs(x) + self.e) + TINY)


def _scalar(S):
    return _V(np.float64(S), U * abs(S) + (TINY if S != 0 and abs(S) < 2.0 ** -126 else 0.0))


def _add(a, b, sign=1.0):
    return _V(a.x + sign * b.x, a.e + b.e).rounded()


def _mul(a, b):
    return _V(a.x * b.x, np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e).rounded()


def _div(a, b):
    room = np.abs(b.x) - b.e
    q = a.x / b.x
    e = np.where(room > 0, (a.e + np.abs(q) * b.e) / np.where(room > 0, room, 1.0), np.inf)
    return _V(q, e).rounded()


def _sqrt(a, ulps):
    r = np.sqrt(a.x)
    e = np.minimum(np.sqrt(a.e), np.where(r > 0, a.e / np.where(r > 0, r, 1.0), np.inf))
    return _V(r, e).rounded(ulps)


def exact_and_bound(p, g, m, v, s, sqrt_ulps=0.5):
    """((p, m, v) in fp64, (bound of p, of m, of v)) for fp32 inputs and host_scalars() s.  sqrt_ulps: the square root's
    own error, 0.5 for the contract's correctly rounded one (the kernel's, numpy's), 1 for a faithfully rounded one
    (torch's CPU sqrt on an MKL build: 0.65 % of its results are the float on the other side of the exact root)."""
    with np.errstate(all="ignore"):
        p, g, m, v = (_V(np.asarray(x, dtype=F)) for x in (p, g, m, v))
        q = p
        if s["mode"] == L2:
            g = _add(g, _mul(_scalar(s["wd"]), p))
        if s["mode"] == DECOUPLED:
            q = _mul(p, _scalar(s["cwd"]))
        m = _add(m, _mul(_scalar(s["w1"]), _add(g, m, -1.0)))
        v = _add(_mul(v, _scalar(s["b2"])), _mul(_scalar(s["w2"]), _mul(g, g)))
        den = _add(_div(_sqrt(v, sqrt_ulps), _scalar(s["s2"])), _scalar(s["eps"]))
        p = _add(q, _mul(_scalar(s["a"]), _div(m, den)), -1.0)
    return (p.x, m.x, v.x), (p.e, m.e, v.e)


def share(got, want, bound):
    """The largest |got - want| / bound over EVERY element, after the conditions no element escapes: at a NaN of `want`
    `got` is a NaN and nowhere else; where `want` is infinite `got` is the same infinity and nowhere else."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == bound.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), "infinities differ"
    fin = np.isfinite(want)
    assert not np.isnan(bound[fin]).any()
    err, b = np.abs(got[fin] - want[fin]), bound[fin]
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(r.max()) if r.size else 0.0


def units(got, want, scale):
    """The largest |got - want| in units of 2^-24 scale (the issue's table; an observation)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want) & (scale > 0)
    return float((np.abs(got[fin] - want[fin]) / (U * scale[fin])).max()) if fin.any() else 0.0


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.int32)


def same_bits(got, want):
    """Equal int32 patterns, except that where both are NaN any NaN matches."""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def gradients(rng, n):
    """N(0, 1) 10^U(-7, 0): the spread of a network's gradients, tensor to tensor."""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-7, 0, n)).astype(F)


def state_at(rng, n, step, beta1, beta2):
    """A plausible (p, m, v) in front of step `step`: zeros in front of the first, else what steps of such gradients leave."""
    p = (rng.standard_normal(n) * 0.05).astype(F)
    if step == 1:
        return p, np.zeros(n, F), np.zeros(n, F)
    scale = 10.0 ** rng.uniform(-7, 0, n)
    k = min(step - 1, 50)
    m = (rng.standard_normal(n) * scale * (1 - beta1 ** k) * 0.3).astype(F)
    v = ((rng.standard_normal(n) * scale) ** 2 * (1 - beta2 ** k)).astype(F)
    return p, m, v
