"""fp64 restatement of the GAN criteria's contract (ssl_amd/csrc/ssg_gan.hip, include/ssg_hip.h section (Q)): l(d) and
l'(d) of the five kinds, the plain and multi-scale reductions, the relativistic term and generator with both gradients,
and the error bound an fp32 evaluation is held to.  torch on the CPU, nothing of ssl_amd.

Contract: d = x - shift, ONE fp32 subtraction (shift = 0: d = x); t = the label as an fp32 value, s = +-1;
    BCE       l = max(d, 0) - d t + log1p(exp(-|d|))      l' = sigmoid(d) - t
    LS        l = (d - t)^2                                l' = 2 (d - t)
    LINEAR    l = s d                                      l' = s
    SOFTPLUS  l = softplus(z), z = s d                     l' = s sigmoid(z)
    HINGE     l = relu(z), z = 1 + s d                     l' = 0 where z <= 0, else s (torch's ReLU backward)
    plain          L = w mean l(x)                               dL/dx_i = w l'(x_i) / n
    relativistic   L = w mean_i l(p_i - m), m = fl32(mean(o))    dL/dp_i = w l'(d_i) / n_p,
                                                                 dL/do_j = -w sum_i l'(d_i) / (n_p n_o)
    generator      L = (term_A(real, fake) + term_B(fake, real)) / 2, gradients added.
With exact=True nothing is rounded to fp32 (the mean stays fp64, d = x - m in fp64): that form is what fp64 autograd
through the torch expressions computes, and is held to it to 1e-12 (tests/test_cpu_gan.py).

The bound (first order, u = 2^-24), evaluated at the same fp32 d as the restatement:
  exp, log1p  an fp32 libm result is within 1 ulp <= 2 u relative (FN_U = 2; documented for the device library, for
              glibc and for the vectorised library torch's CPU kernels call): exp's error reaches l through
              d log1p(e) / de = 1 / (1 + e), i.e. 2 u e / (1 + e) (BCE) -- torch's softplus takes log1p(exp(z)) directly
              below its cut, where the same term is 2 u exp(z) / (1 + exp(z)) = 2 u sigmoid(z) >= the other form's --;
              log1p's own error is 2 u l.
  arithmetic  one rounding per operation, relative to the value it rounds.  BCE is evaluated as max(d, 0) - d t + l by
              the kernels and as (1 - t) d + max(-d, 0) + l by torch: four roundings at most (1 - t, a product, two
              additions) on M = |d| + |d t| + |(1 - t) d| + l, which bounds every intermediate of both.  LS: d - t
              (twice its relative error on the square) and the square: 3 u (d - t)^2.  LINEAR: exact.  SOFTPLUS: one
              addition, u l.  HINGE: one addition, u |z| (s d and the relu are exact).
  sigmoid     exp (2 u, at most 2 u on the quotient), 1 + e, the division, the product e r: SIG_U = 5 roundings on
              sigmoid(z); BCE's subtraction of t one more on |sigmoid - t|.  LS's 2 (d - t): one rounding, taken twice
              for a backward pass that multiplies in another order.  LINEAR and HINGE derivatives are exact: fl32(1 + s d)
              has the sign of 1 + s d (a sum of two floats that cancels to less than an ulp of either is exact).
  subnormals  one absolute term TINY = 2^-126 per element: softplus(-100) = 3.8e-44, the inputs +-1e-40 and gradients
              below the normal range may be flushed or lose bits; none of that exceeds the smallest normal number.
  cut         torch's softplus returns z beyond 20; the function differs from z by log1p(exp(-20)) < CUT = 2.1e-9 there
              (its backward by 1 - sigmoid(20) < CUT): added where z > 20.
  shift       a result computed at a d that is off by d_err (the reference's fp32 mean of `other` against the fp64 mean
              rounded once: MEAN err = (n_sum + 1) u mean|other|, plus the subtraction's u |d|): d_err |l'| on l, and
              d_err max|l''| on l' (1/4 for BCE and SOFTPLUS, 2 for LS, 0 for LINEAR; HINGE's derivative is a step --
              the inputs keep every 1 + s d more than an ulp from 0, tests/gan_cases.py).
  loss        |w| (mean of the element bounds + n_sum u mean|l|) + 3 u |L|: n_sum = 4 ceil(log2 n) + 64 additions on one
              element's path in a cascade summation in blocks of 16 (torch's CPU reduction; the kernels add in fp64),
              and three roundings of the result (the division by n, the weight, the cast).
  gradient    |c| (element bound of l') + 3 u |grad| + TINY, c = upstream w / n (its two products and the product with
              l' are the three roundings); through a mean: |c| (sum of the element bounds + n_sum u sum|l'|) / n_o +
              3 u |grad| + TINY; the generator's sum of the two one rounding more.

This is a worst-case envelope that catches structural errors (a wrong sign, label, shift, coefficient or a dropped
element); the shares the reference's fp32 results and the kernels use are recorded in profiles/gan_parity.txt.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
FN_U = 2
SIG_U = 5
TINY = 2.0 ** -126
CUT = 2.1e-9
D = torch.float64

BCE, LS, LINEAR, SOFTPLUS, HINGE = range(5)
KIND_NAMES = ("bce", "ls", "linear", "softplus", "hinge")


def _t(a):
    return torch.as_tensor(a).detach().to(D)


def fl32(v):
    """A Python float rounded to fp32 once."""
    return float(np.float32(v))


def spec(gan_type, target_is_real, is_disc=False, real_label_val=1.0, fake_label_val=0.0):
    """(kind, s, t) of one call of the criterion `gan_type` (basicsr's and KAIR's names, lower case)."""
    t = fl32(real_label_val if target_is_real else fake_label_val)
    toward = -1.0 if target_is_real else 1.0
    if gan_type in ("vanilla", "gan", "ragan"):
        return BCE, 1.0, t
    if gan_type == "lsgan":
        return LS, 1.0, t
    if gan_type == "wgan":
        return LINEAR, toward, 0.0
    if gan_type in ("wgan_softplus", "softplusgan"):
        return SOFTPLUS, toward, 0.0
    if gan_type == "hinge":
        return (HINGE, toward, 0.0) if is_disc else (LINEAR, -1.0, 0.0)
    raise KeyError(gan_type)


def delta(x, shift=None, exact=False):
    """d as fp64: the fp32 difference x - shift rounded once (x itself without a shift), or the fp64 one (exact)."""
    if shift is None:
        return _t(x)
    if exact:
        return _t(x) - _t(shift)
    return (torch.as_tensor(x).detach().to(torch.float32) - torch.as_tensor(shift, dtype=torch.float32)).to(D)


def mean_shift(other, exact=False):
    """The mean of `other`: fp64, rounded to fp32 once unless exact."""
    m = _t(other).mean()
    return m if exact else m.to(torch.float32).to(D)


def ell(d, kind, s, t):
    if kind == BCE:
        return d.clamp(min=0) - d * t + torch.log1p(torch.exp(-d.abs()))
    if kind == LS:
        return (d - t) ** 2
    if kind == LINEAR:
        return s * d
    z = s * d
    if kind == SOFTPLUS:
        return z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
    return (1 + z).clamp(min=0)


def dell(d, kind, s, t):
    if kind == BCE:
        return torch.sigmoid(d) - t
    if kind == LS:
        return 2 * (d - t)
    if kind == LINEAR:
        return torch.full_like(d, s)
    if kind == SOFTPLUS:
        return s * torch.sigmoid(s * d)
    return torch.where(1 + s * d <= 0, torch.zeros_like(d), torch.full_like(d, s))


def plain(x, sp, weight=1.0, upstream=1.0):
    """(L, upstream dL/dx) of L = w mean l(x)."""
    d = delta(x)
    return weight * ell(d, *sp).mean(), upstream * weight / d.numel() * dell(d, *sp)


def multiscale(xs, sp, weight=1.0, upstream=1.0):
    """The mean over the scales; of a list the last element counts.  (L, [dL/dx_k])."""
    xs = [x[-1] if isinstance(x, (list, tuple)) else x for x in xs]
    parts = [plain(x, sp, weight, upstream / len(xs)) for x in xs]
    return sum(p[0] for p in parts) / len(xs), [p[1] for p in parts]


def relativistic_term(pred, other, sp, weight=1.0, upstream=1.0, exact=False):
    """(L, dL/dpred, dL/dother, shift) of L = w mean l(pred - mean(other))."""
    m = mean_shift(other, exact)
    d = delta(pred, m, exact)
    dl = dell(d, *sp)
    c = upstream * weight / d.numel()
    n_o = torch.as_tensor(other).numel()
    return weight * ell(d, *sp).mean(), c * dl, torch.full(tuple(torch.as_tensor(other).shape), float(-c * dl.sum() / n_o),
                                                             dtype=D), m


def relativistic_generator(real, fake, sp_a, sp_b, weight=1.0, upstream=1.0, exact=False):
    """(L, dL/dreal, dL/dfake) of (term_A(real, fake) + term_B(fake, real)) / 2."""
    la, ga_r, ga_f, _ = relativistic_term(real, fake, sp_a, weight, upstream / 2, exact)
    lb, gb_f, gb_r, _ = relativistic_term(fake, real, sp_b, weight, upstream / 2, exact)
    return (la + lb) / 2, ga_r + gb_r, ga_f + gb_f


# ------------------------------------------------------------------------------------------------------- bounds ---
def n_sum(n):
    return 4 * math.ceil(math.log2(max(n, 2))) + 64


def mean_error(other):
    """What an fp32 mean of `other` may differ by from the fp64 mean rounded once."""
    o = _t(other)
    return (n_sum(o.numel()) + 1) * U * float(o.abs().mean())


def element_bounds(d, sp, shift_err=0.0):
    """Per-element bounds on l(d) and l'(d) of an fp32 evaluation; shift_err > 0: evaluated with a shift off by that
    much (and its own rounding of the subtraction)."""
    kind, s, t = sp
    d_err = shift_err + U * d.abs() if shift_err else torch.zeros_like(d)
    lv, dv = ell(d, *sp), dell(d, *sp)
    if kind == BCE:
        e = torch.exp(-d.abs())
        lp, sig = torch.log1p(e), torch.sigmoid(d)
        M = d.abs() + (d * t).abs() + ((1 - t) * d).abs() + lp
        bl = 4 * U * M + FN_U * U * lp + FN_U * U * e / (1 + e)
        bd = SIG_U * U * sig + U * dv.abs() + 0.25 * d_err
    elif kind == LS:
        bl = 3 * U * lv
        bd = 2 * U * dv.abs() + 2 * d_err
    elif kind == LINEAR:
        bl, bd = torch.zeros_like(d), torch.zeros_like(d)
    elif kind == SOFTPLUS:
        z = s * d
        cut = CUT * (z > 20).to(D)
        sig = torch.sigmoid(z)
        bl = U * lv + FN_U * U * lv + FN_U * U * sig + cut
        bd = SIG_U * U * sig + cut + 0.25 * d_err
    else:
        bl, bd = U * (1 + s * d).abs(), torch.zeros_like(d)
    return bl + d_err * dv.abs() + TINY, bd + TINY


def loss_bound(d, sp, weight=1.0, shift_err=0.0):
    bl, _ = element_bounds(d, sp, shift_err)
    lv = ell(d, *sp)
    return abs(weight) * (float(bl.mean()) + n_sum(d.numel()) * U * float(lv.abs().mean())) \
        + 3 * U * abs(weight) * abs(float(lv.mean()))


def grad_bound(d, sp, coef, shift_err=0.0):
    """Per element, for grad = coef l'(d), coef = upstream w / n."""
    _, bd = element_bounds(d, sp, shift_err)
    return abs(coef) * bd + 3 * U * abs(coef) * dell(d, *sp).abs() + TINY


def mean_path_bound(d, sp, coef, n_other, shift_err=0.0):
    """A scalar: for the constant -coef sum l'(d) / n_other that reaches every element of `other`."""
    _, bd = element_bounds(d, sp, shift_err)
    dv = dell(d, *sp)
    return abs(coef) * (float(bd.sum()) + n_sum(d.numel()) * U * float(dv.abs().sum())) / n_other \
        + 3 * U * abs(coef) * abs(float(dv.sum())) / n_other + TINY


def term_bounds(pred, other, sp, weight=1.0, upstream=1.0, reference_mean=False):
    """(loss bound, per-element bound on dL/dpred, scalar bound on dL/dother) of relativistic_term;
    reference_mean: the result was computed with an fp32 mean of `other` (the reference on the CPU)."""
    err = mean_error(other) if reference_mean else 0.0
    d = delta(pred, mean_shift(other))
    c = upstream * weight / d.numel()
    return (loss_bound(d, sp, weight, err), grad_bound(d, sp, c, err),
            mean_path_bound(d, sp, c, torch.as_tensor(other).numel(), err))


def generator_bounds(real, fake, sp_a, sp_b, weight=1.0, upstream=1.0, reference_mean=False):
    """(loss bound, per-element bounds on dL/dreal and dL/dfake) of relativistic_generator."""
    la, ba_r, ba_f = term_bounds(real, fake, sp_a, weight, upstream / 2, reference_mean)
    lb, bb_f, bb_r = term_bounds(fake, real, sp_b, weight, upstream / 2, reference_mean)
    L, gr, gf = relativistic_generator(real, fake, sp_a, sp_b, weight, upstream)
    return (la + lb) / 2 + 2 * U * abs(float(L)), ba_r + bb_r + U * gr.abs(), bb_f + ba_f + U * gf.abs()


def share(got, want, bound):
    """The largest share of the bound a result uses (0 / 0 counts as 0; anything / 0 as inf)."""
    d = (_t(got) - _t(want)).abs()
    b = _t(bound).expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    return float(r.max())


# ---- contents (shared by the fixture generator and the GPU cases; seeded) ----
def logits(shape, seed=0, mean=0.0):
    """N(mean, 3^2) fp32 logits."""
    g = torch.Generator().manual_seed(2000 + seed)
    return (mean + 3.0 * torch.randn(shape, generator=g, dtype=D)).to(torch.float32)


# ---- the fixture's cases (tests/golden/make_golden_gan.py writes them, tests/test_cpu_gan.py reads them) ----
BASICSR_TYPES = ("vanilla", "lsgan", "wgan", "wgan_softplus", "hinge")
KAIR_TYPES = ("gan", "ragan", "lsgan", "wgan", "softplusgan")
LABELS = ((1.0, 0.0), (0.9, 0.1))
FIXTURE_WEIGHT = 0.1          # the loss_weight of the reference's training files
REL_FORMS = ("gen_fake", "gen_both", "disc_real", "disc_fake")


def fixture_plain_cases():
    """(source, gan_type, target_is_real, is_disc, labels): basicsr's class with loss_weight FIXTURE_WEIGHT, KAIR's
    (which has neither is_disc nor a weight)."""
    cases = [("basicsr", t, real, disc, lab) for t in BASICSR_TYPES for real in (True, False) for disc in (False, True)
             for lab in LABELS]
    return cases + [("kair", t, real, False, lab) for t in KAIR_TYPES for real in (True, False) for lab in LABELS]


def fixture_rel_cases():
    """(source, gan_type, labels, form): the relativistic generator line with the gradient to fake alone (the models
    detach real) and to both, and the discriminator's two lines (x 0.5, the other tensor detached).  KAIR's lines take
    torch.mean(x, 0, True) of (B, 1) outputs, which is the scalar mean."""
    cases = [("basicsr", t, lab, form) for t in BASICSR_TYPES for lab in LABELS for form in REL_FORMS]
    return cases + [("kair", t, LABELS[0], form) for t in ("ragan", "lsgan") for form in REL_FORMS]


def fixture_inputs():
    """The fixture's fp32 inputs: x for the plain cases (specials in front), real / fake of different sizes for the
    relativistic ones, (B, 1) outputs for KAIR's lines, three scales."""
    x = logits((2, 1, 7, 5), 0)
    x.view(-1)[:6] = torch.tensor([0.0, 1.0, -1.0, 20.5, -100.0, 88.8])
    return dict(x=x, real=logits((2, 1, 7, 5), 1, 0.5), fake=logits((3, 1, 4, 4), 2, -0.5),
                kreal=logits((16, 1), 3, 0.5), kfake=logits((16, 1), 4, -0.5),
                s0=logits((2, 1, 5, 5), 5), s1=logits((2, 1, 3, 3), 6), s2=logits((2, 1, 2, 1), 7))


def rel_form(form, real, fake, term, generator):
    """One relativistic line on leaves `real`, `fake` (requires_grad set by the caller as the form says): `term(pred,
    other, target_is_real, is_disc)` and `generator(real, fake)` are the callables under test."""
    if form in ("gen_fake", "gen_both"):
        return generator(real, fake)
    if form == "disc_real":
        return term(real, fake.detach(), True, True) * 0.5
    return term(fake, real.detach(), False, True) * 0.5


def rel_needs(form):
    """(real requires grad, fake requires grad)"""
    return {"gen_fake": (False, True), "gen_both": (True, True), "disc_real": (True, False),
            "disc_fake": (False, True)}[form]
