"""Inputs of the GAN criteria's GPU tests (tests/test_gpu_gan.py): shapes, contents, criterion configurations and the
relativistic pairs, with the condition the relativistic inputs must meet asserted here, on the CPU.

Shapes: the smallest at which the streaming kernels can go wrong.  A workgroup is WORKGROUP threads of PER_THREAD
elements a trip (one 16-byte load); `view67` is a 67-element view that starts one float into its buffer (a scalar head
of three, sixteen float4, no tail; the gradient buffer is aligned, so its stores go one by one); `trip` is
ssg_gan_grid_cap() * WORKGROUP * PER_THREAD + 5 elements, computed from the exported cap: every workgroup makes a second
trip and a tail remains (tests/test_cpu_gan.py ties trip_elements to the cap).
"""
import functools

import numpy as np
import torch

import gan_reference as R

WORKGROUP, PER_THREAD = 256, 4


def trip_elements(cap):
    return cap * WORKGROUP * PER_THREAD + 5


SHAPES = ("1x1", "16x1", "1x1x3x3", "2x1x7x5", "view67", "trip")
CONTENTS = ("normal", "special", "constant")


def _ulp(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


# 0, +-1 and +-20 with their fp32 neighbours (the hinge's corner, torch's softplus cut), +-88.8 (exp(88.8) overflows fp32:
# the naive forms give inf), +-100, a small normal and a subnormal magnitude
SPECIALS = torch.tensor(
    [0.0, 1.0, -1.0, _ulp(1, False), _ulp(-1, True), _ulp(1, True), _ulp(-1, False), 20.0, -20.0, _ulp(20, True),
     _ulp(20, False), _ulp(-20, True), _ulp(-20, False), 88.8, -88.8, 100.0, -100.0, 1e-30, -1e-30, 1e-40, -1e-40],
    dtype=torch.float64).to(torch.float32)


def shape_of(name, cap):
    if name == "view67":
        return (67,)
    if name == "trip":
        return (trip_elements(cap),)
    return tuple(int(v) for v in name.split("x"))


@functools.lru_cache(maxsize=None)
def content(name, shape, seed=0):
    """An fp32 CPU tensor.  'special': N(0, 3^2) with the special values first, last and from a 16-byte boundary in the
    middle; a tensor too small for three runs of them is filled with them alone, from a different start per size so
    that the small shapes together hold every one."""
    n = int(np.prod(shape))
    x = R.logits(shape, seed + n % 997)
    if name == "constant":
        x = torch.full(shape, 0.75)
    elif name == "special":
        k, flat = SPECIALS.numel(), x.view(-1)
        if n >= 3 * k:
            mid = (n // 2) // 4 * 4
            flat[:k], flat[mid:mid + k], flat[n - k:] = SPECIALS, SPECIALS, SPECIALS
        else:
            flat[:] = SPECIALS[(torch.arange(n) + {1: 1, 16: 0, 9: 12}.get(n, 0)) % k]
    return x


# (gan_type, labels, target_is_real, is_disc, upstream): every kind, sign and label of the kernels, through the module
CONFIGS = [(t, lab, real, disc, up)
           for t in ("vanilla", "lsgan")
           for lab, real, disc, up in (((1.0, 0.0), True, False, 1.0), ((1.0, 0.0), False, True, 0.5),
                                       ((0.9, 0.1), True, True, 1.0), ((0.9, 0.1), False, False, 0.5))] + \
          [("wgan", (1.0, 0.0), True, False, 0.5), ("wgan", (1.0, 0.0), False, True, 1.0),
           ("wgan_softplus", (1.0, 0.0), True, True, 0.5), ("wgan_softplus", (1.0, 0.0), False, False, 1.0),
           ("hinge", (1.0, 0.0), True, True, 1.0), ("hinge", (1.0, 0.0), False, True, 0.5),
           ("hinge", (1.0, 0.0), True, False, 0.5)]
WEIGHT = 0.3       # the modules' loss_weight: it must not reach a discriminator's term

# ---- relativistic pairs: (name, real shape name, fake shape name) and the forms ----
REL_PAIRS = (("sizes_differ", "2x1x7x5", "3x1x4x4"), ("16x1", "16x1", "16x1"), ("views", "view67", "view67"),
             ("trip", "trip", "1030"))
REL_TYPES = (("vanilla", (0.9, 0.1)), ("lsgan", (1.0, 0.0)), ("wgan", (1.0, 0.0)), ("wgan_softplus", (1.0, 0.0)),
             ("hinge", (1.0, 0.0)))
REL_FORMS = R.REL_FORMS + ("gen_real",)


def rel_needs(form):
    return (True, False) if form == "gen_real" else R.rel_needs(form)


def _mean_is_clear_of_a_rounding_boundary(x):
    """The fp64 mean of x lies further than 2^-53 sum|x| (n roundings of n 2^-53 sum|x| / n: what a different summation
    order can move it by) from the midpoint of two neighbouring fp32 values: every correct fp64 summation rounds to the
    same fp32 shift."""
    x64 = x.double()
    m = float(x64.mean())
    m32 = np.float32(m)
    half = float(np.spacing(np.abs(m32))) / 2
    return half - abs(m - float(m32)) > 2.0 ** -53 * float(x64.abs().sum())


def _hinge_is_clear_of_its_corner(pred, other):
    d = R.delta(pred, R.mean_shift(other))
    return all(bool(((1 + s * d).abs() > 2.0 ** -23 * d.abs().clamp(min=1)).all()) for s in (1.0, -1.0))


@functools.lru_cache(maxsize=None)
def rel_inputs(pair, cap):
    """(real, fake) fp32 CPU tensors of a relativistic pair, real around +0.5 and fake around -0.5; the condition on
    them is asserted, not measured: no element is left out of a comparison."""
    _, rs, fs = next(p for p in REL_PAIRS if p[0] == pair)
    shape = lambda s: (1030,) if s == "1030" else ((3, 1, 4, 4) if s == "3x1x4x4" else shape_of(s, cap))   # noqa: E731
    real, fake = R.logits(shape(rs), 11, 0.5), R.logits(shape(fs), 12, -0.5)
    assert _mean_is_clear_of_a_rounding_boundary(real) and _mean_is_clear_of_a_rounding_boundary(fake), pair
    assert _hinge_is_clear_of_its_corner(real, fake) and _hinge_is_clear_of_its_corner(fake, real), pair
    return real, fake
