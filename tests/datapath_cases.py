"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Inputs and case tables shared by tests/test_cpu_datapath.py and tests/test_gpu_datapath.py: the data-path kernels
(ssl_amd/csrc/ssg_datapath.hip, ssg_degrade.hip) beyond the fixture shapes.  Everything is seeded numpy / torch on
the CPU; the CPU module pins the properties the GPU module relies on (no USM tie, the Poisson level counts, the
filter2D kernels' norms, oracle = torch at the resize shapes), so the GPU module only compares.
"""
import functools

import numpy as np
import torch

from oracle import datapath_oracle as dp


def q8(rng, *shape):
    """Random multiples of 1/255 in [0, 1], float32."""
    return (np.round(rng.random(shape) * 255) / 255).astype(np.float32)


# ------------------------------------------------------------------ augment_crop ----
FLIPS8 = [(h, v, r) for r in (0, 1) for v in (0, 1) for h in (0, 1)]      # every (hflip, vflip, rot90)


def distinct_source(shape, dtype):
    """fp32: arange, every element distinct (exact below 2^24); uint8: arange mod 251 -- 251 is prime and divides no
    row or plane stride used here, so no neighbour, row-mate or transpose partner of an element holds its value."""
    n = int(np.prod(shape))
    if dtype == np.float32:
        assert n < 1 << 24
        return np.arange(n, dtype=np.float32).reshape(shape)
    return (np.arange(n, dtype=np.int64) % 251).astype(np.uint8).reshape(shape)


def corner_origins(flips, Hs, Ws, Ho, Wo, shift):
    """One (top, left) per sample on ITS augmented sample, all eight distinct: sample i takes kind (i + shift) % 8 of
    the four corners (0, 0), far, top-right, bottom-left and four interior origins that depend on i; over shift = 0..7
    every flip combination meets every corner."""
    out = []
    for i, (_, _, r) in enumerate(flips):
        Ha, Wa = (Ws, Hs) if r else (Hs, Ws)
        mt, ml = Ha - Ho, Wa - Wo
        assert mt > 2 * i + 2 and ml > i + 2
        out.append([(0, 0), (mt, ml), (0, ml), (mt, 0), (2 * i + 1, i + 1), (i + 1, ml - 1 - i), (mt - 1 - 2 * i, i + 1),
                    (mt - 1 - i, ml - 1 - i)][(i + shift) % 8])
    assert len(set(out)) == len(out)
    return out


def augment_crop_oracle(x, out_hw, top_left, flips):
    """dp.augment_crop_nchw sample by sample (it takes one origin)."""
    return np.concatenate([dp.augment_crop_nchw(x[b:b + 1], top_left[b][0], top_left[b][1], out_hw, [flips[b]])
                           for b in range(x.shape[0])])


# ------------------------------------------------------------------ pair pool ----
def pool_stream(b, steps=40):
    """`steps` incoming (lq (b,3,5,5) f32 = 300 B, gt (b,3,10,10) f32 = 1200 B, mask (b,1,10,10) u8 = 100 B) batches;
    every sample of the stream carries values no other sample has (its index in the first two mask bytes)."""
    out = []
    for t in range(steps):
        ids = np.arange(b) + t * b
        lq = (ids[:, None] * 75 + np.arange(75)[None]).astype(np.float32).reshape(b, 3, 5, 5)
        gt = (ids[:, None] * 300 + np.arange(300)[None] + 0.5).astype(np.float32).reshape(b, 3, 10, 10)
        mk = ((np.arange(100)[None] * 5 + ids[:, None]) % 251).astype(np.uint8)
        mk[:, 0], mk[:, 1] = ids % 256, ids // 256
        out.append((lq, gt, mk.reshape(b, 1, 10, 10)))
    return out


# ------------------------------------------------------------------ filter2D ----
FILTER_KS = list(range(1, 22, 2))


@functools.lru_cache(maxsize=None)
def filter_kernels(k, B=3):
    """(B,k,k) float32 per-sample kernels without axis or point symmetry, signed: 2.5 P - 1.5 N with P, N >= 0 of sum 1
    on disjoint random supports, so sum(taps) = 1 and sum|taps| = 4 (the sinc-like case of the 3e-6 bound).  k = 1 has
    the one tap 1."""
    rng = np.random.default_rng(1300 + k)
    if k == 1:
        return np.ones((B, 1, 1), np.float32)
    out = np.empty((B, k, k), np.float64)
    for b in range(B):
        m = rng.random((k, k)) < 0.5
        m.flat[0], m.flat[-1] = True, False                      # both supports non-empty
        P, N = rng.random((k, k)) * m, rng.random((k, k)) * ~m
        out[b] = 2.5 * P / P.sum() - 1.5 * N / N.sum()
    return out.astype(np.float32)


def filter_images(k):
    """[(tag, img)]: one past the 16 x 64 tile both ways, and the minimum legal side k // 2 + 1 in H and in W."""
    rng = np.random.default_rng(1400 + k)
    r = k // 2
    return [("17x65", q8(rng, 3, 2, 17, 65)), ("minH", q8(rng, 3, 2, r + 1, 37)), ("minW", q8(rng, 3, 2, 19, r + 1))]


# ------------------------------------------------------------------ USM ----
# (tag, taps, sigma, weight, threshold, shape, seed).  ksize 51 is the compile-time path (F12); everything here runs
# usm_pass<.., .., 0>.  Seeds and thresholds are those for which the fp64 oracle has no residual within 1e-3 / 255 of
# the threshold (test_cpu_datapath.py asserts it), so the mask is decided at fp32 and the 2e-6 bound applies.  The fixed
# tables are dyadic, so on multiples of 1/255 their residual x 255 is a multiple of 1/16 .. 1/1024: a threshold of x.03
# keeps every such residual clear of it.
USM_CASES = [
    ("t1_fixed", 1, 0.0, 0.5, 10.0, (1, 2, 20, 67), 7),
    ("t3_fixed", 3, 0.0, 0.7, 4.03, (1, 2, 20, 67), 7),
    ("t5_fixed", 5, 0.0, 0.5, 10.0, (1, 2, 20, 67), 7),
    ("t7_fixed", 7, 0.0, 0.5, 6.03, (1, 2, 20, 67), 7),
    ("t7_s1.1", 7, 1.1, 0.9, 10.0, (1, 2, 20, 67), 7),
    ("t31_17x150", 31, 0.0, 0.5, 10.0, (1, 1, 17, 150), 8),
    ("t31_100x17", 31, 0.0, 0.5, 10.0, (1, 1, 100, 17), 7),
    ("t63_32x32", 63, 0.0, 0.5, 10.0, (1, 1, 32, 32), 7),
    ("t63_33x40", 63, 0.0, 0.5, 10.0, (1, 1, 33, 40), 7),
    ("t63_70x131", 63, 2.5, 0.5, 7.0, (2, 3, 70, 131), 10),
] + [(f"t9_{h}x{w}", 9, 1.5, 0.8, 4.0, (1, 1, h, w), 7) for h in (63, 64, 65) for w in (127, 128, 129)] \
  + [(f"t31_{h}x{w}", 31, 0.0, 0.5, 12.0, (1, 1, h, w), 7) for h, w in ((63, 129), (64, 128), (65, 127))]


@functools.lru_cache(maxsize=None)
def usm_case(tag):
    """(img, kwargs of dp.usm_sharp, out64, residual64) of one USM case, computed once."""
    _, taps, sigma, weight, thr, shape, seed = next(c for c in USM_CASES if c[0] == tag)
    img = q8(np.random.default_rng(seed), *shape)
    kw = dict(radius=taps, sigma=sigma, weight=weight, threshold=thr)
    out, res, _ = dp.usm_sharp(img, return_parts=True, **kw)
    for a in (img, out, res):
        a.setflags(write=False)
    return img, kw, out, res


def usm_ties(res, threshold):
    """Residuals whose mask bit fp32 cannot decide: | |res| 255 - threshold | < 1e-3."""
    return int((np.abs(np.abs(res) * 255 - threshold) < 1e-3).sum())


def usm_sharp_fp32(img, radius, sigma, weight, threshold):
    """The same separable expression as dp.usm_sharp evaluated in float32 numpy (taps rounded once from fp64, like the
    kernel's): the yardstick for what fp32 can reach on a case."""
    f = np.float32
    img = np.asarray(img, f)
    k = dp.gaussian_kernel_1d(radius, sigma).astype(f)
    blur = dp.filter2d_reflect(img, k).astype(f)
    res = (img - blur).astype(f)
    mask = (np.abs(res) * f(255) > f(threshold)).astype(f)
    soft = dp.filter2d_reflect(mask, k).astype(f)
    sharp = np.clip(img + f(weight) * res, f(0), f(1)).astype(f)
    return (soft * sharp + (f(1) - soft) * img).astype(f)


# ------------------------------------------------------------------ interpolate ----
RESIZE_MODES = ("area", "bilinear", "bicubic")
RESIZE_CASES = [
    ("1x1", (2, 1, 1, 1), dict(size=(1, 1))),
    ("1x9_to_5x3", (2, 2, 1, 9), dict(size=(5, 3))),
    ("7x1_sf2.6", (2, 2, 7, 1), dict(scale_factor=2.6)),
    ("5x130_to_1x1", (1, 2, 5, 130), dict(size=(1, 1))),
    ("33x65_to_4x129", (2, 2, 33, 65), dict(size=(4, 129))),
    ("33x65_sf0.11", (2, 2, 33, 65), dict(scale_factor=0.11)),
    ("16x16_sf4", (1, 2, 16, 16), dict(scale_factor=4)),
    ("64x63_sf0.25", (1, 2, 64, 63), dict(scale_factor=0.25)),
    ("41x29_sf0.5x1.7", (2, 2, 41, 29), dict(scale_factor=(0.5, 1.7))),
    ("23x200_sf1/3", (1, 2, 23, 200), dict(scale_factor=1 / 3)),
    ("100x100_sf0.07", (1, 2, 100, 100), dict(scale_factor=0.07)),
    ("1025planes_sf1.5", (205, 5, 4, 6), dict(scale_factor=1.5)),       # 1,025 planes: the p += gridDim.z trip
] + [(f"to_{h}x{w}", (1, 2, 11, 97), dict(size=(h, w))) for h in (3, 4, 5) for w in (63, 64, 65)]


@functools.lru_cache(maxsize=None)
def resize_input(tag):
    i, shape = next((i, c[1]) for i, c in enumerate(RESIZE_CASES) if c[0] == tag)
    x = np.random.default_rng(1500 + i).random(shape, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def resize_refs(tag, mode):
    """(oracle fp32, torch CPU fp32) of one resize case."""
    kw = next(c[2] for c in RESIZE_CASES if c[0] == tag)
    x = resize_input(tag)
    o = dp.interpolate(x, mode=mode, dtype=np.float32, **kw)
    t = torch.nn.functional.interpolate(torch.from_numpy(x.copy()), mode=mode, **kw).numpy()
    return o, t


# ------------------------------------------------------------------ noise ----
POISSON_LEVELS = (1, 2, 3, 4, 5, 128, 129, 256)
POISSON_VALS = (1, 2, 4, 4, 8, 128, 256, 256)
POISSON_GRAY = (1, 0, 1, 0, 1, 0, 0, 1)


def poisson_level_batch(perturb, H=24, W=31, seed=1600):
    """(8,3,H,W) float32: sample s holds exactly POISSON_LEVELS[s] distinct levels.
    perturb False: r = g = b = level k, so the colour census and the gray census (0.9999 k rounds to k) both count
    POISSON_LEVELS[s].  perturb True: every second pixel becomes (k + 3, k - 1, k - 3) for 3 <= k <= 252 -- its gray
    level stays k (0.9999 k - 0.03), so the gray census still counts POISSON_LEVELS[s] while the colour census counts
    more: the two are then checked apart.  Values carry a sub-level jitter (|j| < 0.25 / 255, same level) and levels 0
    and 255 sit slightly outside [0, 1] on some pixels, where the level clamp applies."""
    rng = np.random.default_rng(seed + int(perturb))
    B, n_px = len(POISSON_LEVELS), H * W
    assert n_px >= 2 * 256
    lev = np.empty((B, 3, n_px), np.float64)
    for s, n in enumerate(POISSON_LEVELS):
        S = np.array([77]) if n == 1 else np.round(np.linspace(0, 255, n)).astype(np.int64)
        assert len(np.unique(S)) == n
        k = S[rng.permutation(n_px) % n]
        lev[s] = k[None]
        if perturb:
            sel = (np.arange(n_px) % 2 == 1) & (k >= 3) & (k <= 252)
            lev[s][:, sel] += np.array([3.0, -1.0, -3.0])[:, None]
    jit = rng.uniform(-0.25, 0.25, (B, 1, n_px))
    out = lev + jit
    edge = rng.random((B, 1, n_px)) < 0.5
    out = np.where(edge & (lev == 0), lev - rng.uniform(0.5, 8.0, (B, 1, n_px)), out)        # below 0
    out = np.where(edge & (lev == 255), lev + rng.uniform(0.5, 8.0, (B, 1, n_px)), out)      # above 1
    return (out / 255).astype(np.float32).reshape(B, 3, H, W)


def poisson_draws(rates, seed):
    """torch.poisson on the CPU, seeded: the draw the reference makes on these rates."""
    gen = torch.Generator().manual_seed(seed)
    return torch.poisson(torch.from_numpy(np.ascontiguousarray(rates)), generator=gen).numpy()


def clamp_round_input(n):
    """n float32 values over [-0.2, 1.2], the first 262 of them the half-integers (k + 1/2) / 255, k = -3 .. 258, where
    round-half-to-even decides."""
    v = np.linspace(-0.2, 1.2, n, dtype=np.float64)
    half = (np.arange(-3, 259) + 0.5) / 255
    v[:len(half)] = half
    return v.astype(np.float32)
