"""Generated inputs that take the NIQE kernels (ssl_amd/csrc/ssg_niqe.hip) past the six blocks of the fixture, shared by
tests/test_cpu_niqe_blocks.py (what each case reaches, on the restatement alone) and tests/test_gpu_niqe_blocks.py (the
kernels against the restatement).  Everything is seeded numpy; no file is read but the kernels' own sources, for the
constants the shapes are derived from: the threads of a workgroup (niqe_fit's flag loop makes a second trip past them),
the lanes of a wave (rows whose flag is counted by wave 1) and the row lanes of the column means.

Planes are float32 (input_order 'HW', kind SSG_NIQE_F32_PLANE) holding integers, except `rgb`.

"Natural" content is a product of sinusoids plus Gaussian noise of sigma 8, clipped and rounded.  Flat parts are LEVEL 0
ONLY.  On a flat non-zero level I - mu is not 0 but the rounding noise of the window's last bit (the 49 weights do not
sum to exactly 1), and the signs that decide every feature of such a block are decided by whether the host's exp equals
numpy's in the last bit of the weights.  That would test the two libm's against each other, not the kernel.  On level 0
every product is 0 and I - mu is 0 whatever the weights are.  The same holds on PLANE 2 and on linear slopes: a 1-pixel
pattern of two levels is flat at their mean after the antialiased half, and a ramp equals its own window mean, so the
patterns below use iid lit levels and no ramp (pattern_planes).  tests/test_cpu_niqe_blocks.py holds every case to this:
one ulp on every weight of the window must not move its features.

"Black block b" is zeros over block b and MARGIN pixels around it, clipped to the plane: the 7 x 7 window (3 pixels)
and the resize taps of both scales (plane 2's window reaches 2 * 3 + 4 = 10 pixels of plane 1) stay inside the zeros.
Blocks are numbered column-major (bx, by = divmod(b, nbh)), as the kernel numbers its rows."""
import os
import re

import numpy as np

import niqe_reference as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = N.BS
MARGIN = 16


def _constant(header, name):
    text = open(os.path.join(ROOT, "ssl_amd", "csrc", header)).read()
    m = re.search(r"constexpr int " + name + r" = (\d+);", text)
    assert m, (header, name)
    return int(m.group(1))


NT = _constant("ssg_pixel.hpp", "NT")          # threads of a workgroup: trips of niqe_fit's flag loop
FL = _constant("ssg_niqe.hip", "FL")           # row lanes per column of niqe_fit's column means
WAVE = 64                                      # lanes of a wave (wave_good[] has NT / 64 entries)
assert _constant("ssg_niqe.hip", "NF") == N.NF and _constant("ssg_niqe.hip", "BS") == BS and NT % WAVE == 0

LANES_NBH, LANES_NBW = 2, FL // 2 + 1          # the fewest block columns of 2 rows with more blocks than row lanes
WAVES_NBH = 5
WAVES_BLACK = (3, WAVE + 2)                    # one black row counted by wave 0, one by wave 1
WAVES_NBW = WAVES_BLACK[1] // WAVES_NBH + 1    # the block column that holds row WAVE + 2
TRIPS_NBH = 3
TRIPS_NBW = (NT + 1) // TRIPS_NBH + 1          # the smallest 3-row plane with nblk > NT + 1: rows NT and NT + 1 exist
TRIPS_BLACK = (100, NT + 1)                    # one black row of the first trip, one of the second
PATTERN_BLOCKS = tuple((by, bx) for by in (0, 2) for bx in (0, 2, 4, 6))
PATTERN_NAMES = ("checker1", "vstripes", "hstripes", "checker2", "impulses", "lines", "binary", "black")

SEEDS = dict(lanes=2601, waves=2602, trips=2603, patterns=2604, two_good=2605, one_good=2606, dead_column=2607, rgb=2608,
             batch_natural=2609, batch_black=2610, batch_uniform=2611)


def natural(rng, H, W):
    """(H, W) float64 holding integers 0 .. 255."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 90 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 20 * np.sin((xx + yy) / 23.0)
    return np.clip(base + rng.normal(0, 8, (H, W)), 0, 255).round()


def region(H, W, nbh, b):
    """The slices of block b with its margin, clipped to the plane."""
    bx, by = divmod(b, nbh)
    return (slice(max(by * BS - MARGIN, 0), min((by + 1) * BS + MARGIN, H)),
            slice(max(bx * BS - MARGIN, 0), min((bx + 1) * BS + MARGIN, W)))


def blacken(p, b):
    p[region(p.shape[0], p.shape[1], p.shape[0] // BS, b)] = 0
    return p


def pattern_planes(rng, H, W):
    """The eight patterns over the whole plane, in PATTERN_NAMES' order.  The lit pixels of the 1- and 2-pixel patterns
    take iid levels 192 .. 255 over level 0, not one level: at scale 1 that changes no sign (a lit pixel lies above its
    window's mean, a dark one below), but the antialiased half of a two-level 1-pixel pattern is FLAT at the mean of the
    two levels, a flat non-zero level on plane 2 (see the header).  `lines` are wrap lines like those of a ramp (x + 2 y)
    mod 64 without its slopes, on level 0: on a linear slope I - mu is rounding noise just as on a flat level."""
    yy, xx = np.mgrid[0:H, 0:W]
    lit = rng.integers(192, 256, (H, W)).astype(np.float64)
    impulses = np.zeros((H, W))
    impulses.flat[rng.choice(H * W, 400, replace=False)] = 255
    return (lit * ((xx + yy) % 2), lit * (xx % 2), lit * (yy % 2),
            np.repeat(np.repeat(lit[::2, ::2], 2, 0), 2, 1)[:H, :W] * ((xx // 2 + yy // 2) % 2), impulses,
            255.0 * ((xx + 2 * yy) % 64 == 0), 255.0 * rng.integers(0, 2, (H, W)), np.zeros((H, W)))


def _plane(name):
    rng = np.random.default_rng(SEEDS.get(name, 0))
    if name == "lanes":
        return natural(rng, LANES_NBH * BS, LANES_NBW * BS)
    if name == "waves":
        p = natural(rng, WAVES_NBH * BS, WAVES_NBW * BS)
        for b in WAVES_BLACK:
            blacken(p, b)
        return p
    if name == "trips":
        p = natural(rng, TRIPS_NBH * BS, TRIPS_NBW * BS)
        for b in TRIPS_BLACK:
            blacken(p, b)
        return p
    if name == "patterns":
        H, W = 3 * BS, 7 * BS
        p = natural(rng, H, W)
        for (by, bx), q in zip(PATTERN_BLOCKS, pattern_planes(rng, H, W)):
            s = region(H, W, 3, bx * 3 + by)
            p[s] = q[s]
        return p
    if name == "two_good":                       # natural in block column 0 (rows 0 and 1), level 0 elsewhere
        p = natural(rng, LANES_NBH * BS, LANES_NBW * BS)
        p[:, BS:] = 0
        return p
    if name == "one_good":                       # natural in block 0 alone
        p = natural(rng, LANES_NBH * BS, LANES_NBW * BS)
        p[:, BS:] = 0
        p[BS:] = 0
        return p
    if name == "dead_column":
        return pattern_planes(np.random.default_rng(SEEDS[name]), BS, 2 * BS)[0]
    # the batch's other members, on `patterns`' shape
    if name == "batch_natural":
        return natural(rng, 3 * BS, 7 * BS)
    if name == "batch_black":
        return blacken(natural(rng, 3 * BS, 7 * BS), 10)
    if name == "batch_uniform":
        return rng.integers(0, 256, (3 * BS, 7 * BS)).astype(np.float64)
    raise KeyError(name)


RGB_SHAPE, RGB_CROP = (200, 492, 3), 4
PLANE_CASES = ("lanes", "waves", "trips", "patterns", "two_good", "one_good", "dead_column")
CASES = PLANE_CASES + ("rgb",)
BATCH = ("patterns", "batch_natural", "batch_black", "batch_uniform")
# name -> (blocks high, blocks wide)
BLOCKS = dict(lanes=(LANES_NBH, LANES_NBW), waves=(WAVES_NBH, WAVES_NBW), trips=(TRIPS_NBH, TRIPS_NBW), patterns=(3, 7),
              two_good=(LANES_NBH, LANES_NBW), one_good=(LANES_NBH, LANES_NBW), dead_column=(1, 2), rgb=(2, 5))
NAN_SCORE = ("one_good", "dead_column")

_CACHE = {}


def image(name):
    """(array, input_order, crop_border) as calculate_niqe takes it: a float32 (H,W) plane, or the uint8 HWC image."""
    if ("img", name) not in _CACHE:
        if name == "rgb":
            rng = np.random.default_rng(SEEDS[name])
            H, W, _ = RGB_SHAPE
            yy, xx = np.mgrid[0:H, 0:W]
            base = np.stack([128 + 90 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c) + 20 * np.sin((xx + yy) / 23.0)
                             for c in range(3)], -1)
            img = np.clip(base + rng.normal(0, 8, base.shape), 0, 255).round().astype(np.uint8)
            _CACHE["img", name] = (img, 'HWC', RGB_CROP)
        else:
            _CACHE["img", name] = (_plane(name).astype(np.float32), 'HW', 0)
        _CACHE["img", name][0].setflags(write=False)
    return _CACHE["img", name]


def restated(name, P):
    """The restatement's stages of a case (niqe_reference.niqe), computed once; P holds the pristine model."""
    if ("ref", name) not in _CACHE:
        img, order, crop = image(name)
        _CACHE["ref", name] = N.niqe(img, crop, P["mu_pris_param"], P["cov_pris_param"], order)
    return _CACHE["ref", name]
