"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

Inputs of the JPEG sweep (jpeg_kernel, ssl_amd/csrc/ssg_datapath.hip, behind ssg_diffjpeg / datapath.DiffJPEG), shared
by tests/test_cpu_jpeg.py, tests/test_gpu_jpeg.py and tests/golden/make_golden_jpeg.py (fixture F25: the reference's own
fp32 output for every case).  Small on purpose, seeded numpy, every value a multiple of 1/255.

  shapes      1 x 1, 15 x 17, 16 x 16, 17 x 15, 33 x 31, 32 x 48, 45 x 83: sides = 0, 1 and 15 mod 16, odd sides (there the
              2 x 2 chroma average reaches into the zero padding: a padded pixel's Cb and Cr are 128, not 0)
  content     synth.natural_like; random^2; flat grey patches, one odd level per macroblock and per 8 x 8 block (at
              quality 50 every luma DC quotient is then k + 1/2); flat saturated colour patches (three of the colours
              put the Cb DC quotient 6e-5 from k + 1/2 at quality 50); primaries with hard edges (the clamp to 0 / 255);
              a 1-pixel checkerboard; all-zero and all-one images
  quality     tensors [15, 49.5, 50, 88, 95] and [1, 10, 30, 99] -- distinct per sample, both branches of
              quality_to_factor and the value 50 itself; scalars 50, 30 (an int), 72.5, 72.3 and 95 (72.3 is no float32:
              the C ABI takes the scalar as `float` before its double arithmetic, the reference keeps a Python double)

Quality 100 is excluded: its factor is 0, and the reference itself divides by zero there.

tests/test_cpu_jpeg.py asserts on the oracle alone that no macroblock of any case holds more than
jpeg_reference.CAP undecided quotients, so that tests/jpeg_reference.jpeg_match leaves nothing out.  That is a property
of the input, and the seeds are chosen for it where it matters: at quality 99 the quotients reach 3,200, the fp32
deviation about 1e-3 and the window 4e-3 to 5e-3, and hard-edged primaries then put 2 to 9 quotients of a macroblock inside it
depending on the seed (2544: at most 2).
"""
import functools

import numpy as np

import jpeg_reference as jr

QA = np.array([15.0, 49.5, 50.0, 88.0, 95.0], np.float32)
QB = np.array([1.0, 10.0, 30.0, 99.0], np.float32)

SATURATED = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (245, 255, 20),
             (245, 255, 88), (244, 254, 2), (255, 128, 0), (0, 64, 255), (200, 0, 40)]
PRIMARIES = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0), (255, 255, 0), (0, 255, 255), (255, 0, 255)]


def _q8(a):
    return (np.rint(np.clip(a, 0, 1) * 255) / 255).astype(np.float32)


def natural(B, H, W, seed):
    from ssl_amd import synth
    return np.stack([synth.natural_like(seed + i, H, W, 0.15, 0.05) for i in range(B)]).astype(np.float32)


def random_sq(B, H, W, seed):
    return _q8(np.random.default_rng(seed).random((B, 3, H, W)) ** 2)


def _patches(B, H, W, side, colours):
    """One colour per side x side tile (row-major over the batch), colours (n, 3) in 0..255 cycled."""
    ny, nx = -(-H // side), -(-W // side)
    idx = (np.arange(B * ny * nx) % len(colours)).reshape(B, ny, nx)
    tiles = np.asarray(colours, np.float64)[idx]                                   # (B, ny, nx, 3)
    full = np.repeat(np.repeat(tiles, side, 1), side, 2)[:, :H, :W]
    return _q8(full.transpose(0, 3, 1, 2) / 255)


def grey_patches(B, H, W, side):
    """Flat grey tiles of odd levels 129, 131, ...: at quality 50 the luma DC quotient 8 (level - 128) / 16 of every
    whole tile is k + 1/2."""
    n = B * (-(-H // side)) * (-(-W // side))
    lev = 129 + 2 * (np.arange(n) % 63)
    return _patches(B, H, W, side, np.stack([lev] * 3, 1))


def saturated_patches(B, H, W, seed=0):
    return _patches(B, H, W, 16, SATURATED[seed % len(SATURATED):] + SATURATED[:seed % len(SATURATED)])


def primaries(B, H, W, seed):
    """Rectangles of pure primaries with hard edges at arbitrary pixel positions."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 3, H, W), np.float64)
    for b in range(B):
        x[b] = np.asarray(PRIMARIES[b % len(PRIMARIES)], np.float64)[:, None, None] / 255
        for _ in range(6):
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            h, w = rng.integers(1, max(H // 2, 2)), rng.integers(1, max(W // 2, 2))
            x[b, :, y0:y0 + h, x0:x0 + w] = np.asarray(PRIMARIES[rng.integers(len(PRIMARIES))], np.float64)[:, None, None] / 255
    return _q8(x)


def checkerboard(B, H, W):
    """1-pixel checkerboard, sample b between two colours of its own."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy + xx) % 2).astype(np.float64)
    pairs = [((0, 0, 0), (255, 255, 255)), ((255, 0, 0), (0, 255, 255)), ((10, 200, 30), (240, 60, 220)),
             ((0, 0, 255), (255, 255, 0)), ((128, 128, 128), (127, 127, 127))]
    out = [np.stack([m * c1 + (1 - m) * c0 for c0, c1 in zip(*pairs[b % len(pairs)])]) for b in range(B)]
    return _q8(np.stack(out) / 255)


def constant(B, H, W, v):
    return np.full((B, 3, H, W), v, np.float32)


# (tag, builder, quality).  A tensor quality fixes the batch (5 or 4 samples); scalar cases hold 2 samples.
_A, _B = len(QA), len(QB)
CASES = [
    ("natural_45x83_QA", lambda: natural(_A, 45, 83, 2500), QA),
    ("natural_33x31_QB", lambda: natural(_B, 33, 31, 2510), QB),
    ("natural_32x48_QB", lambda: natural(_B, 32, 48, 2520), QB),
    ("random2_1x1_QA", lambda: random_sq(_A, 1, 1, 2530), QA),
    ("random2_1x1_QB", lambda: random_sq(_B, 1, 1, 2531), QB),
    ("random2_15x17_QA", lambda: random_sq(_A, 15, 17, 2532), QA),
    ("random2_17x15_QB", lambda: random_sq(_B, 17, 15, 2533), QB),
    ("random2_16x16_QB", lambda: random_sq(_B, 16, 16, 2534), QB),
    ("random2_32x48_QA", lambda: random_sq(_A, 32, 48, 2535), QA),
    ("random2_33x31_QA", lambda: random_sq(_A, 33, 31, 2536), QA),
    ("grey_mb_32x48_q50", lambda: grey_patches(3, 32, 48, 16), 50),
    ("grey_mb_32x48_QA", lambda: grey_patches(_A, 32, 48, 16), QA),
    ("grey_mb_45x83_QB", lambda: grey_patches(_B, 45, 83, 16), QB),
    ("grey_8x8_16x16_q50", lambda: grey_patches(2, 16, 16, 8), 50),
    ("grey_8x8_33x31_q50", lambda: grey_patches(2, 33, 31, 8), 50),
    ("grey_8x8_17x15_QA", lambda: grey_patches(_A, 17, 15, 8), QA),
    ("saturated_32x48_QA", lambda: saturated_patches(_A, 32, 48, 6), QA),
    ("saturated_33x31_q50", lambda: saturated_patches(2, 33, 31, 6), 50),
    ("saturated_17x15_q95", lambda: saturated_patches(2, 17, 15, 3), 95),
    ("saturated_15x17_QB", lambda: saturated_patches(_B, 15, 17, 5), QB),
    ("primaries_33x31_QB", lambda: primaries(_B, 33, 31, 2544), QB),
    ("primaries_45x83_q30", lambda: primaries(2, 45, 83, 2541), 30),
    ("primaries_16x16_QA", lambda: primaries(_A, 16, 16, 2542), QA),
    ("checker_16x16_QA", lambda: checkerboard(_A, 16, 16), QA),
    ("checker_15x17_QB", lambda: checkerboard(_B, 15, 17), QB),
    ("checker_33x31_q72.5", lambda: checkerboard(2, 33, 31), 72.5),
    ("zero_17x15_QB", lambda: constant(_B, 17, 15, 0.0), QB),
    ("zero_16x16_QA", lambda: constant(_A, 16, 16, 0.0), QA),
    ("one_15x17_QA", lambda: constant(_A, 15, 17, 1.0), QA),
    ("one_32x48_QB", lambda: constant(_B, 32, 48, 1.0), QB),
    ("one_1x1_q50", lambda: constant(2, 1, 1, 1.0), 50),
    ("natural_33x31_q50", lambda: natural(2, 33, 31, 2550), 50),
    ("natural_33x31_q30", lambda: natural(2, 33, 31, 2550), 30),
    ("natural_33x31_q72.5", lambda: natural(2, 33, 31, 2550), 72.5),
    ("natural_33x31_q72.3", lambda: natural(2, 33, 31, 2550), 72.3),
    ("natural_33x31_q95", lambda: natural(2, 33, 31, 2550), 95),
    ("random2_15x17_q72.3", lambda: random_sq(2, 15, 17, 2560), 72.3),
    ("random2_17x15_q30", lambda: random_sq(2, 17, 15, 2561), 30),
]
TAGS = [c[0] for c in CASES]
assert len(set(TAGS)) == len(TAGS)


@functools.lru_cache(maxsize=None)
def case(tag):
    """(x (B,3,H,W) float32 read-only, quality: (B,) float32 read-only, or a Python int / float)."""
    _, build, quality = next(c for c in CASES if c[0] == tag)
    x = build()
    assert x.dtype == np.float32 and np.array_equal(x, (np.rint(x.astype(np.float64) * 255) / 255).astype(np.float32))
    x.setflags(write=False)
    if np.ndim(quality):
        quality = quality.copy()
        quality.setflags(write=False)
        assert x.shape[0] == len(quality)
    return x, quality


@functools.lru_cache(maxsize=None)
def oracle(tag):
    """The JpegOracle of a case (fp64 output, window, undecided quotients), computed once per session."""
    return jr.JpegOracle(*case(tag))
