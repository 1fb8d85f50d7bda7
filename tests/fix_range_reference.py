"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

fp64 reference for the RANGE of the deterministic gradient's fixed-point conversion (ssl_amd/csrc/ssg_common.hpp:
grad_fix_scale_of, fix_round, grad_add / grad_add_wide), shared by tests/test_cpu_fix_range.py and
tests/test_gpu_fix_range.py.

The deterministic backward rounds every contribution v to round(v * scale) and adds 64-bit integers; the scale puts
|G|max * scale into [2^35, 2^36) (|G| = |dL/dD|).  How far a single converted value reaches beyond |G|max is a
property of the KERNEL that forms it: the direct kernels convert per-row terms, the dense-tile backward converts a sum
over all edge pixels of a tile and all offset rows its wave owns.  `tile_reach` computes exactly that sum on the CPU
oracle, tile by tile and offset-row range by offset-row range, so that a test can show ON THE REFERENCE how many bits an
input needs before the GPU is involved.

Everything here restates the device's rules (scale, wave slots, offset-row split) instead of importing them: a change
of the rule in the library has to be made here as well, on purpose.
"""
import math

import numpy as np

from oracle import ssg_oracle as orc

QSPLIT_AUTO_MAX = 5     # ssg_bwd_dense.hip: offset-row parts the grid carries per tile when the device chooses
CASE_SEED = 0           # seed of the committed cases (control_pair / embedded_case; the reaches are re-measured on it)
FIX_BITS = 35           # grad_fix_scale_of: |G|max * scale in [2^35, 2^36) when the bound is the exact maximum


# ---------------------------------------------------------------------------------------------- device rules ----
def fix_scale(bound):
    """Scale of the fixed-point sums for a bound of |G| (a non-negative float32): with the bound's biased exponent e
    (bound < 2^(e-126)), clamped at 40 from below, scale = 2^(35 - (e - 127))."""
    bits = int(np.asarray(bound, np.float32).view(np.uint32))
    e = max((bits >> 23) & 0xFF, 40)
    return math.ldexp(1.0, FIX_BITS - (e - 127))


def tile_rows(ks):
    """Rows of a dense tile (32 columns): 4 at k_s = 49, 8 otherwise."""
    return 4 if ks == 49 else 8


def waves_per_tile(ks):
    """NHALF of the dense backward: one wave covers the 16 halo-grown rows of a 4 x 32 tile, two share an 8 x 32 tile."""
    return 1 if ks == 49 else 2


def wave_slots(cus, ks):
    """Wave slots of the device for the dense backward: CUs x 4 SIMDs x (one wave per SIMD at k_s = 49, two otherwise)."""
    return cus * 4 * (1 if ks == 49 else 2)


def offset_parts(n_dense_tiles, cus, ks):
    """Offset-row parts per tile (`qs`) the dense backward chooses on the device for this many dense tiles."""
    want = wave_slots(cus, ks) // (max(n_dense_tiles, 1) * waves_per_tile(ks))
    return min(max(want, 1), QSPLIT_AUTO_MAX)


def tiles_for_one_part(cus, ks):
    """Smallest dense-tile count from which on offset_parts() == 1."""
    n = wave_slots(cus, ks) // (2 * waves_per_tile(ks)) + 1
    assert offset_parts(n, cus, ks) == 1 and (n == 1 or offset_parts(n - 1, cus, ks) > 1)
    return n


# ---------------------------------------------------------------------------------------------------- inputs ----
def step_edge_pair(H, W, seed, contrast=0.8, noise=0.01):
    """(sr, gt), each (3, H, W) float32: gt a vertical step edge (0 | 1 at W / 2) plus Gaussian noise, sr the same edge
    at `contrast` around 0.5 plus noise of its own -- ordinary [0,1] content whose SSG rows are coherent over a whole
    tile (every edge pixel of a tile sees the edge on the same side)."""
    rng = np.random.default_rng(seed)
    step = np.zeros((3, H, W))
    step[:, :, W // 2:] = 1.0
    gt = step + noise * rng.standard_normal((3, H, W))
    sr = 0.5 + contrast * (gt - 0.5) + noise * rng.standard_normal((3, H, W))
    return sr.astype(np.float32), gt.astype(np.float32)


def filler_mask(H, W, block, ks=49, seed=0):
    """(H, W) float32 mask: fully dense on `block` = (y0, x0, h, w), which must lie on the dense-tile grid of k_s; every
    other tile carries exactly ONE edge pixel at a seeded position inside it, so that with dense threshold 1 every tile
    of the image is a dense tile while the oracle sees few rows."""
    TY, TX = tile_rows(ks), 32
    y0, x0, h, w = block
    assert y0 % TY == 0 and x0 % TX == 0 and h % TY == 0 and w % TX == 0 and y0 + h <= H and x0 + w <= W
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.float32)
    m[y0:y0 + h, x0:x0 + w] = 1
    for ty in range(0, H, TY):
        for tx in range(0, W, TX):
            if y0 <= ty < y0 + h and x0 <= tx < x0 + w:
                continue
            m[ty + rng.integers(min(TY, H - ty)), tx + rng.integers(min(TX, W - tx))] = 1
    return m


SURROUND = 30           # halo of (49,13): the step edge continues this far around the block of embedded_case


def control_pair(seed):
    """The 32 x 96 block of embedded_case on its own: the centre of step_edge_pair(92, 156, seed), edge at column 48."""
    sr, gt = step_edge_pair(32 + 2 * SURROUND, 96 + 2 * SURROUND, seed)
    c = (slice(None), slice(SURROUND, SURROUND + 32), slice(SURROUND, SURROUND + 96))
    return np.ascontiguousarray(sr[c]), np.ascontiguousarray(gt[c])


def embedded_case(ks, cus, seed, min_tiles=None):
    """The step-edge block inside an image with more dense tiles than the device splits: (sr, gt, mask, block, tiles).

    The image is W = 512 (k_s 49) or 1,024 (otherwise) wide and as many tile rows high as `min_tiles` (default: the
    smallest count with offset_parts() == 1) needs.  The mask is dense on a 32 x 96 block on the tile grid, at least 30
    pixels from every border, and holds one pixel in every other tile (filler_mask).  The images hold
    step_edge_pair(92, 156, seed) around the block -- the edge runs through the block's middle and continues through
    its halo, as it does around an interior tile of a full-size image -- and low-contrast noise around 0.5 elsewhere."""
    TY, TX = tile_rows(ks), 32
    W = 512 if ks == 49 else 1024
    need = tiles_for_one_part(cus, ks) if min_tiles is None else min_tiles
    ty_n = max(-(-need // (W // TX)), -(-(32 + 2 * 32) // TY))
    H = ty_n * TY
    y0, x0 = (H // 2 - 16) // TY * TY, W // 2 - 64
    s = SURROUND
    assert min(y0, x0, H - y0 - 32, W - x0 - 96) >= s
    rng = np.random.default_rng(seed + 1)
    gt = 0.5 + 0.02 * rng.standard_normal((3, H, W))
    sr = gt + 0.01 * rng.standard_normal((3, H, W))
    bsr, bgt = step_edge_pair(32 + 2 * s, 96 + 2 * s, seed)
    sr[:, y0 - s:y0 + 32 + s, x0 - s:x0 + 96 + s] = bsr
    gt[:, y0 - s:y0 + 32 + s, x0 - s:x0 + 96 + s] = bgt
    block = (y0, x0, 32, 96)
    mask = filler_mask(H, W, block, ks, seed + 2)
    return sr.astype(np.float32), gt.astype(np.float32), mask, block, ty_n * (W // TX)


# ----------------------------------------------------------------------------------------------------- reach ----
def loss_reference(sr, gt, mask, ks, kw, sigma, w_l1, w_kl, want_grad=True):
    """orc.ssg_loss in fp64 for one image (sr, gt (3,H,W), mask (H,W)) plus what the reach needs: `pos` (N,2) and
    `gD` (N, k_s, k_s) = dL/dD of the sr rows, the G the backward kernels distribute.  want_grad=False leaves the image
    gradient out (a third of the time)."""
    sr64, gt64 = np.asarray(sr, np.float64), np.asarray(gt, np.float64)
    ref = orc.ssg_loss(sr64[None], gt64[None], mask[None], ks, kw, sigma, w_l1, w_kl, want_grad=want_grad)
    _, _, g = orc.criteria(ref["s_sr"], ref["s_gt"], w_l1, w_kl, want_grad=True)
    ref["pos"] = orc.mask_to_pos(mask)
    ref["gD"] = orc.ssg_epilogue_backward(ref["s_sr"], g, ks, kw, sr64.shape[0], sigma, True)
    return ref


def tile_reach(sr, gD, pos, ks, kw, TY, TX, parts):
    """max |partial| / |G|max over every dense tile (TY x TX grid cells holding a row of `pos`) and every one of `parts`
    contiguous offset-row ranges [(ks*k)//parts, (ks*(k+1))//parts): `partial` is orc.distance_backward of the tile's
    rows alone with the other offset rows of gD zeroed -- the image-gradient sum one wave of the dense backward forms
    before its single conversion.  (Evaluated on the tile's neighbourhood, cut at the image borders where the reflect
    folds happen: the rows reach no further than the halo, so the values are those of the whole image.)"""
    sr = np.asarray(sr, np.float64)
    gD = np.asarray(gD, np.float64).reshape(len(pos), ks, ks)
    _, H, W = sr.shape
    halo = ks // 2 + kw // 2
    gmax = np.abs(gD).max()
    key = (pos[:, 0] // TY) * ((W + TX - 1) // TX) + pos[:, 1] // TX
    worst = 0.0
    for t in np.unique(key):
        rows = np.flatnonzero(key == t)
        ty0, tx0 = int(pos[rows[0], 0]) // TY * TY, int(pos[rows[0], 1]) // TX * TX
        ya, yb = max(0, ty0 - halo), min(H, ty0 + TY + halo)
        xa, xb = max(0, tx0 - halo), min(W, tx0 + TX + halo)
        crop = np.ascontiguousarray(sr[:, ya:yb, xa:xb])
        p = pos[rows] - np.array([ya, xa], np.int32)
        for k in range(parts):
            g = np.zeros((len(rows), ks, ks))
            lo, hi = (ks * k) // parts, (ks * (k + 1)) // parts
            g[:, lo:hi] = gD[rows, lo:hi]
            worst = max(worst, float(np.abs(orc.distance_backward(crop, p, ks, kw, g)).max()))
    return worst / gmax


def reach_bits(reach):
    """Lower end of log2 |v * scale| of the largest converted value when the bound of |G| is exact: |G|max * scale is at
    least 2^35.  Up to 1 more by where |G|max falls in its binade, up to 1 less for a bound that is 2x loose."""
    return math.log2(reach) + FIX_BITS
