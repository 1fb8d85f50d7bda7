"""The inputs of the metric tests (test_cpu_metrics.py holds the restatement's two summation orders to its bound on
them, test_gpu_metrics.py the kernels to the restatement): built once, seeded, and never changed by a test.

A case is two image batches in the layout of its input kind plus (crop_border, test_y_channel).  Shapes are named by
their size AFTER the crop; the kernel's map tile is 32 x 16 (W x H) and the map is 10 smaller than the cropped image:
  11 x 11    one map pixel                     12 x 27    a partial tile
  27 x 43    one tile plus one on each axis    45 x 79    two tiles plus a remainder on each axis
  270 x 403  with 3 planes 17 x 13 x 3 = 663 tiles: more than the 512 workgroups an image gets, so a second trip
  379 x 740  24 x 23 = 552 tiles in ONE plane, ragged on both axes: the second trip of a Y plane, where the fp64 sum of
             squared differences is carried from a workgroup's first tile to its second
"""
import collections
import functools
import itertools

import numpy as np

import metrics_reference as R

F32_RGB, U8_HWC, U8_CHW = 0, 1, 2
KIND_NAMES = {F32_RGB: "f32", U8_HWC: "hwc", U8_CHW: "chw"}

Case = collections.namedtuple("Case", "name kind crop y a b")


def layout(q, kind):
    """uint8 (B,H,W,C) BGR -> the array an input kind takes (f32: the RGB tensor q / 255)."""
    if kind == U8_HWC:
        return np.ascontiguousarray(q)
    if kind == U8_CHW:
        return np.ascontiguousarray(q.transpose(0, 3, 1, 2))
    return np.ascontiguousarray(q[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)


def images(case, which):
    """The case's images as the restatement takes them: a list of uint8 (H,W,C) BGR."""
    x = case.a if which == 0 else case.b
    if case.kind == U8_HWC:
        return list(x)
    if case.kind == U8_CHW:
        return [np.ascontiguousarray(i.transpose(1, 2, 0)) for i in x]
    return [R.quantise(i) for i in x]


def _noise(rng, B, H, W, C, amp=12):
    b = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    a = np.clip(b.astype(np.int32) + rng.integers(-amp, amp + 1, b.shape), 0, 255).astype(np.uint8)
    return a, b


def tie_values():
    """Every float32 x = fl32((2k + 1) / 510) whose fp32 product x * 255.0f is exactly k + 0.5: the quantiser's ties."""
    k = np.arange(255, dtype=np.float64)
    x = ((2 * k + 1) / 510).astype(np.float32)
    hit = (x * np.float32(255.0)).astype(np.float64) == k + 0.5
    return x[hit]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(2424)
    out = []

    def add(name, kind, crop, y, a, b):
        out.append(Case(name, kind, crop, bool(y), a, b))

    def noise(name, kind, B, C, hc, wc, crop, y):
        a, b = _noise(rng, B, hc + 2 * crop, wc + 2 * crop, C)
        add(name, kind, crop, y, layout(a, kind), layout(b, kind))

    noise("one_map_pixel", U8_HWC, 1, 3, 11, 11, 0, True)
    noise("crop_leaves_11", U8_HWC, 3, 3, 11, 11, 10, True)
    noise("crop_leaves_11_rgb", U8_CHW, 1, 3, 11, 11, 7, False)
    noise("tile_plus_one", U8_CHW, 1, 3, 27, 43, 4, False)
    noise("two_tiles_remainder_grey", U8_HWC, 1, 1, 45, 79, 0, False)
    noise("many_tiles_second_trip", U8_CHW, 1, 3, 270, 403, 0, False)
    # every kind x C x y x B at 12 x 27 after a crop of 4
    for kind, C, y, B in itertools.product((F32_RGB, U8_HWC, U8_CHW), (1, 3), (False, True), (1, 3)):
        noise(f"cross_{KIND_NAMES[kind]}_c{C}_y{int(y)}_b{B}", kind, B, C, 12, 27, 4, y)
    # floats beyond [0, 1] (clamped by the quantiser) and between the quantisation levels
    gt = rng.random((3, 3, 35, 51), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
    sr = gt + np.float32(0.04) * rng.standard_normal(gt.shape).astype(np.float32)
    add("floats_outside_unit", F32_RGB, 4, True, sr, gt)
    gt = rng.random((1, 1, 45, 79), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
    sr = gt + np.float32(0.04) * rng.standard_normal(gt.shape).astype(np.float32)
    add("floats_outside_unit_grey", F32_RGB, 0, True, sr, gt)
    # the quantiser's ties: half to even, not half up
    t = tie_values()
    assert t.size >= 8
    n = 3 * 16 * 18
    a = np.resize(t, n).reshape(1, 3, 16, 18)
    b = np.resize(t[::-1], n).reshape(1, 3, 16, 18)
    add("round_half_even_ties", F32_RGB, 0, False, a.copy(), b.copy())
    add("round_half_even_ties_y", F32_RGB, 0, True, a.copy(), b.copy())
    # a flat plane: the cancellation worst case of E[x^2] - mu^2
    fa, fb = np.full((1, 27, 43, 3), 255, np.uint8), np.full((1, 27, 43, 3), 254, np.uint8)
    add("flat_255_254", U8_HWC, 0, False, fa, fb)
    add("flat_255_254_y", U8_CHW, 4, True, layout(fa, U8_CHW), layout(fb, U8_CHW))
    # a 0 / 255 checkerboard against its inverse and against noise
    yy, xx = np.mgrid[0:35, 0:51]
    cb = np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], (1, 35, 51, 3))
    add("checkerboard_inverse", F32_RGB, 4, True, layout(cb, F32_RGB), layout(255 - cb, F32_RGB))
    na, _ = _noise(rng, 1, 35, 51, 3)
    add("checkerboard_noise", U8_HWC, 0, False, np.ascontiguousarray(cb), na)
    # SR equal to GT: PSNR inf, SSIM 1
    a, _ = _noise(rng, 3, 20, 35, 3)
    add("identical", U8_HWC, 4, True, a, a.copy())
    a, _ = _noise(rng, 1, 20, 35, 3)
    add("identical_rgb_f32", F32_RGB, 0, False, layout(a, F32_RGB), layout(a, F32_RGB))
    # past 512 tiles: in one Y plane (three channels, then grey), and with three different images in the batch, so that
    # image i's partial sums lie at i * 512 in each of the workspace's three regions
    noise("y_second_trip", U8_HWC, 2, 3, 379, 740, 4, True)
    noise("grey_y_second_trip", U8_CHW, 1, 1, 379, 740, 0, True)
    noise("batch_second_trip", F32_RGB, 3, 3, 270, 403, 0, False)
    return tuple(out)


def geometry(case):
    """(B, C, H, W) of a case."""
    if case.kind == U8_HWC:
        B, H, W, C = case.a.shape
    else:
        B, C, H, W = case.a.shape
    return B, C, H, W


def tiles(case):
    """The 32 x 16 map tiles of one image of a case: planes x tile rows x tile columns."""
    _, C, H, W = geometry(case)
    hm, wm = H - 2 * case.crop - 10, W - 2 * case.crop - 10
    return (1 if case.y else C) * ((hm + 15) // 16) * ((wm + 31) // 32)


@functools.lru_cache(maxsize=None)
def reference(index):
    """The restatement's results for case `index`, one dict per image (metrics_reference.metrics)."""
    case = cases()[index]
    return tuple(R.metrics(a, b, case.crop, case.y) for a, b in zip(images(case, 0), images(case, 1)))
