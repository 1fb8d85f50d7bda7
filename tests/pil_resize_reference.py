"""numpy restatement of Pillow's 8-bit convolution resize (libImaging's ImagingResample with box=None and
reducing_gap=None): the oracle of ssl_amd/csrc/ssg_resample.hip and of ssl_amd/prep.py.

For one axis: scale = in / out, fs = max(scale, 1), support = S fs, ksize = 2 ceil(support) + 1; per output index the
window [xmin, xmin + n) around center = (xx + 0.5) scale, the weights f((i + xmin - center + 0.5) (1 / fs)) normalised
by their sum in index order (all fp64, math.sin / math.cos: the C library's, as Pillow's C code), fixed to 22 fractional
bits with C's truncation; a pass is clip8((2^21 + sum px k) >> 22) on integers.  Columns first, into bytes; rows from
those bytes; a pass whose axis keeps its size is not run.  The result is Pillow's byte for byte (tests/test_cpu_prep.py
holds it to Pillow itself)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
FILTERS = {'lanczos': 1, 'bilinear': 2, 'bicubic': 3, 'box': 4, 'hamming': 5}      # Pillow's Image.Resampling numbers
SUPPORT = {'lanczos': 3.0, 'bilinear': 1.0, 'bicubic': 2.0, 'box': 0.5, 'hamming': 1.0}
_F054, _F046 = float(np.float32(0.54)), float(np.float32(0.46))                    # the C source writes 0.54f, 0.46f


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def filter_value(name, x):
    if name == 'lanczos':
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    if name == 'box':
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    x = abs(x)
    if name == 'bilinear':
        return 1.0 - x if x < 1.0 else 0.0
    if name == 'bicubic':
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if name == 'hamming':
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (_F054 + _F046 * math.cos(x))
    raise ValueError(name)


def ksize(insz, outsz, name):
    fs = max(insz / outsz, 1.0)
    return int(math.ceil(SUPPORT[name] * fs)) * 2 + 1


def table(insz, outsz, name):
    """(bounds (out, 2) int32 {xmin, n}, coef (out, ksize) int32)."""
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    ss = 1.0 / fs
    ks = ksize(insz, outsz, name)
    bounds = np.zeros((outsz, 2), np.int32)
    coef = np.zeros((outsz, ks), np.int32)
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), insz) - xmin
        w = [filter_value(name, (i + xmin - center + 0.5) * ss) for i in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for i, v in enumerate(w):                              # int(): C's truncation toward zero
            coef[xx, i] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    return bounds, coef


def _pass(img, outsz, axis, name):
    x = np.moveaxis(img, axis, 0)
    bounds, coef = table(x.shape[0], outsz, name)
    out = np.empty((outsz,) + x.shape[1:], np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        acc = np.tensordot(coef[xx, :n].astype(np.int64), x[xmin:xmin + n].astype(np.int64), axes=1)
        acc = (acc + (1 << (PRECISION_BITS - 1))).astype(np.int32)      # the sum stays inside int32 (checked by the cast)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size, resample='lanczos'):
    """img uint8 (H,W) or (H,W,C); size (w, h) as Pillow orders it."""
    w, h = size
    x = np.asarray(img)
    assert x.dtype == np.uint8
    if x.shape[1] != w:
        x = _pass(x, w, 1, resample)
    if x.shape[0] != h:
        x = _pass(x, h, 0, resample)
    return np.ascontiguousarray(x)


def content(kind, h, w, c, seed=0):
    """Test images: 'random', 'const255', 'checker', 'blocks' (4 x 4 blocks of 0 / 255: both ends of the clip)."""
    rng = np.random.default_rng(seed)
    if kind == 'random':
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    elif kind == 'const255':
        a = np.full((h, w, c), 255, np.uint8)
    elif kind == 'checker':
        a = (((np.arange(h)[:, None] + np.arange(w)[None]) & 1) * 255).astype(np.uint8)[..., None].repeat(c, 2)
    elif kind == 'blocks':
        b = rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4, c), dtype=np.uint8) * 255
        a = np.kron(b, np.ones((4, 4, 1), np.uint8))[:h, :w]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a)
