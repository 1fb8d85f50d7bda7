"""BSRGAN's degradation chain on the GPU, for a batch of images of differing sizes at once.

The reference is GAN-Based-SR/train_BSGRAN/utils/utils_blindsr.py (`degradation_bsrgan` :443-530, `_nocrop` :532-616,
`_ours_p` :618-706, `_plus` :708-792 and the stages they call), run once per sample on the CPU by
data/dataset_blindsr.py, dataset_blindsrmask.py and dataset_blindsroursp.py.  Every image draws its own stage order
(`random.sample(range(7), 7)`) and its own intermediate sizes (`int(sf1 * w)`, the 1/2 pre-scale, `a / sf`), so neither
the batched kernels of `datapath` (one shape, one operation per launch) nor an image-by-image loop (some twelve tiny
launches per image) fit.  Here the decisions of every image are drawn on the host first, each image gets a PROGRAM of
stages with all sizes (`build_program`, pure host code), and the batch runs slot by slot with ONE launch per operation
family present in the slot: each image carries its own record (sizes, operation, parameters) in a device table
(ssl_amd/csrc/ssg_blindsr.hip, include/ssg_hip.h section (T)).

    host, fp64, numpy only   fspecial_gaussian, fspecial, anisotropic_Gaussian, gm_blur_kernel, shift_pixel
    one HWC image each       add_blur, add_resize, add_Gaussian_noise, add_speckle_noise, add_Poisson_noise,
                             add_sharpening (datapath.USMSharp), random_crop, random_crop_ours_p,
                             degradation_bsrgan, degradation_bsrgan_nocrop, degradation_bsrgan_ours_p,
                             degradation_bsrgan_plus      (names and arguments of utils_blindsr, plus `draws=`)
    the batch                BlindSRDegradation(sf, lq_patchsize, ...).feed(images)

Randomness.  The decisions come from python's `random` and `numpy.random` in the reference's call order (`BlindSRDraws`;
tests replay recorded ones).  The noise FIELDS come from the GPU's generator (`torch.randn`, `torch.poisson`); the
reference takes them from `numpy.random`'s global stream, on which its later decisions then depend, so equal seeds do
NOT reproduce the reference's decisions: the results are equal in distribution.  The correlated Gaussian mode applies
the factor `numpy.random.multivariate_normal` uses (the SVD one) to a standard-normal colour field.

`cv2.resize` is restated from OpenCV's rules (the header lists them); equality with cv2 itself is supposed, not verified.
`isp_model` is accepted and must be None, as every caller in the reference passes it.
"""
import math
import random
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .datapath import Draws, USMSharp, augment_crop, jpeg_roundtrip
from ._gpu import current_gpu, launch, on, ptr as _ptr

__all__ = ["fspecial_gaussian", "fspecial", "anisotropic_Gaussian", "gm_blur_kernel", "shift_pixel", "add_blur",
           "add_resize", "add_Gaussian_noise", "add_speckle_noise", "add_Poisson_noise", "add_sharpening", "add_JPEG_noise",
           "random_crop", "random_crop_ours_p", "degradation_bsrgan", "degradation_bsrgan_nocrop",
           "degradation_bsrgan_ours_p", "degradation_bsrgan_plus", "BlindSRDegradation", "BlindSRDraws", "Stage",
           "Program", "build_program", "ragged_apply"]

_K = _lib.CONSTANTS
CONV, RESIZE, NOISE = _K["SSG_BSR_CONV"], _K["SSG_BSR_RESIZE"], _K["SSG_BSR_NOISE"]
CLIP, LEAD_CLIP = _K["SSG_BSR_CLIP"], _K["SSG_BSR_LEAD_CLIP"]
NOISE_OPS = {name: _K["SSG_BSR_" + name] for name in
             ("GAUSS_COLOR", "GAUSS_GRAY", "GAUSS_CORR", "SPECKLE_COLOR", "SPECKLE_GRAY", "SPECKLE_CORR", "POISSON_RATES",
              "POISSON_COLOR", "POISSON_RATES_GRAY", "POISSON_GRAY")}
MAX_KERNEL = 9

# ssg_blindsr_record (include/ssg_hip.h)
_REC = np.dtype([("in_off", "<u4"), ("out_off", "<u4"), ("C", "<i4"), ("h", "<i4"), ("w", "<i4"), ("oh", "<i4"),
                 ("ow", "<i4"), ("op", "<i4"), ("stride", "<i4"), ("flags", "<i4"), ("pool_off", "<u4"),
                 ("field_off", "<u4"), ("p0", "<f4"), ("tile0", "<i4"), ("tiles_x", "<i4"), ("reserved", "<i4")])
assert _REC.itemsize == 64


# ------------------------------------------------------------------ the kernels: host, fp64, numpy only ----
def fspecial_gaussian(hsize, sigma):
    """utils_blindsr.py:188-199 (MATLAB's fspecial('gaussian', hsize, sigma))."""
    siz = (hsize - 1.0) / 2.0
    x, y = np.meshgrid(np.arange(-siz, siz + 1), np.arange(-siz, siz + 1))
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(float).eps * h.max()] = 0
    sumh = h.sum()
    return h / sumh if sumh != 0 else h


def fspecial(filter_type, *args, **kwargs):
    """utils_blindsr.py:211-219; the chain uses 'gaussian' only."""
    if filter_type == 'gaussian':
        return fspecial_gaussian(*args, **kwargs)
    if filter_type == 'laplacian':
        alpha = max(0, min(args[0] if args else kwargs['alpha'], 1))
        h1, h2 = alpha / (alpha + 1), (1 - alpha) / (alpha + 1)
        return np.array([[h1, h2, h1], [h2, -4 / (alpha + 1), h2], [h1, h2, h1]])
    return None


def gm_blur_kernel(mean, cov, size=15):
    """utils_blindsr.py:86-96: the bivariate normal density at the pixel centres, normalised to sum 1.  The density's
    constant cancels in the normalisation, so it is the exponent of the quadratic form of inv(cov) alone."""
    center = size / 2.0 + 0.5
    c = np.arange(size) - center + 1
    cx, cy = np.meshgrid(c - mean[0], c - mean[1])            # k[y, x] = pdf([cx, cy])
    cov = np.asarray(cov, dtype=np.float64)
    cov = (cov + cov.T) / 2                                   # (scipy reads the symmetric part)
    P = np.linalg.inv(cov)
    k = np.exp(-0.5 * (P[0, 0] * cx * cx + (P[0, 1] + P[1, 0]) * cx * cy + P[1, 1] * cy * cy))
    return k / np.sum(k)


def anisotropic_Gaussian(ksize=15, theta=np.pi, l1=6, l2=6):
    """utils_blindsr.py:64-83."""
    v = np.dot(np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]]), np.array([1., 0.]))
    V = np.array([[v[0], v[1]], [v[1], -v[0]]])
    D = np.array([[l1, 0], [0, l2]])
    Sigma = np.dot(np.dot(V, D), np.linalg.inv(V))
    return gm_blur_kernel(mean=[0, 0], cov=Sigma, size=ksize)


def _interp_axis(n, at):
    """(lower index, fraction) of the positions `at` on the grid 0 .. n - 1"""
    i0 = np.clip(np.floor(at).astype(np.int64), 0, max(n - 2, 0))
    return i0, at - i0


def shift_pixel(x, sf, upper_left=True):
    """utils_blindsr.py:99-125: the image sampled (sf - 1) / 2 pixels further along both axes, bilinear, on coordinates
    clamped to the image: what `interp2d(xv, yv, x)(x1, y1)` (linear) gives.  (H,W) or (H,W,C), fp64."""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape[:2]
    shift = (sf - 1) * 0.5 * (1 if upper_left else -1)
    x1 = np.clip(np.arange(0, w, 1.0) + shift, 0, w - 1)
    y1 = np.clip(np.arange(0, h, 1.0) + shift, 0, h - 1)
    (ix, fx), (iy, fy) = _interp_axis(w, x1), _interp_axis(h, y1)
    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    tail = (1,) * (x.ndim - 2)
    fxr, fyr = fx.reshape((1, -1) + tail), fy.reshape((-1, 1) + tail)
    top = x[iy][:, ix] * (1 - fxr) + x[iy][:, ix1] * fxr
    bot = x[iy1][:, ix] * (1 - fxr) + x[iy1][:, ix1] * fxr
    return top * (1 - fyr) + bot * fyr


def correlated_factor(D, U, L):
    """The 3 x 3 matrix M with noise_c = sum_j M[c][j] z_j for add_Gaussian_noise's third mode (:371-375): cov =
    |L^2 U^T diag(D) U| and numpy's multivariate_normal factor of it, x = z @ (sqrt(s)[:, None] * v) from (u, s, v) =
    svd(cov), transposed."""
    conv = np.dot(np.dot(np.transpose(U), np.diag(D)), U)
    cov = np.abs(L ** 2 * conv)
    _, s, v = np.linalg.svd(cov)
    return (np.sqrt(s)[:, None] * v).T


def _orth(A):
    """scipy.linalg.orth: an orthonormal basis of A's range from its SVD"""
    u, s, _ = np.linalg.svd(A, full_matrices=False)
    tol = max(A.shape) * np.amax(s) * np.finfo(s.dtype).eps
    return u[:, :int(np.sum(s > tol))]


# ------------------------------------------------------------------ the draws ----
class BlindSRDraws(Draws):
    """The random decisions of utils_blindsr, from the reference's generators under the reference's names; `randn` and
    `poisson` (the noise fields, from the GPU's generator) are `datapath.Draws`'s.  Tests subclass it to replay."""

    def random(self):                                   # random.random()
        return random.random()

    def py_uniform(self, lo, hi):                       # random.uniform
        return random.uniform(lo, hi)

    def sample(self, population, k):                    # random.sample
        return random.sample(population, k)

    def np_rand(self, *shape):                          # np.random.rand
        return np.random.rand(*shape)


# ------------------------------------------------------------------ programs: pure host code ----
# One stage of one image with every size: kind in 'conv' | 'resize' | 'noise' | 'poisson' | 'jpeg' | 'imresize';
# (h, w) -> (oh, ow); params by kind:
#   conv      kernel (k, k) fp64, stride, clip          resize    interp 1 | 2 | 3, clip
#   noise     op (a name of NOISE_OPS), scale, matrix (3, 3) | None, clip, lead_clip
#   poisson   vals, gray                                jpeg      quality
#   imresize  scale (MATLAB's bicubic, prep.imresize), clip
Stage = namedtuple("Stage", "kind h w oh ow params")
# rows, cols: the mod crop of the input; order: the reference's shuffle_order (after the downsample3 swap); crop:
# (rnd_h, rnd_w) of the LQ patch or None
Program = namedtuple("Program", "variant C rows cols sf sf_ori lq_patchsize stages order crop")


def _blur_stage(h, w, sf, d):
    wd2 = wd = 0.2 + 0.2 * sf
    if d.random() < 0.3:
        l1 = wd2 * d.random()
        l2 = wd2 * d.random()
        ksize = 2 * d.randint(0, 3) + 3
        k = anisotropic_Gaussian(ksize=ksize, theta=d.random() * np.pi, l1=l1, l2=l2)
    else:
        ksize = 2 * d.randint(0, 3) + 3
        k = fspecial('gaussian', ksize, wd * d.random())
    return Stage("conv", h, w, h, w, dict(kernel=k, stride=1, clip=False))


def _resize_stage(h, w, ow, oh, interp, clip=True):
    if oh < 1 or ow < 1:
        raise ValueError(f"ssl_amd.blindsr: a resize of ({h}, {w}) to ({oh}, {ow}) is empty (cv2.resize raises too)")
    return Stage("resize", h, w, oh, ow, dict(interp=interp, clip=clip))


def _add_resize_stage(h, w, sf, d):
    rnum = float(d.np_rand())
    if rnum > 0.8:
        sf1 = d.py_uniform(1, 2)
    elif rnum < 0.7:
        sf1 = d.py_uniform(0.5 / sf, 1)
    else:
        sf1 = 1.0
    return _resize_stage(h, w, int(sf1 * w), int(sf1 * h), d.choice([1, 2, 3]))


def _matrix(noise_level2, C, d, who):
    if C != 3:
        raise ValueError(f"ssl_amd.blindsr: {who}'s correlated mode needs a 3-channel image (the reference fails too)")
    D = np.asarray(d.np_rand(3), dtype=np.float64)
    U = _orth(np.asarray(d.np_rand(3, 3), dtype=np.float64))
    return correlated_factor(D, U, noise_level2 / 255.)


def _gaussian_stage(h, w, C, l1, l2, d):
    level = d.randint(l1, l2)
    rnum = float(d.np_rand())
    if rnum > 0.6:
        p = dict(op="GAUSS_COLOR", scale=level / 255.0, matrix=None)
    elif rnum < 0.4:
        p = dict(op="GAUSS_GRAY", scale=level / 255.0, matrix=None)
    else:
        p = dict(op="GAUSS_CORR", scale=1.0, matrix=_matrix(l2, C, d, "add_Gaussian_noise"))
    return Stage("noise", h, w, h, w, dict(p, clip=True, lead_clip=False))


def _speckle_stage(h, w, C, l1, l2, d):
    level = d.randint(l1, l2)
    rnum = d.random()
    if rnum > 0.6:
        p = dict(op="SPECKLE_COLOR", scale=level / 255.0, matrix=None)
    elif rnum < 0.4:
        p = dict(op="SPECKLE_GRAY", scale=level / 255.0, matrix=None)
    else:
        p = dict(op="SPECKLE_CORR", scale=1.0, matrix=_matrix(l2, C, d, "add_speckle_noise"))
    return Stage("noise", h, w, h, w, dict(p, clip=True, lead_clip=True))


def _poisson_stage(h, w, C, d):
    vals = 10 ** (2 * d.random() + 2.0)
    gray = not d.random() < 0.5
    if gray and C != 3:
        raise ValueError("ssl_amd.blindsr: add_Poisson_noise's gray form needs a 3-channel image (the reference fails too)")
    return Stage("poisson", h, w, h, w, dict(vals=vals, gray=gray))


def _jpeg_stage(h, w, d):
    return Stage("jpeg", h, w, h, w, dict(quality=d.randint(75, 95)))


def build_program(variant, h1, w1, draws, sf=4, lq_patchsize=72, shuffle_prob=0.5, C=3):
    """The stages of one image of (h1, w1, C) under `variant` ('bsrgan' | 'nocrop' | 'ours_p' | 'plus'), every decision
    taken from `draws` in the reference's order and every size worked out as the reference's `int()` and slices do.
    Pure host code: nothing here touches a GPU."""
    if variant not in ("bsrgan", "nocrop", "ours_p", "plus"):
        raise ValueError(f"ssl_amd.blindsr: unknown variant {variant!r}")
    d, sf_ori = draws, sf
    if variant in ("bsrgan", "nocrop"):
        h, w = h1 - h1 % sf, w1 - w1 % sf
    else:                                   # (:636, :725 crop the ROWS by the width's remainder and the other way round)
        h, w = min(h1, w1 - w1 % sf), min(w1, h1 - h1 % sf)
    rows, cols = h, w
    if h < lq_patchsize * sf or w < lq_patchsize * sf:
        raise ValueError(f'img size ({h1}X{w1}) is too small!')
    stages = []
    if variant == "plus":
        if d.random() < shuffle_prob:
            order = d.sample(range(13), 13)
        else:
            order = list(range(13))
            order[2:6] = d.sample(order[2:6], 4)
            order[9:13] = d.sample(order[9:13], 4)
        for i in order:
            if i in (0, 7):
                stages.append(_blur_stage(h, w, sf, d))
            elif i in (1, 8):
                stages.append(_add_resize_stage(h, w, sf, d))
            elif i in (2, 9):
                stages.append(_gaussian_stage(h, w, C, 2, 25, d))
            elif i in (3, 10):
                if d.random() < 0.1:
                    stages.append(_poisson_stage(h, w, C, d))
            elif i in (4, 11):
                if d.random() < 0.1:
                    stages.append(_speckle_stage(h, w, C, 2, 25, d))
            elif i in (5, 12):
                d.random()                                     # (the camera-ISP draw; isp_model is None)
            else:
                stages.append(_jpeg_stage(h, w, d))
            if stages:
                h, w = stages[-1].oh, stages[-1].ow
        stages.append(_resize_stage(h, w, int(1 / sf * cols), int(1 / sf * rows), d.choice([1, 2, 3]), clip=False))
        h, w = stages[-1].oh, stages[-1].ow
    else:
        if sf == 4 and d.random() < 0.25:                      # downsample1
            if float(d.np_rand()) < 0.5:
                stages.append(_resize_stage(h, w, int(1 / 2 * w), int(1 / 2 * h), d.choice([1, 2, 3])))
            else:
                stages.append(Stage("imresize", h, w, math.ceil(h * 0.5), math.ceil(w * 0.5), dict(scale=0.5, clip=True)))
            h, w = stages[-1].oh, stages[-1].ow
            sf = 2
        order = d.sample(range(7), 7)
        idx1, idx2 = order.index(2), order.index(3)
        if idx1 > idx2:                                        # keep downsample3 last
            order[idx1], order[idx2] = order[idx2], order[idx1]
        a = b = None
        for i in order:
            if i in (0, 1):
                stages.append(_blur_stage(h, w, sf, d))
            elif i == 2:
                a, b = w, h
                if d.random() < 0.75:
                    sf1 = d.py_uniform(1, 1 / 0.85)
                    stages.append(_resize_stage(h, w, int(1 / sf1 * w), int(1 / sf1 * h), d.choice([1, 2, 3])))
                else:
                    k = fspecial('gaussian', 2 * d.randint(0, 3) + 3, d.py_uniform(0.1, 0.25 * sf))
                    k_shifted = shift_pixel(k, sf)
                    k_shifted = k_shifted / k_shifted.sum()
                    stages.append(Stage("conv", h, w, -(-h // sf), -(-w // sf), dict(kernel=k_shifted, stride=sf, clip=True)))
            elif i == 3:
                stages.append(_resize_stage(h, w, int(1 / sf * a), int(1 / sf * b), d.choice([1, 2, 3])))
            elif i == 4:
                stages.append(_gaussian_stage(h, w, C, 1, 12, d))
            elif i == 5:
                if d.random() < 0.9:
                    stages.append(_jpeg_stage(h, w, d))
            else:
                d.random()                                     # (the camera-ISP draw; isp_model is None)
            if stages:
                h, w = stages[-1].oh, stages[-1].ow
    stages.append(_jpeg_stage(h, w, d))
    crop = None
    if variant != "nocrop":
        if h < lq_patchsize or w < lq_patchsize:
            raise ValueError(f"ssl_amd.blindsr: the degraded image ({h}, {w}) is smaller than the patch {lq_patchsize}")
        crop = (d.randint(0, h - lq_patchsize), d.randint(0, w - lq_patchsize))
    return Program(variant, C, rows, cols, sf, sf_ori, lq_patchsize, stages, list(order), crop)


# ------------------------------------------------------------------ tables and launches ----
def fill_table(family, recs, in_elems, out_elems, field_elems=0, pool_elems=0, same_buffer=False):
    """(the table's host image as a uint8 array, its tile count) of `recs` (a _REC array) from the library's fill, which
    checks every range against the buffers' sizes in elements and refuses overlapping outputs."""
    L = _lib.lib()
    recs = np.ascontiguousarray(recs, dtype=_REC)
    nbytes = L.ssg_blindsr_table_bytes(len(recs))
    table = np.zeros(nbytes, dtype=np.uint8)
    n_tiles = np.zeros(1, dtype=np.int32)
    _lib.check(L.ssg_blindsr_table_fill(family, recs.ctypes.data, len(recs), in_elems, out_elems, field_elems, pool_elems,
                                        int(same_buffer), table.ctypes.data, nbytes, n_tiles.ctypes.data))
    return table, int(n_tiles[0])


class _Pool:
    """The parameter pool of a run: the taps of every convolution and the 3 x 3 matrices, fp32, one behind the other"""

    def __init__(self):
        self.parts, self.n = [], 0

    def add(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64).astype(np.float32).reshape(-1)
        off, self.n = self.n, self.n + v.size
        self.parts.append(v)
        return off

    def array(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, np.float32)


def _set_stage(rec, st, C, pool):
    """the operation's fields of one record (not its offsets); `st` a conv, resize or noise Stage"""
    p = st.params
    rec["C"], rec["h"], rec["w"], rec["oh"], rec["ow"] = C, st.h, st.w, st.oh, st.ow
    rec["flags"] = (CLIP if p.get("clip") else 0) | (LEAD_CLIP if p.get("lead_clip") else 0)
    if st.kind == "conv":
        k = np.asarray(p["kernel"])
        if k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 != 1 or not 3 <= k.shape[0] <= MAX_KERNEL:
            raise ValueError(f"ssl_amd.blindsr: a blur kernel is odd and square, 3 .. {MAX_KERNEL}, got {k.shape}")
        rec["op"], rec["stride"], rec["pool_off"] = k.shape[0], p["stride"], pool.add(k)
    elif st.kind == "resize":
        rec["op"] = p["interp"]
    else:
        rec["op"], rec["p0"] = NOISE_OPS[p["op"]], p["scale"]
        if p.get("matrix") is not None:
            rec["pool_off"] = pool.add(p["matrix"])


def _upload(host, device):
    return torch.from_numpy(host).to(device)


def _launch_family(dev, family, table_ptr, n_tiles, in_ptr, out_ptr, field_ptr, pool_ptr):
    """the family's entry point over one table, on `dev` (each takes the arguments its kernels read)"""
    L = _lib.lib()
    if family == CONV:
        launch(dev, L.ssg_blindsr_conv, table_ptr, n_tiles, in_ptr, out_ptr, pool_ptr)
    elif family == RESIZE:
        launch(dev, L.ssg_blindsr_resize, table_ptr, n_tiles, in_ptr, out_ptr)
    else:
        launch(dev, L.ssg_blindsr_noise, table_ptr, n_tiles, in_ptr, out_ptr, field_ptr, pool_ptr)


def _noise_planes(op, C):
    """(planes of the field, planes of the output) of a noise operation"""
    name = op if isinstance(op, str) else {v: k for k, v in NOISE_OPS.items()}[op]
    fields = 0 if name.startswith("POISSON_RATES") else (1 if name.endswith("_GRAY") else C)
    return fields, (1 if name == "POISSON_RATES_GRAY" else C)


@torch.no_grad()
def ragged_apply(family, images, stages, fields=None):
    """ONE launch of `family` (CONV | RESIZE | NOISE) over a list of planar (C, h, w) float32 GPU images of differing
    sizes, image i under stages[i] (a conv, resize or noise Stage whose (h, w) are the image's); fields[i] the noise
    operation's field ((planes, h, w) or None).  Returns the list of outputs (views of one buffer)."""
    if not images:
        return []
    dev = images[0].device
    pool, recs = _Pool(), np.zeros(len(images), dtype=_REC)
    in_off = out_off = field_off = 0
    outs = []
    for i, (x, st) in enumerate(zip(images, stages)):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and tuple(x.shape[1:]) == (st.h, st.w)):
            raise ValueError(f"ssl_amd.blindsr: image {i} must be a float32 GPU tensor (C, {st.h}, {st.w}), got "
                             f"{x.dtype} {tuple(x.shape)} on {x.device}")
        C = x.shape[0]
        _set_stage(recs[i], st, C, pool)
        recs[i]["in_off"], recs[i]["out_off"], recs[i]["field_off"] = in_off, out_off, field_off
        planes_f, planes_o = _noise_planes(st.params["op"], C) if family == NOISE else (0, C)
        if planes_f and (fields is None or fields[i] is None or fields[i].numel() != planes_f * st.h * st.w):
            raise ValueError(f"ssl_amd.blindsr: image {i} needs a field of {planes_f} plane(s) of ({st.h}, {st.w})")
        outs.append((out_off, planes_o, st.oh, st.ow))
        in_off, out_off, field_off = in_off + x.numel(), out_off + planes_o * st.oh * st.ow, field_off + planes_f * st.h * st.w
    pool_host = pool.array()
    table, n_tiles = fill_table(family, recs, in_off, out_off, field_off, pool_host.size)
    with on(dev):
        src = torch.cat([x.reshape(-1) for x in images])
        dst = torch.empty(out_off, dtype=torch.float32, device=dev)
        fld = None
        if field_off:
            fld = torch.cat([f.to(device=dev, dtype=torch.float32).reshape(-1) for f, r in zip(fields, recs)
                             if _noise_planes(int(r["op"]), int(r["C"]))[0]])
        blob = _upload(np.concatenate([table, pool_host.view(np.uint8)]), dev)
        _launch_family(dev, family, blob.data_ptr(), n_tiles, _ptr(src), _ptr(dst), _ptr(fld), blob.data_ptr() + table.size)
    return [dst[o:o + p * h * w].view(p, h, w) for o, p, h, w in outs]


# ------------------------------------------------------------------ the batch ----
def _planar(img, device):
    """an HWC (or HW) image in [0, 1], numpy or tensor -> float32 (C, h, w) on `device`"""
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if not torch.is_tensor(t) or not t.is_floating_point():
        raise TypeError("ssl_amd.blindsr: an image is a floating numpy array or tensor in [0, 1], (H, W, C)")
    if t.dim() == 2:
        t = t[:, :, None]
    if t.dim() != 3 or t.shape[2] not in (1, 3):
        raise ValueError(f"ssl_amd.blindsr: an image is (H, W, 1 | 3), got {tuple(t.shape)}")
    return t.detach().to(device=device, dtype=torch.float32).permute(2, 0, 1).contiguous()


def _hwc(t, like):
    y = t.permute(1, 2, 0).contiguous()
    return y.cpu().numpy() if isinstance(like, np.ndarray) else y


def _device(images):
    for t in images:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return current_gpu("ssl_amd.blindsr: the degradation chain runs on the GPU and none is visible; there is no CPU path")


def _align(n, a=4):
    return (n + a - 1) // a * a


class _Plan:
    """What a batch of stage lists launches, worked out on the host before anything runs: the regions of the two
    ping-pong arenas (image i owns the same region of both, as large as its largest intermediate), and slot by slot one
    entry per operation family present.  `launches` counts the kernels of the ragged families."""

    def __init__(self, channels, stage_lists):
        self.n = len(stage_lists)
        sizes = []
        for C, stages in zip(channels, stage_lists):
            sizes.append(max([C * s.h * s.w for s in stages] + [C * s.oh * s.ow for s in stages] + [1]))
        self.region = np.concatenate([[0], np.cumsum([_align(s) for s in sizes])]).astype(np.int64)
        self.arena = int(self.region[-1])
        if 2 * self.arena > 2 ** 32 - 1:
            raise ValueError("ssl_amd.blindsr: the batch's two arenas hold 2^32 elements or more; feed fewer images at once")
        self.pool = _Pool()
        self.steps, self.tables = [], []          # tables: host images, 16-byte aligned inside the upload
        self.table_bytes = 0
        self.launches = 0
        side = [0] * self.n                       # the arena every image lies in
        where = lambda i, s: int(s * self.arena + self.region[i])
        for slot in range(max([len(s) for s in stage_lists] + [0])):
            here = [(i, stages[slot]) for i, stages in enumerate(stage_lists) if slot < len(stages)]
            step = dict(conv=None, resize=None, rates=None, noise=None, jpeg={}, imresize=[], n_normal=0, n_draws=0)
            for fam, kind in ((CONV, "conv"), (RESIZE, "resize")):
                sel = [(i, st) for i, st in here if st.kind == kind]
                if sel:
                    recs = np.zeros(len(sel), dtype=_REC)
                    for r, (i, st) in zip(recs, sel):
                        _set_stage(r, st, channels[i], self.pool)
                        r["in_off"], r["out_off"] = where(i, side[i]), where(i, 1 - side[i])
                    step[kind] = (fam, recs)
            noisy = [(i, st) for i, st in here if st.kind in ("noise", "poisson")]
            if noisy:
                n_normal = sum(_noise_planes(st.params["op"], channels[i])[0] * st.h * st.w
                               for i, st in noisy if st.kind == "noise")
                recs, rates = np.zeros(len(noisy), dtype=_REC), []
                f_normal, f_draw = 0, n_normal
                for r, (i, st) in zip(recs, noisy):
                    C = channels[i]
                    if st.kind == "noise":
                        _set_stage(r, st, C, self.pool)
                        r["field_off"] = f_normal
                        f_normal += _noise_planes(st.params["op"], C)[0] * st.h * st.w
                    else:
                        gray, planes = st.params["gray"], 1 if st.params["gray"] else C
                        r["C"], r["h"], r["w"], r["oh"], r["ow"] = C, st.h, st.w, st.h, st.w
                        r["op"], r["p0"], r["flags"] = NOISE_OPS["POISSON_GRAY" if gray else "POISSON_COLOR"], st.params["vals"], CLIP
                        r["field_off"] = f_draw
                        q = r.copy()
                        q["op"], q["flags"], q["field_off"] = NOISE_OPS["POISSON_RATES_GRAY" if gray else "POISSON_RATES"], 0, 0
                        q["in_off"], q["out_off"] = where(i, side[i]), f_draw - n_normal
                        rates.append(q)
                        f_draw += planes * st.h * st.w
                    r["in_off"], r["out_off"] = where(i, side[i]), where(i, 1 - side[i])
                step["noise"], step["n_normal"], step["n_draws"] = (NOISE, recs), n_normal, f_draw - n_normal
                if rates:
                    step["rates"] = (NOISE, np.array(rates, dtype=_REC))
            for i, st in here:
                if st.kind == "jpeg":
                    step["jpeg"].setdefault((channels[i], st.h, st.w), []).append(
                        (where(i, side[i]), where(i, 1 - side[i]), st.params["quality"]))
                elif st.kind == "imresize":
                    step["imresize"].append((where(i, side[i]), where(i, 1 - side[i]), channels[i], st))
                elif st.kind not in ("conv", "resize", "noise", "poisson"):
                    raise ValueError(f"ssl_amd.blindsr: unknown stage kind {st.kind!r}")
                side[i] = 1 - side[i]
            self.steps.append(step)
        self.side = side
        self.where = where

    def finish(self):
        """the tables, now that the pool is complete: one host image (tables, then the pool) for ONE upload"""
        pool = self.pool.array()
        parts, at = [], 0
        for step in self.steps:
            for key in ("conv", "resize", "rates", "noise"):
                if step[key] is None:
                    continue
                fam, recs = step[key]
                if key == "rates":
                    table, n_tiles = fill_table(fam, recs, 2 * self.arena, step["n_draws"], 0, pool.size)
                else:
                    table, n_tiles = fill_table(fam, recs, 2 * self.arena, 2 * self.arena,
                                                step["n_normal"] + step["n_draws"], pool.size, same_buffer=True)
                pad = np.zeros(_align(table.size, 16) - table.size, np.uint8)
                step[key] = (fam, at, n_tiles)
                parts += [table, pad]
                at += table.size + pad.size
                self.launches += 1
        self.pool_at = at
        return np.concatenate(parts + [pool.view(np.uint8)]) if at or pool.size else np.zeros(0, np.uint8)


@torch.no_grad()
def run_stages(images, stage_lists, draws=None, trace=None):
    """Planar (C, h, w) float32 GPU images through their stage lists, slot by slot, one launch per operation family
    present in a slot.  Returns (the list of results, the number of ragged launches made).  `trace`, a list, receives
    per slot the list of every image's copy after its stage of that slot (None where it has none): what the tests
    compare stage by stage."""
    from . import prep
    draws = draws if draws is not None else BlindSRDraws()
    if not images:
        return [], 0
    dev = images[0].device
    channels = [int(x.shape[0]) for x in images]
    for i, (x, stages) in enumerate(zip(images, stage_lists)):
        h, w = (stages[0].h, stages[0].w) if stages else tuple(x.shape[1:])
        if tuple(x.shape[1:]) != (h, w):
            raise ValueError(f"ssl_amd.blindsr: image {i} is {tuple(x.shape[1:])} and its first stage takes ({h}, {w})")
    plan = _Plan(channels, stage_lists)
    host = plan.finish()
    with on(dev):
        buf = torch.empty(max(2 * plan.arena, 1), dtype=torch.float32, device=dev)
        for i, x in enumerate(images):
            buf[plan.where(i, 0):plan.where(i, 0) + x.numel()].copy_(x.reshape(-1))
        blob = _upload(host, dev) if host.size else None
        base = blob.data_ptr() if blob is not None else 0
        pool_ptr = base + plan.pool_at if blob is not None else None
        for slot, step in enumerate(plan.steps):
            for key in ("conv", "resize"):
                if step[key]:
                    fam, at, n_tiles = step[key]
                    _launch_family(dev, fam, base + at, n_tiles, _ptr(buf), _ptr(buf), None, pool_ptr)
            if step["noise"]:
                field = draws.randn((step["n_normal"],), dev) if step["n_normal"] else None
                if step["rates"]:
                    rates = torch.empty(step["n_draws"], dtype=torch.float32, device=dev)
                    fam, at, n_tiles = step["rates"]
                    _launch_family(dev, fam, base + at, n_tiles, _ptr(buf), _ptr(rates), None, pool_ptr)
                    drawn = draws.poisson(rates).to(torch.float32)
                    field = drawn if field is None else torch.cat([field.reshape(-1), drawn])
                fam, at, n_tiles = step["noise"]
                _launch_family(dev, fam, base + at, n_tiles, _ptr(buf), _ptr(buf), _ptr(field.contiguous()), pool_ptr)
            for (C, h, w), group in step["jpeg"].items():
                n = C * h * w
                batch = torch.stack([buf[s:s + n].view(C, h, w) for s, _, _ in group])
                y = jpeg_roundtrip(batch, [q for _, _, q in group])
                for (_, dst, _), yi in zip(group, y):
                    buf[dst:dst + n].copy_(yi.reshape(-1))
            for src, dst, C, st in step["imresize"]:
                y = prep.imresize(buf[src:src + C * st.h * st.w].view(C, st.h, st.w), st.params["scale"], True)
                if tuple(y.shape) != (C, st.oh, st.ow):
                    raise RuntimeError(f"ssl_amd.blindsr: imresize gave {tuple(y.shape)}, the program has ({C}, {st.oh}, {st.ow})")
                buf[dst:dst + y.numel()].copy_((y.clamp_(0.0, 1.0) if st.params["clip"] else y).reshape(-1))
            if trace is not None:
                snap = []
                for i, stages in enumerate(stage_lists):
                    if slot < len(stages):
                        st, at = stages[slot], plan.where(i, (slot + 1) % 2)
                        snap.append(buf[at:at + channels[i] * st.oh * st.ow].view(channels[i], st.oh, st.ow).clone())
                    else:
                        snap.append(None)
                trace.append(snap)
        outs = []
        for i, (x, stages) in enumerate(zip(images, stage_lists)):
            h, w = (stages[-1].oh, stages[-1].ow) if stages else tuple(x.shape[1:])
            at = plan.where(i, plan.side[i])
            outs.append(buf[at:at + channels[i] * h * w].view(channels[i], h, w))
    return outs, plan.launches


def _crop_groups(images, size, tops):
    """augment_crop over images of differing sizes: one call per group of equal size; (B, C, size, size)"""
    out = [None] * len(images)
    groups = {}
    for i, x in enumerate(images):
        groups.setdefault(tuple(x.shape), []).append(i)
    for idx in groups.values():
        y = augment_crop(torch.stack([images[i] for i in idx]), (size, size), [tops[i] for i in idx])
        for i, yi in zip(idx, y):
            out[i] = yi
    return torch.stack(out)


class BlindSRDegradation:
    """The batched form of utils_blindsr's four chains: `feed(images)` takes a list of HWC images in [0, 1] (numpy or
    tensors, sizes may all differ) and returns (lq (B, C, p, p), hq (B, C, p sf, p sf)) on the GPU, p = lq_patchsize --
    for variant 'ours_p' (lq, hq, hq_E) with `images_E`, for 'nocrop' two lists of (C, h, w) tensors.  `variant`:
    'bsrgan' (degradation_bsrgan), 'nocrop', 'ours_p', 'plus' (with shuffle_prob and use_sharp).  After a feed,
    `programs` holds every image's Program and `launches` the number of ragged kernel launches made."""

    def __init__(self, sf=4, lq_patchsize=72, variant="bsrgan", shuffle_prob=0.5, use_sharp=False, isp_model=None,
                 draws=None):
        if isp_model is not None:
            raise NotImplementedError("ssl_amd.blindsr: isp_model must be None (every caller in the reference passes None)")
        if variant not in ("bsrgan", "nocrop", "ours_p", "plus"):
            raise ValueError(f"ssl_amd.blindsr: unknown variant {variant!r}")
        self.sf, self.lq_patchsize, self.variant = int(sf), int(lq_patchsize), variant
        self.shuffle_prob, self.use_sharp = shuffle_prob, bool(use_sharp) and variant == "plus"
        self.draws = draws if draws is not None else BlindSRDraws()
        self.programs, self.launches = [], 0

    def draw_programs(self, shapes):
        """one Program per (h, w, C), the decisions drawn image by image in the reference's order"""
        return [build_program(self.variant, h, w, self.draws, self.sf, self.lq_patchsize, self.shuffle_prob, C)
                for h, w, C in shapes]

    @torch.no_grad()
    def feed(self, images, images_E=None, programs=None, trace=None):
        if self.variant == "ours_p" and (images_E is None or len(images_E) != len(images)):
            raise ValueError("ssl_amd.blindsr: variant 'ours_p' takes images_E, one per image")
        dev = _device(images)
        planar = [_planar(x, dev) for x in images]
        if programs is None:
            programs = self.draw_programs([(x.shape[1], x.shape[2], x.shape[0]) for x in planar])
        self.programs = programs
        planar = [x[:, :p.rows, :p.cols].contiguous() for x, p in zip(planar, programs)]
        if self.use_sharp:
            sharp = USMSharp(radius=50)
            planar = [sharp(x[None], weight=0.5, threshold=10)[0] for x in planar]
        lq, self.launches = run_stages(planar, [p.stages for p in programs], self.draws, trace)
        if self.variant == "nocrop":
            return [x.clone() for x in lq], planar
        size, sf = self.lq_patchsize, self.sf
        tops = [p.crop for p in programs]
        tops_h = [(int(t * sf), int(l * sf)) for t, l in tops]
        out = (_crop_groups(lq, size, tops), _crop_groups(planar, size * sf, tops_h))
        if self.variant == "ours_p":
            # (the reference slices past the end silently where hq_E is smaller; augment_crop raises instead)
            out += (_crop_groups([_planar(x, dev) for x in images_E], size * sf, tops_h),)
        return out


# ------------------------------------------------------------------ one image, the reference's names ----
def _one(img, stage_of, draws):
    draws = draws if draws is not None else BlindSRDraws()
    x = _planar(img, _device([img]))
    st = stage_of(x.shape[1], x.shape[2], x.shape[0], draws)
    return _hwc(run_stages([x], [[st]], draws)[0][0], img)


def add_blur(img, sf=4, draws=None):
    """utils_blindsr.py:335-346."""
    return _one(img, lambda h, w, C, d: _blur_stage(h, w, sf, d), draws)


def add_resize(img, sf=4, draws=None):
    """utils_blindsr.py:349-360."""
    return _one(img, lambda h, w, C, d: _add_resize_stage(h, w, sf, d), draws)


def add_Gaussian_noise(img, noise_level1=1, noise_level2=12, draws=None):
    """utils_blindsr.py:363-377 (a new image is returned; the reference also adds into its argument)."""
    return _one(img, lambda h, w, C, d: _gaussian_stage(h, w, C, noise_level1, noise_level2, d), draws)


def add_speckle_noise(img, noise_level1=2, noise_level2=25, draws=None):
    """utils_blindsr.py:380-395."""
    return _one(img, lambda h, w, C, d: _speckle_stage(h, w, C, noise_level1, noise_level2, d), draws)


def add_Poisson_noise(img, draws=None):
    """utils_blindsr.py:398-409."""
    return _one(img, lambda h, w, C, d: _poisson_stage(h, w, C, d), draws)


def add_JPEG_noise(img, draws=None):
    """utils_blindsr.py:412-418 (datapath.add_JPEG_noise, the codec of ssg_jpegcodec.hip)."""
    from .datapath import add_JPEG_noise as _add
    return _add(img, draws=draws)


def add_sharpening(img, weight=0.5, radius=50, threshold=10):
    """utils_blindsr.py:309-332 on datapath.USMSharp, whose arithmetic it is."""
    x = _planar(img, _device([img]))
    return _hwc(USMSharp(radius=radius)(x[None], weight=weight, threshold=threshold)[0], img)


def random_crop(lq, hq, sf=4, lq_patchsize=64, draws=None):
    """utils_blindsr.py:421-429."""
    return random_crop_ours_p(lq, hq, None, sf, lq_patchsize, draws)[:2]


def random_crop_ours_p(lq, hq, hq_E, sf=4, lq_patchsize=64, draws=None):
    """utils_blindsr.py:431-440."""
    draws = draws if draws is not None else BlindSRDraws()
    dev = _device([lq, hq])
    a = _planar(lq, dev)
    top = draws.randint(0, a.shape[1] - lq_patchsize), draws.randint(0, a.shape[2] - lq_patchsize)
    top_h = (int(top[0] * sf), int(top[1] * sf))
    cut = lambda x, n, t: _hwc(augment_crop(_planar(x, dev)[None], (n, n), [t])[0], x)
    return (cut(lq, lq_patchsize, top), cut(hq, lq_patchsize * sf, top_h),
            None if hq_E is None else cut(hq_E, lq_patchsize * sf, top_h))


def _chain(variant, img, img_E=None, draws=None, isp_model=None, **kw):
    deg = BlindSRDegradation(variant=variant, isp_model=isp_model, draws=draws, **kw)
    out = deg.feed([img], None if img_E is None else [img_E])
    return tuple(_hwc(t[0], img) for t in out)


def degradation_bsrgan(img, sf=4, lq_patchsize=72, isp_model=None, draws=None):
    """utils_blindsr.py:443-530: (lq patch, hq patch), HWC."""
    return _chain("bsrgan", img, draws=draws, isp_model=isp_model, sf=sf, lq_patchsize=lq_patchsize)


def degradation_bsrgan_nocrop(img, sf=4, lq_patchsize=72, isp_model=None, draws=None):
    """utils_blindsr.py:532-616: (lq, hq), HWC, uncropped."""
    return _chain("nocrop", img, draws=draws, isp_model=isp_model, sf=sf, lq_patchsize=lq_patchsize)


def degradation_bsrgan_ours_p(img, img_E, sf=4, lq_patchsize=72, isp_model=None, draws=None):
    """utils_blindsr.py:618-706: (lq patch, hq patch, hq_E patch), HWC."""
    return _chain("ours_p", img, img_E, draws=draws, isp_model=isp_model, sf=sf, lq_patchsize=lq_patchsize)


def degradation_bsrgan_plus(img, sf=4, shuffle_prob=0.5, use_sharp=False, lq_patchsize=64, isp_model=None, draws=None):
    """utils_blindsr.py:708-792: (lq patch, hq patch), HWC."""
    return _chain("plus", img, draws=draws, isp_model=isp_model, sf=sf, lq_patchsize=lq_patchsize,
                  shuffle_prob=shuffle_prob, use_sharp=use_sharp)
