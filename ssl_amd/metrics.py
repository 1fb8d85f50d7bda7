"""PSNR, SSIM and NIQE as the reference computes them, on the GPU (ssl_amd/csrc/ssg_metrics.hip, ssg_niqe.hip).

Named as `basicsr.metrics` names them: `calculate_psnr`, `calculate_ssim` and `calculate_metric` keep the reference's
signatures, its ValueError and its shape assertion; `psnr_ssim` is the batched call on a model's own tensors (what
`tensor2img` + `calculate_metric` do per image, without leaving the device), `MetricAverager` the validation loop's
`metric_results[name] += ...; metric_results[name] /= idx + 1` with one synchronisation at the end.

Contract: include/ssg_hip.h section (J).  A NaN in a float input is unspecified, as in the reference.  An image whose
cropped side is shorter than 11 is refused (the reference's SSIM would be the mean of an empty map); there is no CPU
path.

NIQE (section (K)): `calculate_niqe` keeps the reference's signature, `niqe` is the batched call on a model's tensors,
`MetricAverager.add_niqe` its running mean.  It is computed in fp64 from the rounded plane on.  The pristine model
(mu_pris_param, cov_pris_param) is the reference's data and does not ship with the package: `load_niqe_params` takes
it from a path, a mapping, the environment variable SSL_AMD_NIQE_PARAMS or an installed basicsr.  `calculate_metric`
and `add_all` do not dispatch to NIQE (no reference YAML lists it under val.metrics).

LPIPS and DISTS (section (V)), the other two entries of the reference's val.metrics blocks, live in
ssl_amd/metrics_feat.py and are re-exported here: `calculate_lpips`, `calculate_dists`, the batched `lpips_dists`, the
`LPIPS` and `DISTS` modules, `MetricAverager.add_lpips` / `add_dists`; `calculate_metric` and `add_all` dispatch on
their types.  Unlike the metrics above they have a CPU path (the packages' torch lines)."""
import importlib.util
import os
from copy import deepcopy

import numpy as np
import torch

from . import _lib, metrics_feat
from ._gpu import current_gpu, launch as _launch, need_gpu as _need_gpu, ptr as _ptr, workspace as _workspace
from .metrics_feat import DISTS, LPIPS, calculate_dists, calculate_lpips, lpips_dists  # noqa: F401

__all__ = ["calculate_psnr", "calculate_ssim", "calculate_niqe", "calculate_metric", "psnr_ssim", "niqe",
           "load_niqe_params", "MetricAverager", "calculate_lpips", "calculate_dists", "lpips_dists", "LPIPS", "DISTS"]

KIND_F32_RGB, KIND_U8_HWC, KIND_U8_CHW = (_lib.CONSTANTS["SSG_METRIC_" + k] for k in ("F32_RGB", "U8_HWC", "U8_CHW"))
KIND_F32_PLANE = _lib.CONSTANTS["SSG_NIQE_F32_PLANE"]   # NIQE only: a float32 (B,H,W) plane (input_order 'HW')
NIQE_BLOCK, NIQE_FEATURES = 96, 36
NIQE_PARAMS_ENV = "SSL_AMD_NIQE_PARAMS"
NIQE_PARAMS_FILE = "niqe_pris_params.npz"
_CONVERT = {'y': 0, 'gray': 1}


def _device():
    return current_gpu("ssl_amd.metrics: the metrics run on the GPU and none is visible; there is no CPU path")


def _run(a, b, kind, B, C, H, W, crop_border, y_channel):
    """(B,4) float64 on the device: PSNR, SSIM, the sum of squared plane differences, its number of terms."""
    _need_gpu(a, b)
    L = _lib.lib()
    out = torch.empty((B, 4), dtype=torch.float64, device=a.device)
    ws, nb = _workspace(L.ssg_metric_workspace_bytes(B, C, H, W, int(crop_border)), a.device)
    _launch(a.device, L.ssg_psnr_ssim, _ptr(a), _ptr(b), kind, B, C, H, W, int(crop_border), int(bool(y_channel)),
            _ptr(out), _ptr(ws), nb)
    return out


def metric_planes(img, kind, crop_border=0, test_y_channel=False):
    """The float32 planes (B,P,Hc,Wc) the metrics are computed on, after quantise, crop and Y: `img` is a contiguous
    device tensor laid out as `kind` says ((B,C,H,W), or (B,H,W,C) for KIND_U8_HWC)."""
    _need_gpu(img)
    if kind == KIND_U8_HWC:
        B, H, W, C = img.shape
    else:
        B, C, H, W = img.shape
    P = 1 if test_y_channel else C
    out = torch.empty((B, P, max(H - 2 * crop_border, 0), max(W - 2 * crop_border, 0)), dtype=torch.float32,
                      device=img.device)
    _launch(img.device, _lib.lib().ssg_metric_planes, _ptr(img.contiguous()), kind, B, C, H, W, int(crop_border),
            int(bool(test_y_channel)), _ptr(out))
    return out


def psnr_ssim(sr, gt, crop_border=0, test_y_channel=False):
    """PSNR and SSIM of float (N,C,H,W) (or (C,H,W)) RGB tensors in nominal [0, 1], as `visuals['result']` and
    `visuals['gt']` hold them: what the reference gets from tensor2img (clamp, * 255, round half to even, uint8, BGR)
    followed by calculate_psnr / calculate_ssim.  Returns a device (N,2) float64 tensor {PSNR, SSIM}; runs on the
    current stream without synchronising with the host."""
    assert sr.shape == gt.shape, (f'Image shapes are different: {sr.shape}, {gt.shape}.')
    if not (torch.is_tensor(sr) and sr.is_floating_point() and gt.is_floating_point()):
        raise TypeError("ssl_amd: psnr_ssim takes floating-point tensors (use calculate_psnr / calculate_ssim for "
                        "uint8 images)")
    if sr.dim() == 3:
        sr, gt = sr[None], gt[None]
    if sr.dim() != 4:
        raise ValueError(f"ssl_amd: psnr_ssim takes (N,C,H,W) or (C,H,W) tensors, got {tuple(sr.shape)}")
    dev = sr.device if sr.is_cuda else _device()       # host tensors are uploaded, as arrays are
    a = sr.detach().to(device=dev, dtype=torch.float32).contiguous()
    b = gt.detach().to(device=dev, dtype=torch.float32).contiguous()
    B, C, H, W = a.shape
    return _run(a, b, KIND_F32_RGB, B, C, H, W, crop_border, test_y_channel)[:, :2]


def _as_image(img, input_order):
    """A uint8 device tensor and its kind for an image in the reference's conventions: (H,W), (H,W,C) or (C,H,W), BGR,
    uint8 or a float type holding the integers 0 .. 255 (the offline script's `img * 255`; rounded to the nearest)."""
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if not t.is_cuda:
        t = t.to(_device())
    if t.dtype != torch.uint8:
        t = t.round().clamp(0, 255).to(torch.uint8)
    if t.dim() == 2:
        return t.contiguous()[None, None], KIND_U8_CHW
    if t.dim() != 3:
        raise ValueError(f"ssl_amd: an image is (H,W), (H,W,C) or (C,H,W), got {tuple(t.shape)}")
    return t.contiguous()[None], (KIND_U8_CHW if input_order == 'CHW' else KIND_U8_HWC)


def _both(img, img2, crop_border, input_order, test_y_channel):
    assert img.shape == img2.shape, (f'Image shapes are different: {img.shape}, {img2.shape}.')
    if input_order not in ['HWC', 'CHW']:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    a, kind = _as_image(img, input_order)
    b, _ = _as_image(img2, input_order)
    if kind == KIND_U8_HWC:
        B, H, W, C = a.shape
    else:
        B, C, H, W = a.shape
    return _run(a, b, kind, B, C, H, W, crop_border, test_y_channel)


def calculate_psnr(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    """basicsr.metrics.calculate_psnr: images with range [0, 255], BGR, numpy arrays (uploaded) or tensors.  Returns a
    Python float (inf for identical images)."""
    return float(_both(img, img2, crop_border, input_order, test_y_channel)[0, 0])


def calculate_ssim(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    """basicsr.metrics.calculate_ssim: as calculate_psnr."""
    return float(_both(img, img2, crop_border, input_order, test_y_channel)[0, 1])


# ---------------------------------------------------------------------------------------------------------- NIQE ---
_niqe_params = {}                       # (source, device) -> (mu, cov)


def _find_niqe_params():
    """The parameter file's path when no source is given: the environment variable, then an installed basicsr."""
    path = os.environ.get(NIQE_PARAMS_ENV)
    if path:
        return path
    try:
        spec = importlib.util.find_spec("basicsr")          # located, never imported
    except (ImportError, ValueError):
        spec = None
    for root in (spec.submodule_search_locations or []) if spec is not None else []:
        cand = os.path.join(root, "metrics", NIQE_PARAMS_FILE)
        if os.path.exists(cand):
            return cand
    raise FileNotFoundError(
        f"ssl_amd: NIQE needs the pristine model ({NIQE_PARAMS_FILE}: mu_pris_param, cov_pris_param), which is the "
        f"reference's data and does not ship with this package: set {NIQE_PARAMS_ENV} to its path, install basicsr "
        f"(the file lies beside basicsr.metrics), or pass niqe_pris_params= (a path or a mapping of the two arrays)")


def load_niqe_params(source=None, device=None):
    """(mu (36,), cov (36,36)) as float64 tensors on `device` (the current GPU by default), cached per source and
    device.  `source`: a path to niqe_pris_params.npz, a mapping holding mu_pris_param and cov_pris_param, or None
    (SSL_AMD_NIQE_PARAMS, then the file beside an installed basicsr.metrics, else FileNotFoundError)."""
    dev = torch.device(device) if device is not None else _device()
    mapping = source is not None and not isinstance(source, (str, os.PathLike))
    if not mapping:
        path = os.fspath(source) if source is not None else _find_niqe_params()
        key = (os.path.abspath(path), str(dev))
        if key in _niqe_params:
            return _niqe_params[key]
        source = np.load(path)
    mu = np.asarray(source["mu_pris_param"], dtype=np.float64).reshape(-1)
    cov = np.asarray(source["cov_pris_param"], dtype=np.float64)
    if mu.shape != (NIQE_FEATURES,) or cov.shape != (NIQE_FEATURES, NIQE_FEATURES):
        raise ValueError(f"ssl_amd: NIQE parameters are (36,) and (36,36), got {mu.shape} and {cov.shape}")
    out = (torch.from_numpy(mu).to(dev), torch.from_numpy(np.ascontiguousarray(cov)).to(dev))
    if not mapping:
        _niqe_params[key] = out
    return out


def _niqe_geometry(t, kind):
    if kind == KIND_U8_HWC:
        B, H, W, C = t.shape
    elif kind == KIND_F32_PLANE:
        (B, H, W), C = t.shape, 1
    else:
        B, C, H, W = t.shape
    return B, C, H, W


def _niqe_blocks(H, W, crop_border):
    return max(H - 2 * crop_border, 0) // NIQE_BLOCK, max(W - 2 * crop_border, 0) // NIQE_BLOCK


def _niqe_run(t, kind, crop_border, convert_to, params):
    """(B,) float64 scores on the device for a contiguous device tensor laid out as `kind` says."""
    _need_gpu(t)
    B, C, H, W = _niqe_geometry(t, kind)
    mu, cov = load_niqe_params(params, t.device)
    L = _lib.lib()
    out = torch.empty((B,), dtype=torch.float64, device=t.device)
    ws, nb = _workspace(L.ssg_niqe_workspace_bytes(B, C, H, W, int(crop_border)), t.device)
    _launch(t.device, L.ssg_niqe, _ptr(t), kind, B, C, H, W, int(crop_border), _CONVERT[convert_to], _ptr(mu), _ptr(cov),
            _ptr(out), _ptr(ws), nb)
    return out


def niqe_planes(t, kind, crop_border=0, convert_to='y'):
    """The two planes NIQE is computed on: (B,96 nbh,96 nbw) float32 (the rounded plane) and (B,48 nbh,48 nbw) float64
    (its antialiased bicubic half), for a contiguous device tensor laid out as `kind` says."""
    _need_gpu(t)
    B, C, H, W = _niqe_geometry(t, kind)
    nbh, nbw = _niqe_blocks(H, W, crop_border)
    p1 = torch.empty((B, 96 * nbh, 96 * nbw), dtype=torch.float32, device=t.device)
    p2 = torch.empty((B, 48 * nbh, 48 * nbw), dtype=torch.float64, device=t.device)
    _launch(t.device, _lib.lib().ssg_niqe_planes, _ptr(t), kind, B, C, H, W, int(crop_border), _CONVERT[convert_to],
            _ptr(p1), _ptr(p2))
    return p1, p2


def niqe_features(t, kind, crop_border=0, convert_to='y'):
    """The (B,nblk,36) float64 feature rows, blocks in the reference's order (block column outer)."""
    _need_gpu(t)
    B, C, H, W = _niqe_geometry(t, kind)
    nbh, nbw = _niqe_blocks(H, W, crop_border)
    L = _lib.lib()
    feat = torch.empty((B, nbh * nbw, NIQE_FEATURES), dtype=torch.float64, device=t.device)
    ws, nb = _workspace(L.ssg_niqe_workspace_bytes(B, C, H, W, int(crop_border)), t.device)
    _launch(t.device, L.ssg_niqe_features, _ptr(t), kind, B, C, H, W, int(crop_border), _CONVERT[convert_to], _ptr(feat),
            _ptr(ws), nb)
    return feat


def _as_niqe_image(img, input_order):
    """The device tensor and kind of an image as calculate_niqe receives it: 'HW' keeps its float values (the kernel
    rounds them half to even, as the reference's img.round() does); 'HWC' / 'CHW' are images holding 0 .. 255."""
    if input_order != 'HW':
        return _as_image(img, input_order)
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if t.dim() != 2:
        raise ValueError(f"ssl_amd: input_order 'HW' takes an (H,W) plane, got {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.to(_device())
    return t.to(torch.float32).contiguous()[None], KIND_F32_PLANE


def calculate_niqe(img, crop_border, input_order='HWC', convert_to='y', **kwargs):
    """basicsr.metrics.calculate_niqe: an image with range [0, 255], BGR for 'HWC' / 'CHW', or an (H,W) plane for 'HW';
    a numpy array (uploaded) or a tensor.  `niqe_pris_params=` names the pristine model (see load_niqe_params).
    Returns a Python float; NaN where fewer than two blocks give NaN-free features (the reference's pinv raises or
    returns NaN there)."""
    if input_order not in ['HWC', 'CHW', 'HW']:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC", "CHW" and "HW"')
    if convert_to not in _CONVERT:
        raise ValueError(f'Wrong convert_to {convert_to}. Supported values are "y" and "gray"')
    t, kind = _as_niqe_image(img, input_order)
    return float(_niqe_run(t, kind, crop_border, convert_to, kwargs.get('niqe_pris_params'))[0])


def niqe(sr, crop_border=0, convert_to='y', niqe_pris_params=None):
    """NIQE of float (N,3,H,W) (or (3,H,W)) RGB tensors in nominal [0, 1], as `visuals['result']` holds them: what the
    reference gets from tensor2img followed by calculate_niqe.  Returns a device (N,) float64 tensor; runs on the
    current stream without synchronising with the host (once the parameters and the alpha table are on the device:
    the first call per device uploads them)."""
    if not (torch.is_tensor(sr) and sr.is_floating_point()):
        raise TypeError("ssl_amd: niqe takes floating-point tensors (use calculate_niqe for images)")
    if convert_to not in _CONVERT:
        raise ValueError(f'Wrong convert_to {convert_to}. Supported values are "y" and "gray"')
    if sr.dim() == 3:
        sr = sr[None]
    if sr.dim() != 4:
        raise ValueError(f"ssl_amd: niqe takes (N,C,H,W) or (C,H,W) tensors, got {tuple(sr.shape)}")
    dev = sr.device if sr.is_cuda else _device()
    a = sr.detach().to(device=dev, dtype=torch.float32).contiguous()
    return _niqe_run(a, KIND_F32_RGB, crop_border, convert_to, niqe_pris_params)


_COLUMN = {"calculate_psnr": 0, "calculate_ssim": 1}


def _column(metric_type):
    if metric_type not in _COLUMN:
        raise KeyError(f"No object named '{metric_type}' found in 'metric' registry!")
    return _COLUMN[metric_type]


def _is_model_tensor(x):
    return torch.is_tensor(x) and x.is_floating_point()


def calculate_metric(data, opt):
    """basicsr.metrics.calculate_metric: dispatches on opt['type'].  Floating-point TENSORS in `data` (img=, img2=) are
    taken for a model's (C,H,W) / (1,C,H,W) RGB tensors in [0, 1] and go through the quantising path, so a validation
    loop can drop tensor2img; arrays and uint8 tensors are images as the reference passes them."""
    # (a state_dict given as lpips_weights= / dists_weights= is handed on as the object it is: the networks are cached per
    # weights source, and a copy would be a new source, and a new network, per call)
    weights = {k: opt[k] for k in metrics_feat.WEIGHT_OPTIONS if k in opt}
    opt = dict(deepcopy({k: v for k, v in opt.items() if k not in weights}), **weights)
    metric_type = opt.pop('type')
    img, img2 = data['img'], data['img2']
    if metric_type in metrics_feat.FEATURE_METRICS:
        if _is_model_tensor(img) and _is_model_tensor(img2):
            out = metrics_feat.batched(metric_type, img, img2, opt)
            if out.shape[0] != 1:
                raise ValueError("ssl_amd: calculate_metric takes one image per call (lpips_dists is the batched call)")
            return float(out[0])
        return (calculate_lpips if metric_type == "calculate_lpips" else calculate_dists)(img, img2, **opt)
    col = _column(metric_type)
    if _is_model_tensor(img) and _is_model_tensor(img2):
        opt.pop('input_order', None)
        out = psnr_ssim(img, img2, opt.get('crop_border', 0), opt.get('test_y_channel', False))
        if out.shape[0] != 1:
            raise ValueError("ssl_amd: calculate_metric takes one image per call (psnr_ssim is the batched call)")
        return float(out[0, col])
    return (calculate_psnr, calculate_ssim)[col](img, img2, **opt)


class MetricAverager:
    """The validation loop's running sums, kept on the device:

        avg = MetricAverager()
        for val_data in dataloader:                       # any image sizes
            ...
            avg.add_all(visuals['result'], visuals['gt'], opt['val']['metrics'])
        metric_results = avg.result()                     # the one synchronisation

    `add(name, sr, gt, **opt)` adds one metric (opt as in the YAML: type, crop_border, test_y_channel; type defaults
    to 'calculate_' + name); `add_all` takes the YAML's whole `metrics` dict and runs the fused call once per distinct
    (crop_border, test_y_channel).  `result()` returns {name: sum / images}: the reference's
    metric_results[name] / (idx + 1)."""

    def __init__(self):
        self._sum = {}
        self._count = {}

    def _accumulate(self, name, values):
        s = values.sum()
        self._sum[name] = self._sum[name] + s if name in self._sum else s
        self._count[name] = self._count.get(name, 0) + values.numel()

    def add(self, name, sr, gt, **opt):
        metric_type = opt.get('type', 'calculate_' + name)
        if metric_type in metrics_feat.FEATURE_METRICS:
            return self._accumulate(name, metrics_feat.batched(metric_type, sr, gt, opt))
        col = _column(metric_type)
        out = psnr_ssim(sr, gt, opt.get('crop_border', 0), opt.get('test_y_channel', False))
        self._accumulate(name, out[:, col])

    def add_all(self, sr, gt, metrics):
        done = {}
        for name, opt in metrics.items():
            if opt.get('type', 'calculate_' + name) in metrics_feat.FEATURE_METRICS:
                self.add(name, sr, gt, **opt)
                continue
            col = _column(opt.get('type', 'calculate_' + name))
            key = (int(opt.get('crop_border', 0)), bool(opt.get('test_y_channel', False)))
            if key not in done:
                done[key] = psnr_ssim(sr, gt, *key)
            self._accumulate(name, done[key][:, col])

    def add_niqe(self, name, sr, **opt):
        """One NIQE value per image of `sr` (float RGB tensors in [0, 1]); opt: crop_border, convert_to,
        niqe_pris_params."""
        out = niqe(sr, opt.get('crop_border', 0), opt.get('convert_to', 'y'), opt.get('niqe_pris_params'))
        self._accumulate(name, out)

    def add_lpips(self, name, sr, gt, **opt):
        """One LPIPS value per image (float RGB tensors in [0, 1]); opt: crop_border, lpips_weights, lpips_net."""
        self._accumulate(name, metrics_feat.batched("calculate_lpips", sr, gt, opt))

    def add_dists(self, name, sr, gt, **opt):
        """One DISTS value per image (float RGB tensors in [0, 1]); opt: crop_border, dists_weights."""
        self._accumulate(name, metrics_feat.batched("calculate_dists", sr, gt, opt))

    def result(self):
        if not self._sum:
            return {}
        names = list(self._sum)
        sums = torch.stack([self._sum[n] for n in names]).cpu().tolist()
        return {n: s / self._count[n] for n, s in zip(names, sums)}
