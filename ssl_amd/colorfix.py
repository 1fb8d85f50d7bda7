"""StableSR's colour correction of a diffusion sample on the GPU (ssl_amd/csrc/ssg_colorfix.hip).

Named as the Diffusion fork's `scripts/wavelet_color_fix.py` names them, with its signatures and argument order (content
first, style second): `wavelet_blur`, `wavelet_decomposition`, `wavelet_reconstruction`, `calc_mean_std`,
`adaptive_instance_normalization`, and the PIL pair `adain_color_fix` / `wavelet_color_fix`.  `color_fix` is the fused
call of the sampling scripts: the correction and the `clamp((x + 1) / 2, 0, 1)` (and the `255 x` -> byte of the PNG) that
follows it, one launch for 'wavelet' and three for 'adain', without leaving the device.

Contract: include/ssg_hip.h section (L).  Tensors are (B,C,H,W), any C (the reference hard-codes three), float32 on the
GPU; float16 / bfloat16 (the scripts run under autocast) and float64 are computed in float32 and the float results cast
back to the promoted dtype of the inputs.  This is inference post-processing: an input that requires grad while grad is
enabled raises instead of dropping the gradient, and there is no CPU path."""
import numpy as np
import torch

from . import _lib
from ._gpu import launch as _launch, need_gpu as _need_gpu, ptr as _ptr, workspace as _workspace

__all__ = ["wavelet_blur", "wavelet_decomposition", "wavelet_reconstruction", "calc_mean_std",
           "adaptive_instance_normalization", "adain_color_fix", "wavelet_color_fix", "color_fix"]

OUT_RAW, OUT_UNIT, OUT_UINT8 = (_lib.CONSTANTS["SSG_COLORFIX_" + k] for k in ("RAW", "UNIT", "U8_NHWC"))
_OUT = {'raw': OUT_RAW, 'unit': OUT_UNIT, 'uint8': OUT_UINT8}
_KINDS = ('wavelet', 'adain', 'nofix')
MAX_LEVELS = 5
_FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _check(name, *tensors):
    """The argument checks that need no device, then the device check; returns the float32 contiguous inputs."""
    for t in tensors:
        if not torch.is_tensor(t) or t.dtype not in _FLOATS:
            raise TypeError(f"ssl_amd: {name} takes floating-point tensors")
        if t.dim() != 4:
            raise ValueError(f"ssl_amd: {name} takes 4D (B,C,H,W) tensors, got {tuple(t.shape)}")
        if t.numel() == 0:
            raise ValueError(f"ssl_amd: {name} got an empty tensor {tuple(t.shape)}")
    if len(tensors) == 2 and tensors[0].shape != tensors[1].shape:
        raise ValueError(f"ssl_amd: {name}: content {tuple(tensors[0].shape)} and style {tuple(tensors[1].shape)} "
                         "differ in shape")
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(f"ssl_amd: {name} is inference post-processing and has no backward; call it under "
                           "torch.no_grad() or on detached tensors")
    _need_gpu(*tensors)
    if len(tensors) == 2 and tensors[0].device != tensors[1].device:
        raise RuntimeError(f"ssl_amd: {name}: content and style are on different devices")
    return [t.detach().to(torch.float32).contiguous() for t in tensors]


def _levels(levels):
    if not isinstance(levels, int) or isinstance(levels, bool) or not 1 <= levels <= MAX_LEVELS:
        raise NotImplementedError(f"ssl_amd: the wavelet tile pass holds 1 .. {MAX_LEVELS} levels, got {levels!r}")
    return levels


def _result_dtype(*tensors):
    dt = tensors[0].dtype
    for t in tensors[1:]:
        dt = torch.promote_types(dt, t.dtype)
    return dt


def _empty_out(x, out_kind):
    B, C, H, W = x.shape
    if out_kind == OUT_UINT8:
        return torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    return torch.empty_like(x)


def wavelet_blur(image, radius):
    """The 3 x 3 kernel [1/4, 1/2, 1/4]^2 dilated by `radius` on the replicate-padded image."""
    if not isinstance(radius, int) or isinstance(radius, bool) or radius < 1:
        raise ValueError(f"ssl_amd: wavelet_blur takes an integer radius >= 1, got {radius!r}")
    x, = _check("wavelet_blur", image)
    out = torch.empty_like(x)
    _launch(x.device, _lib.lib().ssg_wavelet_blur, _ptr(x), *x.shape, radius, _ptr(out))
    return out.to(image.dtype)


def wavelet_decomposition(image, levels=5, want=('high', 'low')):
    """(high_freq, low_freq) after `levels` blurs of radius 1, 2, 4, ...; `want` names the parts to form, the other is
    returned as None."""
    levels = _levels(levels)
    x, = _check("wavelet_decomposition", image)
    high = torch.empty_like(x) if 'high' in want else None
    low = torch.empty_like(x) if 'low' in want else None
    if high is None and low is None:
        raise ValueError("ssl_amd: wavelet_decomposition: `want` names neither 'high' nor 'low'")
    _launch(x.device, _lib.lib().ssg_wavelet_decompose, _ptr(x), *x.shape, levels, _ptr(high), _ptr(low))
    return (None if high is None else high.to(image.dtype), None if low is None else low.to(image.dtype))


def _wavelet(c, s, levels, out_kind):
    out = _empty_out(c, out_kind)
    _launch(c.device, _lib.lib().ssg_colorfix_wavelet, _ptr(c), _ptr(s), *c.shape, levels, out_kind, _ptr(out))
    return out


def wavelet_reconstruction(content_feat, style_feat):
    """The content's high frequencies on the style's low frequencies (five levels)."""
    c, s = _check("wavelet_reconstruction", content_feat, style_feat)
    return _wavelet(c, s, MAX_LEVELS, OUT_RAW).to(_result_dtype(content_feat, style_feat))


def _stats(c, s, eps=1e-5):
    """(n_img, B C, 2) float64 on the device: {mean, sqrt(var + eps)} of every plane of c (and s)."""
    L = _lib.lib()
    B, C, H, W = c.shape
    stats = torch.empty((1 if s is None else 2, B * C, 2), dtype=torch.float64, device=c.device)
    ws, nb = _workspace(L.ssg_colorfix_workspace_bytes(B, C, H, W), c.device)
    _launch(c.device, L.ssg_colorfix_stats, _ptr(c), _ptr(s), B, C, H, W, float(eps), _ptr(stats), _ptr(ws), nb)
    return stats


def calc_mean_std(feat, eps=1e-5):
    """(mean, std) of every plane, each (B,C,1,1): std = sqrt(unbiased variance + eps)."""
    x, = _check("calc_mean_std", feat)
    B, C = x.shape[:2]
    st = _stats(x, None, eps)[0].to(feat.dtype)
    return st[:, 0].reshape(B, C, 1, 1), st[:, 1].reshape(B, C, 1, 1)


def _adain(c, s, out_kind):
    stats = None if s is None else _stats(c, s)
    out = _empty_out(c, out_kind)
    _launch(c.device, _lib.lib().ssg_colorfix_adain, _ptr(c), _ptr(stats), *c.shape, out_kind, _ptr(out))
    return out


def adaptive_instance_normalization(content_feat, style_feat):
    """The content, plane by plane, at the style's mean and standard deviation."""
    c, s = _check("adaptive_instance_normalization", content_feat, style_feat)
    return _adain(c, s, OUT_RAW).to(_result_dtype(content_feat, style_feat))


def color_fix(x_samples, init_image, kind='wavelet', out='unit', levels=5):
    """The sampling scripts' colour correction and what follows it, fused: `kind` 'wavelet' (wavelet_reconstruction),
    'adain' (adaptive_instance_normalization) or 'nofix' (the epilogue alone; `init_image` may be None); `out` 'raw',
    'unit' (clamp((x + 1) / 2, 0, 1)) or 'uint8' (255 times that, truncated: a device (B,H,W,C) byte tensor, what
    Image.fromarray receives)."""
    if kind not in _KINDS:
        raise ValueError(f"ssl_amd: color_fix kind is one of {_KINDS}, got {kind!r}")
    if out not in _OUT:
        raise ValueError(f"ssl_amd: color_fix out is one of {tuple(_OUT)}, got {out!r}")
    levels = _levels(levels)
    out_kind = _OUT[out]
    if kind == 'nofix':
        c, = _check("color_fix", x_samples)
        res = _adain(c, None, out_kind)
        dt = x_samples.dtype
    else:
        if init_image is None:
            raise ValueError(f"ssl_amd: color_fix kind {kind!r} needs init_image")
        c, s = _check("color_fix", x_samples, init_image)
        res = _wavelet(c, s, levels, out_kind) if kind == 'wavelet' else _adain(c, s, out_kind)
        dt = _result_dtype(x_samples, init_image)
    return res if out_kind == OUT_UINT8 else res.to(dt)


# ------------------------------------------------------------------------------------------------------ PIL pair ---
def _to_tensor(img):
    """torchvision's ToTensor on an 8-bit image: / 255, HWC -> CHW, on the current GPU, with a batch axis."""
    a = np.array(img)                                       # (a copy: PIL hands out a read-only buffer)
    if a.dtype != np.uint8:
        raise TypeError(f"ssl_amd: the PIL colour fixes take 8-bit images, got mode {getattr(img, 'mode', '?')}")
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", torch.cuda.current_device()))
    return (t.permute(2, 0, 1).to(torch.float32) / 255)[None].contiguous()


def _to_image(t):
    """torchvision's ToPILImage on a float tensor clamped to [0, 1]: * 255, truncated to bytes."""
    from PIL import Image
    a = t[0].clamp_(0.0, 1.0).mul(255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    return Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a)


def adain_color_fix(target, source):
    """AdaIN colour fix of PIL image `target` towards PIL image `source` (of the same size)."""
    return _to_image(adaptive_instance_normalization(_to_tensor(target), _to_tensor(source)))


def wavelet_color_fix(target, source):
    """Wavelet colour fix of PIL image `target` towards PIL image `source` (of the same size)."""
    return _to_image(wavelet_reconstruction(_to_tensor(target), _to_tensor(source)))
