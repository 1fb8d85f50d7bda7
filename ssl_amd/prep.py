"""Pillow-exact image resize, MATLAB's bicubic imresize and the dataset preparation around them, on the GPU
(ssl_amd/csrc/ssg_resample.hip, ssl_amd/csrc/ssg_imresize.hip).

`resize` is `PIL.Image.resize(size, resample)` for 8-bit 'L' and 'RGB' images and the five convolution filters, byte for
byte (the algorithm is integer from its coefficient tables on; the tables are computed on the host in fp64 with the C
library's sin / cos, as Pillow's C code computes them, and cached per (in, out, filter) and device).  On top of it:

* `load_img`: the Diffusion fork's `load_img` (test.py:111-120): RGB, sides rounded down to a multiple of 32, LANCZOS,
  `2 (x / 255) - 1`, as one launch with a float epilogue;
* `multiscale` / `multiscale_plan`: generate_multiscale_img.py ('gan') and generate_multiscale_DF2K.py ('dm');
* `subimage_grid` / `extract_subimages`: extract_subimages.py:82-99.

`imresize` (alias `imresize_np`) is the reference's `basicsr.utils.matlab_functions.imresize` / KAIR's
`utils_image.imresize(_np)`: MATLAB's bicubic imresize for any scale, with or without antialiasing, evaluated in fp64
(include/ssg_hip.h section (O)); `modcrop` is generate_bicubic_img.m's.

Contract: include/ssg_hip.h section (N).  Images are uint8 tensors on the GPU, (H,W), (H,W,C) or (B,H,W,C) with C 1 or 3;
decoding and encoding image files stay on the CPU (PIL), there is no CPU path for the resize itself."""
import numpy as np
import torch

from . import _lib
from ._gpu import current_gpu, launch as _launch, need_gpu as _need_gpu, ptr as _ptr

__all__ = ["resize", "load_img", "from_pil", "multiscale", "multiscale_plan", "subimage_grid", "extract_subimages",
           "subimage_name", "FILTERS", "imresize", "imresize_np", "modcrop"]

_C = _lib.CONSTANTS                      # the numbers of include/ssg_hip.h
# Pillow's Image.Resampling numbers
FILTERS = {name: _C["SSG_RESAMPLE_" + name.upper()] for name in ('lanczos', 'bilinear', 'bicubic', 'box', 'hamming')}
_OUT = {'uint8': _C["SSG_RESAMPLE_U8_HWC"], 'unit': _C["SSG_RESAMPLE_F32_UNIT"], 'signed': _C["SSG_RESAMPLE_F32_SIGNED"]}
_tables = {}


def _filter(resample):
    if isinstance(resample, str) and resample.lower() in FILTERS:
        return FILTERS[resample.lower()]
    if not isinstance(resample, (str, bool)) and resample in FILTERS.values():
        return int(resample)
    raise ValueError(f"ssl_amd: resize takes one of {tuple(FILTERS)} (or Pillow's number of one), got {resample!r}")


def host_table(insz, outsz, filt):
    """(bounds (out, 2), coef (out, ksize)) int32 numpy arrays from the library's host function."""
    L = _lib.lib()
    ks = L.ssg_resample_ksize(insz, outsz, filt)
    _lib.check(min(ks, 0))
    bounds = np.empty((outsz, 2), np.int32)
    coef = np.empty((outsz, ks), np.int32)
    _lib.check(L.ssg_resample_table(insz, outsz, filt, bounds.ctypes.data, coef.ctypes.data))
    return bounds, coef


def _device_table(insz, outsz, filt, dev):
    key = (insz, outsz, filt, dev)
    if key not in _tables:
        _tables[key] = tuple(torch.from_numpy(t).to(dev) for t in host_table(insz, outsz, filt))
    return _tables[key]


def _check_size(size):
    try:
        w, h = size
    except (TypeError, ValueError):
        raise ValueError(f"ssl_amd: resize takes size = (width, height), got {size!r}") from None
    for v in (w, h):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"ssl_amd: resize takes integer sizes, got {size!r}")
    if w < 1 or h < 1:
        raise ValueError(f"ssl_amd: height and width must be > 0, got size {size!r}")
    return int(w), int(h)


def resize(img, size, resample='lanczos', out='uint8'):
    """`img` uint8 on the GPU, (H,W), (H,W,C) or (B,H,W,C), C 1 or 3; `size` = (w, h) as Pillow orders it.  `out` 'uint8'
    returns the bytes in the layout of `img`; 'unit' (v / 255) and 'signed' (2 (v / 255) - 1) return float32 (B,C,h,w)."""
    filt = _filter(resample)
    w, h = _check_size(size)
    if out not in _OUT:
        raise ValueError(f"ssl_amd: resize out is one of {tuple(_OUT)}, got {out!r}")
    if not torch.is_tensor(img) or img.dtype != torch.uint8:
        raise TypeError("ssl_amd: resize takes a uint8 tensor (8-bit 'L' or 'RGB' pixels)")
    if img.dim() not in (2, 3, 4):
        raise ValueError(f"ssl_amd: resize takes (H,W), (H,W,C) or (B,H,W,C), got {tuple(img.shape)}")
    x = img[..., None] if img.dim() == 2 else img
    x = x[None] if x.dim() == 3 else x
    B, H, W, C = x.shape
    if C not in (1, 3):
        raise ValueError(f"ssl_amd: resize takes 1 ('L') or 3 ('RGB') channels last, got {C}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"ssl_amd: resize got an empty image {tuple(img.shape)}")
    if max(B * H * W * C, B * h * w * C) > 2 ** 31 - 1:
        raise ValueError("ssl_amd: resize takes at most 2^31 - 1 elements per call")
    L = _lib.lib()
    r = L.ssg_resample_max_ratio()
    if W > r * w or H > r * h:
        raise NotImplementedError(f"ssl_amd: the fused resize takes in / out <= {r} per axis, got {(W, H)} -> {(w, h)}")
    _need_gpu(img)
    x = x.contiguous()
    dev = x.device
    xb, xk = _device_table(W, w, filt, dev) if W != w else (None, None)
    yb, yk = _device_table(H, h, filt, dev) if H != h else (None, None)
    kind = _OUT[out]
    if kind == _OUT['uint8']:
        res = torch.empty((B, h, w, C), dtype=torch.uint8, device=dev)
    else:
        res = torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
    _launch(dev, L.ssg_resample, _ptr(x), B, C, H, W, h, w, filt, _ptr(xb), _ptr(xk), _ptr(yb), _ptr(yk), kind, _ptr(res))
    if kind == _OUT['uint8']:
        res = res if img.dim() == 4 else res[0]
        res = res[..., 0] if img.dim() == 2 else res
    return res


def _current_device():
    return current_gpu("ssl_amd: the resize runs on the GPU and none is visible; there is no CPU path")


def from_pil(image, device=None):
    """A PIL image of mode 'L' or 'RGB' as a uint8 GPU tensor (H,W) or (H,W,3).  The decode is PIL's, on the CPU."""
    mode = getattr(image, 'mode', None)
    if mode not in ('L', 'RGB'):
        raise NotImplementedError(f"ssl_amd: the GPU resize takes 8-bit 'L' and 'RGB' images, not mode {mode!r}")
    a = np.array(image)                                      # (a copy: PIL hands out a read-only buffer)
    return torch.from_numpy(a).to(device if device is not None else _current_device())


def load_img(image, device=None):
    """The Diffusion fork's load_img on the GPU: `image` is a path, a PIL image (converted to RGB as there), or a uint8
    (H,W,3) array / tensor.  Returns float32 (1,3,h,w) in [-1, 1] with h, w the sides rounded down to a multiple of 32."""
    if isinstance(image, (str, bytes)) or hasattr(image, '__fspath__'):
        from PIL import Image
        image = Image.open(image)
    if hasattr(image, 'convert'):
        image = np.array(image.convert("RGB"))
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not torch.is_tensor(image) or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise TypeError("ssl_amd: load_img takes a path, a PIL image or a uint8 (H,W,3) array")
    H, W = image.shape[:2]
    w, h = W - W % 32, H - H % 32
    if w == 0 or h == 0:
        raise ValueError(f"ssl_amd: load_img rounds the sides down to a multiple of 32; ({W}, {H}) leaves none")
    if not image.is_cuda:
        image = image.to(device if device is not None else _current_device())
    return resize(image, (w, h), 'lanczos', out='signed')


# ------------------------------------------------------------------------------------------------------ multiscale ---
def multiscale_plan(width, height, variant='gan', shortest_edge=512):
    """([(suffix, (w, h)), ...], keep_original) of generate_multiscale_img.py ('gan': a scale whose shorter side falls
    under `shortest_edge` is skipped, the shortest-edge image is 'S') or generate_multiscale_DF2K.py ('dm': every scale,
    the shortest-edge image is 'T3'); the files are {basename}{suffix}.png.  keep_original: the script also copies
    ('gan') or links ('dm') the source file."""
    if variant not in ('gan', 'dm'):
        raise ValueError(f"ssl_amd: multiscale variant is 'gan' or 'dm', got {variant!r}")
    if width < 1 or height < 1 or shortest_edge < 1:
        raise ValueError("ssl_amd: multiscale takes positive sizes")
    scale_list = [0.75, 0.6, 1 / 3]
    plan = []
    for idx, scale in enumerate(scale_list):
        size = (int(width * scale), int(height * scale))
        if variant == 'dm' or min(size) >= shortest_edge:
            plan.append((f"T{idx}", size))
    if width < height:
        ratio = height / width
        w = shortest_edge
        h = int(w * ratio)
    else:
        ratio = width / height
        h = shortest_edge
        w = int(h * ratio)
    plan.append(("S" if variant == 'gan' else f"T{len(scale_list)}", (int(w), int(h))))
    for _, size in plan:
        _check_size(size)                                    # Pillow raises the same ValueError for a side of 0
    return plan, min(width, height) >= shortest_edge


def multiscale(img, variant='gan', shortest_edge=512):
    """([(suffix, image), ...], keep_original) for a uint8 GPU image (H,W) or (H,W,C): the LANCZOS resizes of
    `multiscale_plan`, one launch each."""
    if not torch.is_tensor(img) or img.dim() not in (2, 3):
        raise TypeError("ssl_amd: multiscale takes one uint8 image tensor (H,W) or (H,W,C)")
    plan, keep = multiscale_plan(img.shape[1], img.shape[0], variant, shortest_edge)
    return [(suffix, resize(img, size, 'lanczos')) for suffix, size in plan], keep


# ------------------------------------------------------------------------------------------------------ sub-images ---
def _space(n, crop_size, step, thresh_size):
    space = list(range(0, n - crop_size + 1, step))
    if n - (space[-1] + crop_size) > thresh_size:
        space.append(n - crop_size)
    return space


def subimage_grid(h, w, crop_size=512, step=256, thresh_size=0):
    """(rows, columns): the first pixel of every crop along each axis (extract_subimages.py:82-88)."""
    if crop_size < 1 or step < 1:
        raise ValueError("ssl_amd: subimage_grid takes crop_size, step >= 1")
    if h < crop_size or w < crop_size:
        raise ValueError(f"ssl_amd: a {h} x {w} image holds no {crop_size}-pixel crop")
    return _space(h, crop_size, step, thresh_size), _space(w, crop_size, step, thresh_size)


def extract_subimages(img, crop_size=512, step=256, thresh_size=0):
    """[(index, crop), ...] in row-major order with the reference's 1-based index; `img` is (H,W) or (H,W,C), the crops
    are views of it."""
    hs, ws = subimage_grid(img.shape[0], img.shape[1], crop_size, step, thresh_size)
    out = []
    for x in hs:
        for y in ws:
            out.append((len(out) + 1, img[x:x + crop_size, y:y + crop_size, ...]))
    return out


def subimage_name(name, index, extension):
    """{name}_s{index:03d}{extension} with 'x2', 'x3', 'x4', 'x8' removed from the name (extract_subimages.py:75-78,97)."""
    name = name.replace('x2', '').replace('x3', '').replace('x4', '').replace('x8', '')
    return f"{name}_s{index:03d}{extension}"


# -------------------------------------------------------------------------------------------- MATLAB's imresize ---
_imresize_tables = {}


def _imresize_scale(scale):
    try:
        s = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"ssl_amd: imresize takes a positive finite scale, got {scale!r}") from None
    if not (s > 0.0 and s != float("inf")):
        raise ValueError(f"ssl_amd: imresize takes a positive finite scale, got {scale!r}")
    return s


def imresize_host_table(n, scale, antialiasing=True):
    """(first (m,) int32, weights (m, taps) float64) of one axis from the library's host function: the first tap's
    0-based index before the mirror, and the normalised fp64 weights.  Raises for what the library refuses."""
    L = _lib.lib()
    s, aa = _imresize_scale(scale), int(bool(antialiasing))
    taps = L.ssg_imresize_taps(s, aa)
    if taps == _C["SSG_E_TOOLARGE"]:
        raise NotImplementedError(f"ssl_amd: imresize takes at most 32 taps per output, that is antialiased scales "
                                  f"down to 1 / 8; scale {s} needs {int(np.ceil(4 / s))}")
    m = L.ssg_imresize_out_size(n, s)
    if m == _C["SSG_E_TOOLARGE"]:
        raise ValueError(f"ssl_amd: imresize of a side of {n} by {s} has 2^31 pixels or more")
    _lib.check(min(taps, m, 0))
    first = np.empty(m, np.int32)
    weights = np.empty((m, taps), np.float64)
    rc = L.ssg_imresize_table(n, m, s, aa, first.ctypes.data, weights.ctypes.data)
    if rc == _C["SSG_E_IMAGESMALL"]:
        raise ValueError(f"ssl_amd: imresize by {s} on a side of {n} pixels reaches past one mirror of the image (every "
                         f"tap must lie in [1 - {n}, {2 * n}], as the reference's padding needs); the side is too small")
    _lib.check(rc)
    return first, weights


def _imresize_table(n, scale, aa, dev=None):
    """the tables of one axis, cached per (n, m, scale, antialiasing, device); dev None: the host's, which every call
    asks for first, so that a refusal is raised before anything touches the GPU"""
    m = _lib.lib().ssg_imresize_out_size(n, scale)
    key = (n, m, scale, aa, dev)
    if key not in _imresize_tables:
        host = imresize_host_table(n, scale, aa) if dev is None else _imresize_table(n, scale, aa)
        _imresize_tables[key] = host if dev is None else tuple(torch.from_numpy(t).to(dev) for t in host)
    return _imresize_tables[key]


def _imresize_launch(x, in_kind, B, C, H, W, s, aa, out_kind):
    """x contiguous on the GPU, float32 (B,C,H,W) or uint8 (B,H,W,C) -> the kernel's output tensor"""
    L = _lib.lib()
    dev = x.device
    yf, yw = _imresize_table(H, s, aa, dev)
    xf, xw = _imresize_table(W, s, aa, dev)
    h, w = yf.numel(), xf.numel()
    if out_kind == _C["SSG_IMRESIZE_U8_HWC"]:
        res = torch.empty((B, h, w, C), dtype=torch.uint8, device=dev)
    else:
        res = torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
    _launch(dev, L.ssg_imresize, _ptr(x), in_kind, B, C, H, W, s, int(aa), _ptr(yf), _ptr(yw), _ptr(xf), _ptr(xw),
            out_kind, _ptr(res))
    return res


def imresize(img, scale, antialiasing=True, out=None):
    """MATLAB's bicubic imresize as the reference's `imresize(img, scale, antialiasing=True)` restates it, in fp64 on
    the GPU; output sides are ceil(side * scale).

    * numpy float (H,W) / (H,W,C)                      -> numpy float32 of the same layout (computed on the current GPU)
    * floating GPU tensor (H,W) / (C,H,W) / (B,C,H,W)  -> float32 tensor of the same layout, "w/o round"
      (float16 / bfloat16 / float64 are computed from their float32 cast)
    * uint8 GPU tensor (H,W) / (H,W,C) / (B,H,W,C), C 1 or 3 -> uint8 of the same layout, min(255, floor(y + 0.5)) with
      y summed over the bytes themselves (MATLAB's rounding on uint8); `out='unit'` returns float32 (B,C,h,w) byte / 255.
    A CPU tensor raises RuntimeError (there is no CPU path); a scale <= 0, a side too small for one mirror, 2^31 elements
    and a channel count other than 1 or 3 raise ValueError; more than 32 taps raises NotImplementedError."""
    s = _imresize_scale(scale)
    aa = bool(antialiasing)
    if isinstance(img, np.ndarray):
        if not np.issubdtype(img.dtype, np.floating):
            raise TypeError(f"ssl_amd: imresize takes a numpy float image (the reference's [0, 1] range), got {img.dtype}; "
                            "pass bytes as a uint8 GPU tensor")
        if img.ndim not in (2, 3):
            raise ValueError(f"ssl_amd: imresize takes a numpy (H,W) or (H,W,C) image, got {img.shape}")
        if out is not None:
            raise ValueError("ssl_amd: imresize out is for uint8 tensors; a float image gives float32")
        x = torch.from_numpy(np.ascontiguousarray(img[:, :, None] if img.ndim == 2 else img).astype(np.float32))
        y = imresize(x.permute(2, 0, 1).to(_current_device()), s, aa).permute(1, 2, 0).cpu().numpy()
        return np.ascontiguousarray(y[:, :, 0] if img.ndim == 2 else y)
    if not torch.is_tensor(img):
        raise TypeError("ssl_amd: imresize takes a numpy float image, a floating GPU tensor or a uint8 GPU tensor")
    if img.dtype == torch.uint8:
        if out not in (None, 'uint8', 'unit'):
            raise ValueError(f"ssl_amd: imresize out is None, 'uint8' or 'unit' for bytes, got {out!r}")
        if img.dim() not in (2, 3, 4):
            raise ValueError(f"ssl_amd: imresize takes uint8 (H,W), (H,W,C) or (B,H,W,C), got {tuple(img.shape)}")
        x = img[..., None] if img.dim() == 2 else img
        x = x[None] if x.dim() == 3 else x
        B, H, W, C = x.shape
        if C not in (1, 3):
            raise ValueError(f"ssl_amd: imresize takes 1 ('L') or 3 ('RGB') channels last for bytes, got {C}")
        in_kind = _C["SSG_IMRESIZE_IN_U8_HWC"]
        out_kind = _C["SSG_IMRESIZE_F32_UNIT" if out == 'unit' else "SSG_IMRESIZE_U8_HWC"]
    elif img.is_floating_point():
        if out is not None:
            raise ValueError(f"ssl_amd: imresize out is for uint8 tensors; a float tensor gives float32, got out={out!r}")
        if img.dim() not in (2, 3, 4):
            raise ValueError(f"ssl_amd: imresize takes float (H,W), (C,H,W) or (B,C,H,W), got {tuple(img.shape)}")
        x = img.reshape((1,) * (4 - img.dim()) + tuple(img.shape))
        B, C, H, W = x.shape
        in_kind, out_kind = _C["SSG_IMRESIZE_IN_F32"], _C["SSG_IMRESIZE_F32_PLANES"]
    else:
        raise TypeError(f"ssl_amd: imresize takes floating or uint8 tensors, got {img.dtype}")
    if min(B, C, H, W) < 1:
        raise ValueError(f"ssl_amd: imresize got an empty image {tuple(img.shape)}")
    h, w = (len(_imresize_table(n, s, aa)[0]) for n in (H, W))        # raises what the library refuses of an axis
    if max(B * C * H * W, B * C * h * w) > 2 ** 31 - 1:
        raise ValueError("ssl_amd: imresize takes at most 2^31 - 1 elements per call, input and output")
    _need_gpu(img)
    x = x.detach().to(torch.float32).contiguous() if in_kind == _C["SSG_IMRESIZE_IN_F32"] else x.contiguous()
    res = _imresize_launch(x, in_kind, B, C, H, W, s, aa, out_kind)
    if out_kind == _C["SSG_IMRESIZE_F32_UNIT"]:
        return res
    if in_kind == _C["SSG_IMRESIZE_IN_F32"]:
        return res.reshape(tuple(img.shape[:-2]) + (h, w))
    res = res if img.dim() == 4 else res[0]
    return res[..., 0] if img.dim() == 2 else res


imresize_np = imresize


def modcrop(img, modulo):
    """generate_bicubic_img.m's modcrop: the sides cut down to a multiple of `modulo` (a view).  numpy (H,W) / (H,W,C),
    uint8 tensors (H,W) / (H,W,C) / (B,H,W,C), floating tensors (H,W) / (C,H,W) / (B,C,H,W)."""
    if isinstance(modulo, bool) or not isinstance(modulo, (int, np.integer)) or modulo < 1:
        raise ValueError(f"ssl_amd: modcrop takes an integer modulo >= 1, got {modulo!r}")
    nd = img.ndim if isinstance(img, np.ndarray) else img.dim()
    if nd not in (2, 3, 4) or (isinstance(img, np.ndarray) and nd == 4):
        raise ValueError(f"ssl_amd: modcrop takes the layouts of imresize, got {tuple(img.shape)}")
    channels_last = isinstance(img, np.ndarray) or img.dtype == torch.uint8
    ay = (0 if nd < 4 else 1) if channels_last else nd - 2
    H, W = img.shape[ay], img.shape[ay + 1]
    h, w = H - H % modulo, W - W % modulo
    if h == 0 or w == 0:
        raise ValueError(f"ssl_amd: modcrop by {modulo} of a {H} x {W} image leaves none of it")
    index = [slice(None)] * nd
    index[ay], index[ay + 1] = slice(0, h), slice(0, w)
    return img[tuple(index)]
