"""Pillow-exact image resize and the dataset preparation around it, on the GPU (ssl_amd/csrc/ssg_resample.hip).

`resize` is `PIL.Image.resize(size, resample)` for 8-bit 'L' and 'RGB' images and the five convolution filters, byte for
byte (the algorithm is integer from its coefficient tables on; the tables are computed on the host in fp64 with the C
library's sin / cos, as Pillow's C code computes them, and cached per (in, out, filter) and device).  On top of it:

* `load_img`: the Diffusion fork's `load_img` (test.py:111-120): RGB, sides rounded down to a multiple of 32, LANCZOS,
  `2 (x / 255) - 1`, as one launch with a float epilogue;
* `multiscale` / `multiscale_plan`: generate_multiscale_img.py ('gan') and generate_multiscale_DF2K.py ('dm');
* `subimage_grid` / `extract_subimages`: extract_subimages.py:82-99.

Contract: include/ssg_hip.h section (N).  Images are uint8 tensors on the GPU, (H,W), (H,W,C) or (B,H,W,C) with C 1 or 3;
decoding and encoding image files stay on the CPU (PIL), there is no CPU path for the resize itself."""
import numpy as np
import torch

from . import _lib
from .engine import _launch, _need_gpu, _ptr

__all__ = ["resize", "load_img", "from_pil", "multiscale", "multiscale_plan", "subimage_grid", "extract_subimages",
           "subimage_name", "FILTERS"]

FILTERS = {'lanczos': 1, 'bilinear': 2, 'bicubic': 3, 'box': 4, 'hamming': 5}      # Pillow's Image.Resampling numbers
_OUT = {'uint8': 0, 'unit': 1, 'signed': 2}
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
    if kind == 0:
        res = torch.empty((B, h, w, C), dtype=torch.uint8, device=dev)
    else:
        res = torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
    _launch(dev, L.ssg_resample, _ptr(x), B, C, H, W, h, w, filt, _ptr(xb), _ptr(xk), _ptr(yb), _ptr(yk), kind, _ptr(res))
    if kind == 0:
        res = res if img.dim() == 4 else res[0]
        res = res[..., 0] if img.dim() == 2 else res
    return res


def _current_device():
    if not torch.cuda.is_available():
        raise RuntimeError("ssl_amd: the resize runs on the GPU and none is visible; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


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
