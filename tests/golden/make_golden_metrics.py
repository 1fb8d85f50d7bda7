"""Generate f24_metrics.npz FROM THE REFERENCE ITSELF: calculate_psnr, calculate_ssim and to_y_channel.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_metrics.py <reference root>

It imports the reference's GAN-Based-SR/basicsr/utils/color_util.py, basicsr/metrics/metric_util.py and
basicsr/metrics/psnr_ssim.py by path, with the `basicsr` packages around them stubbed in sys.modules (a registry whose
register() returns the function unchanged) and with `cv2` STUBBED, because OpenCV is not available where the fixture
is made:

  cv2.getGaussianKernel(n, sigma)  OpenCV's documented closed form for sigma > 0: G_i = a exp(-(i - (n - 1) / 2)^2 /
                                   (2 sigma^2)), a chosen so that the G_i sum to 1; an (n,1) float64 column
  cv2.filter2D(img, -1, window)    scipy.ndimage.correlate(img, window, mode='mirror') (BORDER_REFLECT_101).  _ssim
                                   keeps the 'valid' slice [5:-5, 5:-5] only, which no border mode reaches, so the
                                   border mode is immaterial; what the stub fixes is the fp64 correlation itself.

Inputs per case (prefix cN_): `a`, `b` uint8 images in BGR order as the reference's metric functions receive them
((H,W,3) or (H,W)); for a case that starts from float tensors also `xa`, `xb`, the float32 (C,H,W) RGB tensors, of
which a, b are tensor2img's result restated here (img_util.py:65-89: clamp to [0, 1], (H,W,C), RGB -> BGR,
(x * 255.0).round() in fp32, uint8).  Per configuration k (crop_border, test_y_channel): `cfgK` = the pair, `psnrK`,
`ssimK` the reference's results, and `ya`, `yb` = to_y_channel(a), to_y_channel(b) (float32, uncropped).

Only DATA is stored (inputs, expected outputs); no reference source text.
"""
import importlib.util
import os
import sys
import types
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = [(0, False), (4, True), (0, True), (3, False)]


def load_reference(root):
    import scipy.ndimage
    base = os.path.join(root, "GAN-Based-SR", "basicsr")
    for name in ("basicsr", "basicsr.utils", "basicsr.utils.registry", "basicsr.metrics", "cv2"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod

    class _Registry:
        def register(self, *a, **k):
            return lambda obj: obj

    sys.modules["basicsr.utils.registry"].METRIC_REGISTRY = _Registry()

    def get_gaussian_kernel(n, sigma):
        x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
        g = np.exp(-0.5 / (sigma * sigma) * x * x)
        return (g * (1.0 / g.sum())).reshape(n, 1)

    cv2 = sys.modules["cv2"]
    cv2.getGaussianKernel = get_gaussian_kernel
    cv2.filter2D = lambda img, ddepth, window: scipy.ndimage.correlate(img, window, mode='mirror')

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    color = load("basicsr.utils.color_util", ("utils", "color_util.py"))
    sys.modules["basicsr.utils"].bgr2ycbcr = color.bgr2ycbcr
    util = load("basicsr.metrics.metric_util", ("metrics", "metric_util.py"))
    return load("basicsr.metrics.psnr_ssim", ("metrics", "psnr_ssim.py")), util


def tensor2img(x):
    x = np.clip(x.astype(np.float32), np.float32(0), np.float32(1)).transpose(1, 2, 0)
    if x.shape[2] == 1:
        x = x[..., 0]
    else:
        x = np.ascontiguousarray(x[..., ::-1])
    return (x * 255.0).round().astype(np.uint8)


def main():
    ref, util = load_reference(sys.argv[1])
    rng = np.random.default_rng(24)
    out = {}
    cases = []
    # c0: float RGB tensors, values beyond [0, 1] included
    gt = rng.random((3, 24, 29), dtype=np.float32) * 1.2 - 0.1
    sr = gt + 0.05 * rng.standard_normal((3, 24, 29)).astype(np.float32)
    cases.append(dict(xa=sr, xb=gt, a=tensor2img(sr), b=tensor2img(gt)))
    # c1: uint8 BGR images (smooth + noise)
    yy, xx = np.mgrid[0:23, 0:31]
    base = np.stack([128 + 100 * np.sin(xx / 5.0 + c) * np.cos(yy / 4.0) for c in range(3)], -1)
    b = np.clip(base + rng.normal(0, 4, base.shape), 0, 255).round().astype(np.uint8)
    a = np.clip(b + rng.normal(0, 6, base.shape), 0, 255).round().astype(np.uint8)
    cases.append(dict(a=a, b=b))
    # c2: grey uint8, (H,W)
    b = rng.integers(0, 256, (23, 20), dtype=np.uint8)
    a = np.clip(b.astype(np.int32) + rng.integers(-9, 10, b.shape), 0, 255).astype(np.uint8)
    cases.append(dict(a=a, b=b))
    # c3: a float grey tensor
    gt = rng.random((1, 21, 20), dtype=np.float32)
    sr = gt + 0.02 * rng.standard_normal(gt.shape).astype(np.float32)
    cases.append(dict(xa=sr, xb=gt, a=tensor2img(sr), b=tensor2img(gt)))
    for i, c in enumerate(cases):
        for key, v in c.items():
            out[f"c{i}_{key}"] = v
        out[f"c{i}_ya"] = util.to_y_channel(c["a"])
        out[f"c{i}_yb"] = util.to_y_channel(c["b"])
        for k, (crop, y) in enumerate(CONFIGS):
            out[f"c{i}_cfg{k}"] = np.array([crop, int(y)], dtype=np.int32)
            out[f"c{i}_psnr{k}"] = np.float64(ref.calculate_psnr(c["a"], c["b"], crop, test_y_channel=y))
            out[f"c{i}_ssim{k}"] = np.float64(ref.calculate_ssim(c["a"], c["b"], crop, test_y_channel=y))
            print(f"c{i} {c['a'].shape} crop {crop} y {y}: psnr {float(out[f'c{i}_psnr{k}']):.6f} "
                  f"ssim {float(out[f'c{i}_ssim{k}']):.6f}")
    out["n_cases"] = np.int32(len(cases))
    out["n_configs"] = np.int32(len(CONFIGS))
    path = os.path.join(HERE, "f24_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
