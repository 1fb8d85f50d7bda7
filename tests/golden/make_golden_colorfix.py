"""Generate f27_colorfix.npz FROM THE REFERENCE ITSELF: the functions of the Diffusion fork's colour correction.

Needs the reference tree (which never travels with this repository) and runs on the CPU:

    python tests/golden/make_golden_colorfix.py <reference root>

It imports the reference's Diffusion-Based-SR/scripts/wavelet_color_fix.py by path, with a stub
`torchvision.transforms` in sys.modules (the real package is not needed by the tensor functions recorded here; the
stub's ToTensor / ToPILImage raise if called).

Per case (prefix cN_): `content` in [-1.2, 1.2] and `style` in [-1, 1], float32 (1,3,H,W), textured (a smooth field
plus noise, another offset and contrast per plane); the reference's float32 outputs `blur1`, `blur16` (wavelet_blur of
the content at radius 1 and 16), `high`, `low` (wavelet_decomposition of the content), `recon`
(wavelet_reconstruction), `mean_c`, `std_c`, `mean_s`, `std_s` (calc_mean_std) and `adain`
(adaptive_instance_normalization).  Shapes 1 x 3 x 40 x 56 and 1 x 3 x 5 x 40 (sides below the larger radii).

Before writing, every recorded output is held to the bounds of tests/colorfix_reference.py against its fp64
restatement; the script fails if one is outside.  Only DATA is stored; no reference source text.
"""
import importlib.util
import os
import sys
import types
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f27_colorfix.npz")
sys.path.insert(0, os.path.dirname(HERE))
import colorfix_reference as R  # noqa: E402

SHAPES = ((1, 3, 40, 56), (1, 3, 5, 40))


def load_reference(root):
    def refuse(*a, **k):
        raise RuntimeError("the stub torchvision.transforms was called")

    tv = types.ModuleType("torchvision")
    tv.__path__ = []
    tr = types.ModuleType("torchvision.transforms")
    tr.ToTensor = tr.ToPILImage = refuse
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    path = os.path.join(root, "Diffusion-Based-SR", "scripts", "wavelet_color_fix.py")
    spec = importlib.util.spec_from_file_location("reference_wavelet_color_fix", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def textured(rng, shape, amplitude):
    """A smooth field plus noise per plane, scaled so that the largest magnitude of the array is `amplitude`."""
    B, C, H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty(shape)
    for b in range(B):
        for c in range(C):
            f = rng.uniform(0.05, 0.4, 2)
            smooth = np.sin(f[0] * x + rng.uniform(0, 6)) * np.cos(f[1] * y + rng.uniform(0, 6))
            out[b, c] = rng.uniform(-0.3, 0.3) + rng.uniform(0.3, 0.7) * smooth + rng.uniform(0.1, 0.3) * rng.standard_normal((H, W))
    return (out * (amplitude / np.abs(out).max())).astype(np.float32)


def main(root):
    ref = load_reference(root)
    rng = np.random.default_rng(27)
    data = {}
    for n, shape in enumerate(SHAPES):
        content, style = textured(rng, shape, 1.2), textured(rng, shape, 1.0)
        c, s = torch.from_numpy(content), torch.from_numpy(style)
        high, low = ref.wavelet_decomposition(c)
        (mean_c, std_c), (mean_s, std_s) = ref.calc_mean_std(c), ref.calc_mean_std(s)
        rec = dict(content=content, style=style, blur1=ref.wavelet_blur(c, 1), blur16=ref.wavelet_blur(c, 16), high=high,
                   low=low, recon=ref.wavelet_reconstruction(c, s), mean_c=mean_c, std_c=std_c, mean_s=mean_s, std_s=std_s,
                   adain=ref.adaptive_instance_normalization(c, s))
        rec = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in rec.items()}
        assert all(v.dtype == np.float32 for v in rec.values())
        # the reference's own float32 results against the fp64 restatement, within the bounds the kernels are held to
        wb, wb2 = R.wavelet_bound(content), R.wavelet_bound(content, style)
        h64, l64 = R.wavelet_decomposition(content, dtype=np.float64)
        want = dict(blur1=(R.wavelet_blur(content, 1, np.float64), wb), blur16=(R.wavelet_blur(content, 16, np.float64), wb),
                    high=(h64, wb), low=(l64, wb), recon=(R.wavelet_reconstruction(content, style, dtype=np.float64), wb2),
                    adain=(R.adaptive_instance_normalization(content, style, np.float64), R.adain_bound(content, style)))
        for k, (w, bound) in want.items():
            frac = float((np.abs(rec[k] - w) / bound).max())
            print(f"case {n} {shape} {k:7s}: max error / bound = {frac:.3f}")
            if not frac <= 1.0:
                raise SystemExit(f"case {n} {k}: the reference's float32 output is outside the bound ({frac:.3f} of it)")
        for img, tag in ((content, "c"), (style, "s")):
            m64, s64 = R.calc_mean_std(img, dtype=np.float64)
            for k, w in (("mean_" + tag, m64), ("std_" + tag, s64)):
                # a float32 reduction of a few thousand values and its rounding: 2^-20 of the plane's magnitude
                err = float(np.abs(rec[k] - w).max())
                print(f"case {n} {shape} {k:7s}: max error = {err:.2e}")
                if not err <= 2.0 ** -20 * float(np.abs(img).max()):
                    raise SystemExit(f"case {n} {k}: the reference's statistic is {err:.2e} from fp64")
        data.update({f"c{n}_{k}": v for k, v in rec.items()})
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
