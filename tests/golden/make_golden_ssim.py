"""Generate f28_ssim.npz FROM THE REFERENCE ITSELF: the KAIR fork's SSIM criterion.

Needs the reference tree (which never travels with this repository) and runs on the CPU:

    python tests/golden/make_golden_ssim.py <reference root>

It imports the reference's GAN-Based-SR/train_BSGRAN/models/loss_ssim.py by path (torch and numpy only).

Per case (prefix cN_): the float32 inputs `x`, `y`, `ws` (window_size), `avg` (size_average), `gout` (the upstream
gradient of the result: a scalar, or one value per image), the reference's own float32 `loss` (ssim(x, y, ws, avg)),
`gx`, `gy` (autograd of sum(gout * loss) through it) and `window` (create_window(ws, 1)[0, 0]); and `loss64`, `gx64`,
`gy64`: float64 autograd through the reference's _ssim with its float32 window widened to float64, the yardstick of the
restatement tests/ssim_reference.py.  The shape cases are drawn uniformly; the seven contents of
ssim_reference.CONTENTS are recorded at 1 x 2 x 36 x 40.

Before writing, the restatement's analytic gradient is held to 1e-11 of max|grad| of that float64 autograd and the
reference's float32 results to the derived bounds (where x == y the gradient's terms cancel to zero and the gap is
held to 1e-11 of the terms' size, ssim_reference.term_scale, instead); the script fails if one is outside.  Only DATA is stored; no
reference source text.
"""
import importlib.util
import os
import sys
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f28_ssim.npz")
sys.path.insert(0, os.path.dirname(HERE))
import ssim_reference as R  # noqa: E402

# (shape, window_size, size_average, upstream gradient, content)
CASES = [((1, 1, 1, 1), 11, True, 1.0, "uniform01"),
         ((1, 1, 7, 5), 11, True, 1.0, "uniform11"),
         ((1, 3, 11, 11), 3, True, 1.0, "uniform01"),
         ((1, 3, 11, 11), 7, True, -2.5, "uniform01"),
         ((2, 2, 20, 23), 11, False, (0.7, -1.3), "uniform01")] + \
        [((1, 2, 36, 40), 11, True, 1.0, name) for name in R.CONTENTS]


def load_reference(root):
    path = os.path.join(root, "GAN-Based-SR", "train_BSGRAN", "models", "loss_ssim.py")
    spec = importlib.util.spec_from_file_location("reference_loss_ssim", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, x, y, ws, avg, gout, dtype):
    a = x.to(dtype).clone().requires_grad_(True)
    b = y.to(dtype).clone().requires_grad_(True)
    if dtype == torch.float32:
        loss = ref.ssim(a, b, ws, avg)
    else:
        c = x.shape[1]
        loss = ref._ssim(a, b, ref.create_window(ws, c).to(dtype), ws, c, avg)
    (loss * torch.as_tensor(gout, dtype=dtype)).sum().backward()
    return loss.detach(), a.grad, b.grad


def main(root):
    ref = load_reference(root)
    torch.manual_seed(0)
    out = {}
    for n, (shape, ws, avg, gout, name) in enumerate(CASES):
        x, y = R.content(name, shape, seed=n)
        l32, gx32, gy32 = run(ref, x, y, ws, avg, gout, torch.float32)
        l64, gx64, gy64 = run(ref, x, y, ws, avg, gout, torch.float64)
        window = ref.create_window(ws, 1)[0, 0]
        assert torch.equal(window.double(), R.window(ws))
        numel = x.numel() if avg else x[0].numel()
        coef = torch.as_tensor(gout, dtype=torch.float64) / numel
        rx, ry = R.gradients(x, y, ws, coef)
        scale = max(float(gx64.abs().max()), float(gy64.abs().max()))
        if torch.equal(x, y):           # the gradient is zero analytically: max|grad| is rounding noise
            scale = R.term_scale(x, y, ws, coef)
        gap = max(float((rx - gx64).abs().max()), float((ry - gy64).abs().max()))
        assert gap <= 1e-11 * scale, (n, gap, scale)
        assert float((R.ssim(x, y, ws, avg) - l64).abs().max()) <= 1e-13, n
        lb, bx, by = R.bounds(x, y, ws, coef)
        lb = lb.mean() if avg else lb
        shares = (R.share(l32, l64, lb), R.share(gx32, gx64, bx), R.share(gy32, gy64, by))
        print(f"case {n:2d} {name:10s} {shape} ws {ws}: restatement gap {gap / max(scale, 1e-300):.1e} of max|grad|; "
              f"reference fp32 uses {shares[0]:.2e} / {shares[1]:.2e} / {shares[2]:.2e} of the loss / grad_x / grad_y "
              f"bound; its grad is off by {float((gx32 - gx64).abs().max()) / max(scale, 1e-300):.1e} of max|grad|")
        assert max(shares) <= 1.0, (n, shares)
        rec = dict(x=x, y=y, ws=ws, avg=int(avg), gout=np.asarray(gout, dtype=np.float64), loss=l32, gx=gx32, gy=gy32,
                   window=window, loss64=l64, gx64=gx64, gy64=gy64)
        for k, v in rec.items():
            out[f"c{n}_{k}"] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
