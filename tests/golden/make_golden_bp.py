"""Generate f20_bp.npz FROM THE REFERENCE ITSELF: BebyGAN's imresize on its integer-factor path and the
back-projection loss built on it.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_bp.py <reference root>

It imports the reference's GAN-Based-SR/basicsr/models/bebyganssl_model.py through make_golden_bbl.load_reference (the
stub recipe described there).  Then, on the CPU in fp32, it runs discrete_kernel('cubic', 1 / s) for s = 2, 3, 4 and,
per case, imresize(x, scale=1 / s), the caller's loss (bebyganssl_model.py:727-731 with pixel_bp_opt: L1Loss, weight
1.0, mean, i.e. F.l1_loss(.., 'mean')) and the autograd gradient of that loss with respect to x.

Cases (prefix cN_): 1x3x24x20, 1x3x26x23, 1x1x6x7 (the smallest sides), 1x3x8x9 (one pixel under both mirrors) at
s = 4; 1x3x15x14 at s = 3; 2x1x10x12 at s = 2.  x is seeded uniform noise, lq the reference's own output plus
0.05 N(0,1).  Then (prefix h_, d3_, d2_) an fp16 4-D input, a 3-D and a 2-D input with their outputs.

Only DATA is stored (inputs, expected outputs); no reference source text.
"""
import os
import sys
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_bbl import load_reference  # noqa: E402

CASES = [((1, 3, 24, 20), 4), ((1, 3, 26, 23), 4), ((1, 1, 6, 7), 4), ((1, 3, 15, 14), 3), ((2, 1, 10, 12), 2),
         ((1, 3, 8, 9), 4)]


def case(ref, gen, shape, s):
    x = torch.rand(shape, generator=gen)
    with torch.no_grad():
        y0 = ref.imresize(x, scale=1 / s)
    lq = y0 + 0.05 * torch.randn(y0.shape, generator=gen)
    out = x.clone().requires_grad_(True)
    y = ref.imresize(out, scale=1 / s)
    loss = F.l1_loss(y, lq, reduction="mean")
    loss.backward()
    return dict(x=x.numpy(), lq=lq.numpy(), s=np.int32(s), y=y.detach().numpy(), loss=np.float32(loss.item()),
                grad=out.grad.numpy())


def main():
    ref = load_reference(sys.argv[1])
    gen = torch.Generator().manual_seed(20)
    out = {}
    for s in (2, 3, 4):
        out[f"table_s{s}"] = ref.discrete_kernel('cubic', 1 / s).numpy()
    for i, (shape, s) in enumerate(CASES):
        d = case(ref, gen, shape, s)
        for key, v in d.items():
            out[f"c{i}_{key}"] = v
        print(f"c{i}: shape {shape} s {s} -> {d['y'].shape} loss {float(d['loss']):.6g}")
    out["n_cases"] = np.int32(len(CASES))
    xh = torch.rand((1, 2, 12, 16), generator=gen).half()
    out["h_x"], out["h_y"] = xh.numpy(), ref.imresize(xh, scale=1 / 4).numpy()
    x3 = torch.rand((2, 9, 13), generator=gen)
    out["d3_x"], out["d3_y"] = x3.numpy(), ref.imresize(x3, scale=1 / 3).numpy()
    x2 = torch.rand((11, 8), generator=gen)
    out["d2_x"], out["d2_y"] = x2.numpy(), ref.imresize(x2, scale=1 / 2).numpy()
    for k in ("h", "d3", "d2"):
        print(f"{k}: {out[k + '_x'].shape} {out[k + '_x'].dtype} -> {out[k + '_y'].shape} {out[k + '_y'].dtype}")
    path = os.path.join(HERE, "f20_bp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
