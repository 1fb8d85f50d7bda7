#!/usr/bin/env python3
"""KAIR's SSIM criterion timed: loss and gradient of the fused call (ssl_amd.losses.ssim -> ssg_ssim_loss, two launches)
beside the torch formulation of the same contract on the same GPU (five grouped 11 x 11 conv2d, the map, its mean and
autograd's replay), and the bare C call on preallocated buffers (what the two launches cost without the Python around
them).

Shapes: 48 x 3 x 256 x 256 (batch and H_size of the BSRGAN-SSL configuration) and 1 x 3 x 64 x 64.  A warm-up, then
`--rounds` alternating windows of `--iters` calls each, device events around a window; the median window and the min /
max.  The byte floor at 8 TB/s: two reads and one store per element, twelve bytes; `floor_share` is the floor over the
median.

    python tools/ssim_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bbl_time import compare  # noqa: E402

HBM_BYTES_PER_S = 8e12   # MI355X


def torch_ssim(x, y, window):
    """The contract in torch: 'same' grouped convolutions under the (C,1,11,11) window, fp32."""
    c, pad = x.shape[1], window.shape[-1] // 2
    blur = lambda t: F.conv2d(t, window, padding=pad, groups=c)   # noqa: E731
    mx, my = blur(x), blur(y)
    sx, sy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    s = ((2 * mx * my + 0.01 ** 2) * (2 * sxy + 0.03 ** 2)) / ((mx * mx + my * my + 0.01 ** 2) * (sx + sy + 0.03 ** 2))
    return s.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_time.py needs the MI355X")
    from ssl_amd import _lib, engine
    from ssl_amd.losses import create_window, ssim
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []
    for shape in ((48, 3, 256, 256), (1, 3, 64, 64)):
        gen = torch.Generator().manual_seed(shape[0])
        x = torch.rand(shape, generator=gen).to(dev).requires_grad_(True)
        y = (x.detach() + 0.1 * torch.randn(shape, generator=gen).to(dev)).clamp(0, 1)
        window = create_window(11, shape[1]).to(dev)
        B, C, H, W = shape
        sums = torch.empty(B + 1, dtype=torch.float64, device=dev)
        grad = torch.empty(shape, dtype=torch.float32, device=dev)
        nb = L.ssg_ssim_workspace_bytes(B, C, H, W)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        xd = x.detach()

        def fused():
            x.grad = None
            ssim(x, y).backward()

        def reference():
            x.grad = None
            torch_ssim(x, y, window).backward()

        def c_call():
            _lib.check(L.ssg_ssim_loss(xd.data_ptr(), y.data_ptr(), B, C, H, W, 11, grad.data_ptr(), sums.data_ptr(),
                                       ws.data_ptr(), nb, engine._stream()))

        def c_loss_only():
            _lib.check(L.ssg_ssim_loss(xd.data_ptr(), y.data_ptr(), B, C, H, W, 11, None, sums.data_ptr(),
                                       ws.data_ptr(), nb, engine._stream()))

        fused()
        g_fused, l_fused = x.grad.clone(), float(ssim(x, y).detach())
        reference()
        diff = float((g_fused - x.grad).abs().max() / x.grad.abs().max())
        l_diff = abs(l_fused - float(torch_ssim(x, y, window).detach()))
        res = compare([("fused", fused), ("torch", reference), ("c_call", c_call), ("c_loss_only", c_loss_only)],
                      args.iters, args.rounds, args.warmup)
        floor_ms = x.numel() * 12 / HBM_BYTES_PER_S * 1e3
        for name, (med, lo, hi, peak) in res.items():
            rec = dict(what="ssim loss + grad_x" if name != "c_loss_only" else "ssim loss alone", shape=list(shape),
                       path=name, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), windows=args.rounds,
                       iters=args.iters, peak_MB=round(peak / 2 ** 20, 2))
            if name != "c_loss_only":
                rec.update(byte_floor_ms=round(floor_ms, 5), floor_share=round(floor_ms / med, 4))
            if name == "torch":
                rec.update(torch_over_fused=round(med / res["fused"][0], 2),
                           torch_over_c_call=round(med / res["c_call"][0], 2),
                           max_grad_diff_over_max_grad=diff, loss_diff=l_diff)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/ssim_time.py: ssl_amd.losses.ssim(x, y).backward() (fused), the torch formulation of the same "
                "contract and the bare C call, per call, all on the MI355X; byte_floor_ms: 12 bytes per element at 8 TB/s\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
