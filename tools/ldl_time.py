#!/usr/bin/env python3
"""LDL's artifact loss, forward + backward, timed with device events after a warm-up: the fused path
(ssl_amd.losses.ArtifactLoss -> ssg_ldl_loss, three launches) against the reference's torch formulation restated here
(get_refined_artifact_map + L1Loss as ldlssl_model.py:220-224 writes them: reflect pad, 7 x 7 unfold variance,
per-image variance, pow, masked write, two products, L1, and autograd's backward of each).

Shapes: LDLSSL's 64 x 3 x 128 x 128 and Real-ESRGAN's 12 x 3 x 256 x 256 (k = 7).  One JSON line per (shape, path),
plus the byte floor of the fused step: read output, GT, EMA once and output, GT again, write the gradient
(6 x 4 B per element), over the 8 TB/s HBM peak of the MI355X.

    python tools/ldl_time.py [--iters N] [--warmup W] [--fused-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, MI355X


def torch_ldl(o, g, e, k=7, lam=1.0):
    """The reference formulation (loss_util.py:106-161 + basic_loss.py's L1Loss), restated."""
    residual_ema = torch.sum(torch.abs(g - e), 1, keepdim=True)
    residual_sr = torch.sum(torch.abs(g - o), 1, keepdim=True)
    patch = torch.var(residual_sr.clone(), dim=(-1, -2, -3), keepdim=True) ** (1 / 5)
    pad = (k - 1) // 2
    rp = F.pad(residual_sr.clone(), pad=[pad, pad, pad, pad], mode='reflect')
    pixel = torch.var(rp.unfold(2, k, 1).unfold(3, k, 1), dim=(-1, -2), unbiased=True, keepdim=True)
    w = patch * pixel.squeeze(-1).squeeze(-1)
    w[residual_sr < residual_ema] = 0
    return lam * F.l1_loss(w * o, w * g, reduction='mean')


def time_it(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ldl_time.py needs the MI355X")
    from ssl_amd.losses import ArtifactLoss
    dev = torch.device("cuda:0")
    crit = ArtifactLoss(loss_weight=1.0, ksize=7)
    for shape in ((64, 3, 128, 128), (12, 3, 256, 256)):
        gen = torch.Generator(device="cpu").manual_seed(0)
        g = torch.rand(shape, generator=gen).to(dev)
        o = (g + 0.08 * torch.randn(shape, generator=gen).to(dev)).clamp(0, 1).requires_grad_(True)
        e = (g + 0.06 * torch.randn(shape, generator=gen).to(dev)).clamp(0, 1)

        def fused():
            o.grad = None
            crit(o, g, e).backward()

        def reference():
            o.grad = None
            torch_ldl(o, g, e).backward()

        n = o.numel()
        floor_ms = 6 * 4 * n / HBM_PEAK * 1e3
        paths = [("fused", fused)] + ([] if args.fused_only else [("torch", reference)])
        for name, fn in paths:
            ms = time_it(fn, args.iters, args.warmup)
            print(json.dumps({"shape": list(shape), "path": name, "ms": round(ms, 4), "iters": args.iters,
                              "floor_ms": round(floor_ms, 4), "floor_bytes": 6 * 4 * n,
                              "x_floor": round(ms / floor_ms, 2)}), flush=True)


if __name__ == "__main__":
    main()
