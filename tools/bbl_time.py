#!/usr/bin/env python3
"""BebyGAN's best-buddy loss (forward + backward) and flat mask, timed with device events: the native path
(ssl_amd.losses.BestBuddyLoss -> ssg_bbl_loss, four launches; get_flat_mask -> ssg_flat_mask, one) against the
reference's torch formulation restated here (BBL.forward as bebyganssl_model.py:541-565 writes it -- unfold, two
bicubic levels, two dense bmm score matrices, clamps, min, gather -- then F.l1_loss and autograd's backward;
get_flat_mask as :93-104 writes it: reflect pad, 121-tap unfold, torch.std, threshold).

Shapes: the configured 16 x 3 x 192 x 192 (N = 4,096 rows, M = 5,376 candidates, d = 27) and 4 x 3 x 192 x 192.
Each path: a warm-up, then `--rounds` windows of `--iters` calls each, the two paths alternating window by window;
the median window and the min / max are reported, with the peak device memory of one call
(torch.cuda.max_memory_allocated above what was allocated before it).  The search's arithmetic floor is
B N M (d + 1) 2 FLOP over the 157 TF fp32 matrix peak.

    python tools/bbl_time.py [--iters N] [--rounds R] [--warmup W] [--native-only] [--search-only]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MFMA_F32_PEAK = 157e12   # FLOP/s, MI355X


def _pairwise(x, y):
    x_norm = (x ** 2).sum(dim=2).unsqueeze(2)
    y_norm = (y ** 2).sum(dim=2).unsqueeze(1)
    return torch.clamp(x_norm + y_norm - 2.0 * torch.bmm(x, y.transpose(1, 2)), 0.0)


def torch_bbl_loss(x, gt, alpha=1.0, beta=1.0, k=3, s=3):
    """The reference formulation of the search and its loss, restated."""
    p1 = F.unfold(x, kernel_size=k, padding=0, stride=s).permute(0, 2, 1).contiguous()
    p2 = F.unfold(gt, kernel_size=k, padding=0, stride=s).permute(0, 2, 1).contiguous()
    levels = [p2]
    for f in (0.5, 0.25):
        low = F.interpolate(gt, scale_factor=f, mode='bicubic', align_corners=False)
        levels.append(F.unfold(low, kernel_size=k, padding=0, stride=s).permute(0, 2, 1).contiguous())
    cat = torch.cat(levels, 1)
    score = alpha * _pairwise(p1, cat) + beta * _pairwise(p2, cat)
    _, ind = torch.min(score, dim=2)
    sel = torch.gather(cat, dim=1, index=ind.unsqueeze(-1).expand(-1, -1, cat.shape[-1]))
    return F.l1_loss(p1, sel, reduction='mean')


def torch_flat_mask(img, kernel_size=11, std_thresh=0.025):
    B, _, H, W = img.size()
    r, g, b = torch.unbind(img, dim=1)
    lum = (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=1)
    pad = kernel_size // 2
    unf = F.unfold(F.pad(lum, (pad, pad, pad, pad), mode='reflect'), kernel_size=kernel_size, padding=0, stride=1)
    return torch.lt(torch.std(unf, dim=1, keepdim=True).view(B, 1, H, W), std_thresh).float()


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def compare(paths, iters, rounds, warmup):
    """paths: [(name, fn)].  Alternating windows; {name: (median, min, max, peak bytes)}."""
    peaks = {name: peak_bytes(fn) for name, fn in paths}
    for _, fn in paths:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in paths}
    for _ in range(rounds):
        for name, fn in paths:
            times[name].append(window(fn, iters))
    return {name: (statistics.median(t), min(t), max(t), peaks[name]) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--search-only", action="store_true", help="one native step per shape and nothing else (for a "
                    "kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bbl_time.py needs the MI355X")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import bbl_reference as R
    from ssl_amd.losses import BestBuddyLoss, get_flat_mask
    dev = torch.device("cuda:0")
    crit = BestBuddyLoss()
    for shape in ((16, 3, 192, 192), (4, 3, 192, 192)):
        rng = np.random.default_rng(shape[0])
        gt_cpu = R.textured_gt(rng, shape)
        gt = gt_cpu.to(dev)
        x = R.degraded(rng, gt_cpu, 2, 0.1).to(dev).requires_grad_(True)

        def native():
            x.grad = None
            crit(x, gt).backward()

        def reference():
            x.grad = None
            torch_bbl_loss(x, gt).backward()

        if args.search_only:
            for _ in range(10):
                native()
            torch.cuda.synchronize()
            continue
        B, N, M, d = shape[0], 4096, 5376, 27
        flop = 2.0 * B * N * M * (d + 1)
        floor_ms = flop / MFMA_F32_PEAK * 1e3
        paths = [("native", native)] + ([] if args.native_only else [("torch", reference)])
        res = compare(paths, args.iters, args.rounds, args.warmup)
        for name, (med, lo, hi, peak) in res.items():
            print(json.dumps({"what": "best-buddy loss fwd+bwd", "shape": list(shape), "path": name,
                              "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                              "windows": args.rounds, "iters": args.iters, "peak_MB": round(peak / 2 ** 20, 1),
                              "search_floor_ms": round(floor_ms, 4), "search_GFLOP": round(flop / 1e9, 2)}), flush=True)
        if "torch" in res:
            print(json.dumps({"what": "best-buddy loss fwd+bwd", "shape": list(shape),
                              "torch_over_native": round(res["torch"][0] / res["native"][0], 2)}), flush=True)
        with torch.no_grad():
            mpaths = [("native", lambda: get_flat_mask(gt))] + \
                     ([] if args.native_only else [("torch", lambda: torch_flat_mask(gt))])
            res = compare(mpaths, args.iters, args.rounds, args.warmup)
        for name, (med, lo, hi, peak) in res.items():
            print(json.dumps({"what": "flat mask k=11", "shape": list(shape), "path": name, "ms_median": round(med, 4),
                              "ms_min": round(lo, 4), "ms_max": round(hi, 4), "windows": args.rounds,
                              "iters": args.iters, "peak_MB": round(peak / 2 ** 20, 1)}), flush=True)
        if "torch" in res:
            print(json.dumps({"what": "flat mask k=11", "shape": list(shape),
                              "torch_over_native": round(res["torch"][0] / res["native"][0], 2)}), flush=True)


if __name__ == "__main__":
    main()
