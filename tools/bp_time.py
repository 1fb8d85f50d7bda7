#!/usr/bin/env python3
"""BebyGAN's back-projection loss (forward + backward), timed with device events: the native path
(ssl_amd.losses.BackProjectionLoss -> ssg_bp_loss, two launches) against the reference's torch formulation restated
here (imresize on its integer-factor path as bebyganssl_model.py:351-373 and :164-196 write it -- per axis a zero
buffer, one copy of the image and one single-row copy per padded row in front and behind from a Python loop, then a
1 -> 1 channel 4s x 4s conv2d at stride s on the planes -- then F.l1_loss and autograd's backward through every one of
those copies).

Shapes: the configured 16 x 3 x 192 x 192 and 4 x 3 x 192 x 192 at s = 4.  Each path: a warm-up, then `--rounds`
windows of `--iters` calls each, the two paths alternating window by window; the median window and the min / max are
reported, with the peak device memory of one call (torch.cuda.max_memory_allocated above what was allocated before
it) and the wall time the host spends issuing one native call.  The byte floor of the native call is (2 P H W + 2 P h w) 4 B -- the output read, its gradient written, lq read,
the signs written and read once counted as one pass -- over 8 TB/s.

    python tools/bp_time.py [--iters N] [--rounds R] [--warmup W] [--native-only] [--trace]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bbl_time import compare  # noqa: E402

HBM_BYTES_PER_S = 8e12   # MI355X


def _taps(s):
    K = 4 * s if s % 2 == 0 else 4 * s - 1
    r = ((torch.arange(K, dtype=torch.float64) - (K - 1) / 2) / s).abs()
    c = torch.where(r <= 1, 1.5 * r ** 3 - 2.5 * r ** 2 + 1,
                    torch.where(r <= 2, -0.5 * r ** 3 + 2.5 * r ** 2 - 4 * r + 2, torch.zeros_like(r)))
    return (c / c.sum()).float()


def _sym_pad(t, dim, p):
    """Symmetric padding of axis `dim` by p per side, in the operations the torch formulation costs: a zero buffer,
    one bulk copy of the interior, and one single-slice copy for each of the 2p padded positions.  The source of a
    padded position is the contract's symmetric index (tests/bp_reference.sym_index: -1-i reads i, n+i reads n-1-i)."""
    n = t.shape[dim]
    sides = list(t.shape)
    sides[dim] = n + 2 * p
    out = torch.zeros(sides, dtype=t.dtype, device=t.device)
    out.narrow(dim, p, n).copy_(t)
    for q in list(range(-p, 0)) + list(range(n, n + p)):
        src = -1 - q if q < 0 else 2 * n - 1 - q
        out.select(dim, q + p).copy_(t.select(dim, src))
    return out


def torch_bp_loss(x, lq, k2, s):
    """The torch formulation of the term: every plane as a one-channel image, padded axis by axis, correlated with
    the K x K tap table at stride s, then the mean absolute difference from lq."""
    p = (k2.shape[-1] - s) // 2
    planes = x.reshape(-1, 1, *x.shape[-2:])
    y = F.conv2d(_sym_pad(_sym_pad(planes, -2, p), -1, p), k2, stride=s)
    return F.l1_loss(y.reshape(lq.shape), lq)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--trace", action="store_true", help="ten native steps per shape and nothing else (for a kernel "
                    "trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bp_time.py needs the MI355X")
    from ssl_amd.losses import BackProjectionLoss
    dev = torch.device("cuda:0")
    s = 4
    crit = BackProjectionLoss(scale=s)
    w = _taps(s)
    k2 = torch.outer(w, w)[None, None].to(dev)
    for shape in ((16, 3, 192, 192), (4, 3, 192, 192)):
        gen = torch.Generator().manual_seed(shape[0])
        B, C, H, W = shape
        x = torch.rand(shape, generator=gen).to(dev).requires_grad_(True)
        lq = torch.rand((B, C, H // s, W // s), generator=gen).to(dev)

        def native():
            x.grad = None
            crit(x, lq).backward()

        def reference():
            x.grad = None
            torch_bp_loss(x, lq, k2, s).backward()

        if args.trace:
            for _ in range(10):
                native()
            torch.cuda.synchronize()
            continue
        # the two formulations agree before they are timed
        native()
        g_native, l_native = x.grad.clone(), float(crit(x, lq))
        reference()
        l_torch = float(torch_bp_loss(x, lq, k2, s))
        agree = float((g_native - x.grad).abs().max() / x.grad.abs().max())
        P, h, wo = B * C, H // s, W // s
        floor_ms = (2 * P * H * W + 2 * P * h * wo) * 4 / HBM_BYTES_PER_S * 1e3
        paths = [("native", native)] + ([] if args.native_only else [("torch", reference)])
        res = compare(paths, args.iters, args.rounds, args.warmup)
        for name, (med, lo, hi, peak) in res.items():
            print(json.dumps({"what": "back-projection loss fwd+bwd", "shape": list(shape), "s": s, "path": name,
                              "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                              "windows": args.rounds, "iters": args.iters, "peak_MB": round(peak / 2 ** 20, 2),
                              "byte_floor_ms": round(floor_ms, 5)}), flush=True)
        # the host's share: the wall time the CPU spends issuing one native call (no synchronisation inside the loop)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            native()
        host_ms = (time.perf_counter() - t0) * 1e3 / args.iters
        torch.cuda.synchronize()
        print(json.dumps({"what": "back-projection loss fwd+bwd", "shape": list(shape), "path": "native",
                          "host_issue_ms": round(host_ms, 4)}), flush=True)
        if "torch" in res:
            print(json.dumps({"what": "back-projection loss fwd+bwd", "shape": list(shape),
                              "torch_over_native": round(res["torch"][0] / res["native"][0], 2),
                              "loss_native": l_native, "loss_torch": l_torch,
                              "grad_max_rel_diff": agree}), flush=True)


if __name__ == "__main__":
    main()
