#!/usr/bin/env python3
"""The validation metrics (PSNR and SSIM on Y, crop 4), timed: the fused call (ssl_amd.metrics.psnr_ssim ->
ssg_psnr_ssim, two launches) against the same formulas in torch on the same GPU (quantise, crop, Y in fp64, then the
five 11 x 11 moments as one fp64 depthwise F.conv2d) and against the CPU path a validation loop runs today (the
device-to-host copy of both tensors, then the numpy restatement tests/metrics_reference.py of tensor2img +
calculate_psnr + calculate_ssim; one image at a time, wall clock).

Shapes: 1 x 3 x 2040 x 1356 (a DIV2K validation image) and 16 x 3 x 256 x 256.  GPU paths: a warm-up, then `--rounds`
windows of `--iters` calls each, alternating window by window, device events; the median window and the min / max.
The byte floor of the fused call is both float images read once, 2 B C H W 4 bytes, over 8 TB/s; what the kernel
actually requests is more (each 32 x 16 map tile loads its 42 x 26 halo: 2.13 x, mostly served by the caches).

    python tools/metrics_time.py [--iters N] [--rounds R] [--warmup W] [--cpu-images K] [--out profiles/metrics_time.txt]
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


def torch_psnr_ssim(sr, gt, crop, window):
    """The same formulas in torch ops, fp64 from the Y plane on: (N,2) {PSNR, SSIM}."""
    def plane(t):
        q = (t.clamp(0, 1) * 255.0).round()[..., crop:t.shape[-2] - crop, crop:t.shape[-1] - crop].double() / 255.0
        return ((24.966 * q[:, 2:3] + 128.553 * q[:, 1:2] + 65.481 * q[:, 0:1]) + 16.0) / 255.0 * 255.0
    a, b = plane(sr), plane(gt)
    mse = ((a - b) ** 2).mean(dim=(1, 2, 3))
    psnr = 10.0 * torch.log10(255.0 * 255.0 / mse)
    m = F.conv2d(torch.cat([a, b, a * a, b * b, a * b], 1), window, groups=5)
    mu1, mu2, exx, eyy, exy = m.unbind(1)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s1, s2, s12 = exx - mu1 * mu1, eyy - mu2 * mu2, exy - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return torch.stack([psnr, ssim.mean(dim=(1, 2))], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-images", type=int, default=1, help="images the CPU path is timed on per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_time.py needs the MI355X")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import metrics_reference as R
    from ssl_amd import metrics as M
    dev = torch.device("cuda:0")
    crop = 4
    g = torch.as_tensor(R.taps())
    window = torch.outer(g, g)[None, None].repeat(5, 1, 1, 1).to(dev)
    lines = []

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        lines.append(line)

    for shape in ((1, 3, 2040, 1356), (16, 3, 256, 256)):
        gen = torch.Generator().manual_seed(shape[0])
        gt = torch.rand(shape, generator=gen).to(dev)
        sr = (gt + 0.03 * torch.randn(shape, generator=gen).to(dev)).contiguous()
        what = {"what": "PSNR + SSIM, Y, crop 4", "shape": list(shape)}

        def fused():
            return M.psnr_ssim(sr, gt, crop, True)

        def in_torch():
            return torch_psnr_ssim(sr, gt, crop, window)

        agree = (fused() - in_torch()).abs().max(0).values.cpu().tolist()
        floor_ms = 2 * sr.numel() * 4 / HBM_BYTES_PER_S * 1e3
        res = compare([("fused", fused), ("torch", in_torch)], args.iters, args.rounds, args.warmup)
        for name, (med, lo, hi, peak) in res.items():
            emit(dict(what, path=name, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                      windows=args.rounds, iters=args.iters, peak_MB=round(peak / 2 ** 20, 2),
                      byte_floor_ms=round(floor_ms, 5),
                      GB_per_s_of_floor_bytes=round(2 * sr.numel() * 4 / (med * 1e-3) / 1e9, 1)))
        # the CPU path: copy to the host, quantise, metrics, image by image
        torch.cuda.synchronize()
        n = min(args.cpu_images, shape[0])
        t0 = time.perf_counter()
        cpu = []
        for i in range(n):
            a, b = R.quantise(sr[i].cpu().numpy()), R.quantise(gt[i].cpu().numpy())
            pa, pb = R.planes(a, crop, True), R.planes(b, crop, True)
            cpu.append((R.psnr(pa, pb), R.ssim(pa, pb, "2d")))
        cpu_ms = (time.perf_counter() - t0) * 1e3 / n
        got = fused()[:n].cpu().tolist()
        emit(dict(what, path="cpu restatement incl. device-to-host copy", ms_per_image=round(cpu_ms, 2), images=n,
                  ms_per_batch=round(cpu_ms * shape[0], 2)))
        emit(dict(what, torch_over_fused=round(res["torch"][0] / res["fused"][0], 2),
                  cpu_batch_over_fused=round(cpu_ms * shape[0] / res["fused"][0], 1),
                  max_abs_diff_fused_vs_torch={"psnr": agree[0], "ssim": agree[1]},
                  max_abs_diff_fused_vs_cpu={"psnr": max(abs(g[0] - c[0]) for g, c in zip(got, cpu)),
                                             "ssim": max(abs(g[1] - c[1]) for g, c in zip(got, cpu))}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/metrics_time.py: fused ssg_psnr_ssim vs the same formulas in torch (fp64 depthwise conv2d) vs "
                "the CPU restatement\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
