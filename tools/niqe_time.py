#!/usr/bin/env python3
"""NIQE timed: the fused call (ssl_amd.metrics.niqe -> ssg_niqe, five launches) on a model's float RGB tensors, beside
the reference's CPU seconds for the same shapes as tests/golden/make_golden_niqe.py --timing recorded them
(calculate_niqe image by image, in tests/golden/f26_niqe.npz: timing_shapes, timing_seconds).

Shapes: 1 x 3 x 2040 x 1356 (a DIV2K validation image, 294 blocks) and 16 x 3 x 256 x 256 (4 blocks each), crop 0.
A warm-up (which also uploads the parameters and the alpha table), then `--rounds` windows of `--iters` calls each,
device events around a window; the median window and the min / max.  The byte floor is the float image read once.

    python tools/niqe_time.py --params <niqe_pris_params.npz> [--iters N] [--rounds R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bbl_time import compare  # noqa: E402

HBM_BYTES_PER_S = 8e12   # MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default=os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "niqe_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("niqe_time.py needs the MI355X")
    from ssl_amd import metrics as M
    dev = torch.device("cuda:0")
    recorded = {}
    fixture = os.path.join(ROOT, "tests", "golden", "f26_niqe.npz")
    if os.path.exists(fixture):
        g = np.load(fixture)
        if "timing_seconds" in g.files:
            recorded = {tuple(int(v) for v in s): float(t) for s, t in zip(g["timing_shapes"], g["timing_seconds"])}
    lines = []
    for shape in ((1, 3, 2040, 1356), (16, 3, 256, 256)):
        gen = torch.Generator().manual_seed(shape[0])
        yy, xx = torch.meshgrid(torch.arange(shape[2]), torch.arange(shape[3]), indexing="ij")
        base = 0.5 + 0.35 * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)
        sr = (base[None, None] + 0.03 * torch.randn(shape, generator=gen)).to(dev).contiguous()

        def fused():
            return M.niqe(sr, 0, 'y', args.params)

        scores = fused().cpu().tolist()
        med, lo, hi, peak = compare([("fused", fused)], args.iters, args.rounds, args.warmup)["fused"]
        rec = dict(what="NIQE, Y, crop 0", shape=list(shape), path="fused", ms_median=round(med, 4), ms_min=round(lo, 4),
                   ms_max=round(hi, 4), windows=args.rounds, iters=args.iters, peak_MB=round(peak / 2 ** 20, 2),
                   byte_floor_ms=round(sr.numel() * 4 / HBM_BYTES_PER_S * 1e3, 5), score_first=scores[0])
        if shape in recorded:
            rec["reference_cpu_s"] = round(recorded[shape], 3)
            rec["reference_cpu_over_fused"] = round(recorded[shape] * 1e3 / med, 1)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/niqe_time.py: fused ssg_niqe per call; reference_cpu_s = the reference's calculate_niqe on the "
                "CPU for the same shape (tests/golden/f26_niqe.npz)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
