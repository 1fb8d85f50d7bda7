#!/usr/bin/env python3
"""StableSR's colour correction timed: the fused call (ssl_amd.colorfix.color_fix -> ssg_colorfix_wavelet, one launch;
ssg_colorfix_stats + ssg_colorfix_adain, three launches), with the clamp((x + 1) / 2, 0, 1) of the sampling scripts in
its epilogue, beside the torch formulation of the same step on the same GPU (the reference's expressions restated here:
replicate padding and a dilated grouped conv2d per level, two decompositions; var / mean per plane; then the clamp).

Shapes: 1 x 3 x 512 x 512 (the fork's sample size) and 4 x 3 x 2048 x 2048.  A warm-up, then `--rounds` alternating
windows of `--iters` calls each, device events around a window; the median window and the min / max.  The byte floor at
8 TB/s: two reads and one write per element for wavelet, three reads and one write for AdaIN.

    python tools/colorfix_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE]
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


def torch_wavelet(content, style, levels=5):
    C = content.shape[1]
    k = torch.tensor([0.25, 0.5, 0.25], dtype=content.dtype, device=content.device)
    kernel = torch.outer(k, k)[None, None].repeat(C, 1, 1, 1)

    def decompose(x):
        high = torch.zeros_like(x)
        for i in range(levels):
            r = 2 ** i
            low = F.conv2d(F.pad(x, (r, r, r, r), mode='replicate'), kernel, groups=C, dilation=r)
            high += x - low
            x = low
        return high, low

    return decompose(content)[0] + decompose(style)[1]


def torch_adain(content, style, eps=1e-5):
    def stats(x):
        flat = x.reshape(x.shape[0], x.shape[1], -1)
        return flat.mean(dim=2)[..., None, None], (flat.var(dim=2) + eps).sqrt()[..., None, None]

    (ms, ss), (mc, sc) = stats(style), stats(content)
    return (content - mc) / sc * ss + ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorfix_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colorfix_time.py needs the MI355X")
    from ssl_amd import colorfix as CF
    dev = torch.device("cuda:0")
    lines = []
    for shape in ((1, 3, 512, 512), (4, 3, 2048, 2048)):
        gen = torch.Generator().manual_seed(shape[0])
        yy, xx = torch.meshgrid(torch.arange(shape[2]), torch.arange(shape[3]), indexing="ij")
        base = 0.7 * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)
        s = (base[None, None] + 0.05 * torch.randn(shape, generator=gen)).clamp(-1, 1).to(dev).contiguous()
        c = (0.8 * base[None, None] + 0.1 + 0.2 * torch.randn(shape, generator=gen)).to(dev).contiguous()
        for kind, ref, accesses in (("wavelet", torch_wavelet, 3), ("adain", torch_adain, 4)):
            with torch.no_grad():
                paths = [("fused", lambda: CF.color_fix(c, s, kind=kind, out="unit")),
                         ("torch", lambda: torch.clamp((ref(c, s) + 1) / 2, 0, 1))]
                diff = float((paths[0][1]() - paths[1][1]()).abs().max())
                res = compare(paths, args.iters, args.rounds, args.warmup)
            for name, (med, lo, hi, peak) in res.items():
                rec = dict(what=f"color_fix {kind}, out unit", shape=list(shape), path=name, ms_median=round(med, 4),
                           ms_min=round(lo, 4), ms_max=round(hi, 4), windows=args.rounds, iters=args.iters,
                           peak_MB=round(peak / 2 ** 20, 2),
                           byte_floor_ms=round(c.numel() * 4 * accesses / HBM_BYTES_PER_S * 1e3, 5),
                           max_abs_fused_minus_torch=diff)
                if name == "torch":
                    rec["torch_over_fused"] = round(med / res["fused"][0], 2)
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/colorfix_time.py: ssl_amd.colorfix.color_fix (fused) and the torch formulation of the same step, "
                "per call, both on the MI355X; byte_floor_ms at 8 TB/s\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
