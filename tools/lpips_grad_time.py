#!/usr/bin/env python3
"""The differentiable LPIPS term timed beside the package's torch lines, on the same GPU, the same features and in the
same run: the criterion alone and the whole generator branch of LPIPSWithDiscriminator.

Shapes: 1 x 3 x 512 x 512 (configs/autoencoder/autoencoder_kl_64x64x4_resi.yaml) and 4 x 3 x 256 x 256.  A random-weight
VGG16 LPIPS and the default discriminator (the timings do not depend on the values).  Per shape:
    bare_backward_1    ssg_lpips_layers_backward alone, side 1 (the reconstruction's, as the generator step needs)
    bare_backward_both the same launch writing both sides
    criterion          lpips_criterion forward + backward on precomputed VGG16 features (gradient to side 1)
    criterion_torch    the same with set_native_criteria(False): lpips_torch_lines and torch's autograd
    generator          LPIPSWithDiscriminator(optimizer_idx=0) on a reconstruction formed from a `last_layer` parameter,
                       forward and backward(): calculate_adaptive_weight's two autograd.grad(retain_graph=True) included,
                       so the criterion's backward runs twice
    generator_torch    the same with set_native_criteria(False)
A warm-up, then `--rounds` alternating windows of `--iters` calls, device events around a window; the median window and
the min / max.  `device_ops` are the device activities torch's profiler records for one call (null if the profiler is
not available), `peak_MB` the peak of torch's allocator above what was allocated before the call.  The byte floor of the
bare launch: both maps read once, 8 bytes per element pair, and 4 bytes per gradient element written, at the 6.3 TB/s the
kernel guide gives for element-wise streams on the MI355X (the second channel walk is meant to hit L2 and is not
counted).

    python tools/lpips_grad_time.py [--iters N] [--rounds R] [--warmup W] [--label TEXT] [--append] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bbl_time import compare  # noqa: E402
from gan_time import device_ops  # noqa: E402

STREAM_BYTES_PER_S = 6.3e12
SHAPES = ((1, 3, 512, 512), (4, 3, 256, 256))


def record(lines, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_grad_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_grad_time.py needs the MI355X")
    import featmetric_cases as cases
    from ssl_amd import _lib, distributions
    from ssl_amd.engine import address_array
    from ssl_amd.losses import contperceptual, lpips, set_native_criteria
    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    record(lines, unit=L.ssg_featmetric_unit(), grid_cap=L.ssg_featmetric_grid_cap(), device=torch.cuda.get_device_name(0))
    state = cases.lpips_state("vgg")[0]
    net = lpips.LPIPS(state).to(dev)
    lins = [p.detach() for p in net.lins]
    torch.manual_seed(0)
    crit = contperceptual.LPIPSWithDiscriminator(disc_start=0, kl_weight=1e-6, disc_weight=0.5, lpips_weights=state).to(dev)

    def switched_off(fn):
        def run():
            prev = set_native_criteria(False)
            try:
                return fn()
            finally:
                set_native_criteria(prev)
        return run

    for shape in SHAPES:
        gen = torch.Generator().manual_seed(11)
        target = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        base = (target + 0.2 * torch.randn(shape, generator=gen).to(dev)).clamp(-1, 1)
        hidden = 0.3 * torch.randn(shape, generator=gen).to(dev)
        last = torch.nn.Parameter(torch.full((1, 3, 1, 1), 0.5, device=dev))
        post = distributions.DiagonalGaussianDistribution(
            0.5 * torch.randn(shape[0], 8, shape[2] // 8, shape[3] // 8, generator=gen).to(dev))
        with torch.no_grad():
            f0 = [t.contiguous() for t in net.features(target)]
            f1 = [t.contiguous() for t in net.features(base)]
        leaves = [t.clone().requires_grad_(True) for t in f1]
        K, N = len(f0), shape[0]
        n_el = sum(t.numel() for t in f0)
        C, H, W = (np.ascontiguousarray([t.shape[i] for t in f0], dtype=np.int32) for i in (1, 2, 3))
        a0, a1, aw = (address_array([t.data_ptr() for t in ts]) for ts in (f0, f1, lins))
        g0, g1 = [torch.empty_like(t) for t in f0], [torch.empty_like(t) for t in f1]
        b0, b1 = (address_array([t.data_ptr() for t in ts]) for ts in (g0, g1))
        coef = torch.ones(N, device=dev)

        def bare(p0, p1):
            def run():
                _lib.check(L.ssg_lpips_layers_backward(K, N, a0.ctypes.data, a1.ctypes.data, aw.ctypes.data, C.ctypes.data,
                                                       H.ctypes.data, W.ctypes.data, coef.data_ptr(), p0, p1, stream))
            return run

        def criterion():
            for t in leaves:
                t.grad = None
            lpips.lpips_criterion(f0, leaves, lins).sum().backward()

        def generator():
            last.grad = None
            rec = base + hidden * last
            loss, _ = crit(target, rec, post, 0, 10, last_layer=last)
            loss.backward()

        paths = [("bare_backward_1", bare(None, b1.ctypes.data)), ("bare_backward_both", bare(b0.ctypes.data, b1.ctypes.data)),
                 ("criterion", criterion), ("criterion_torch", switched_off(criterion)),
                 ("generator", generator), ("generator_torch", switched_off(generator))]
        res = compare(paths, args.iters, args.rounds, args.warmup)
        ops = {p: device_ops(fn) for p, fn in paths}
        record(lines, shape=list(shape), layers=[list(t.shape[1:]) for t in f0], element_pairs=n_el)
        for p, (med, lo, hi, peak) in res.items():
            rec = dict(shape=list(shape), path=p, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                       windows=args.rounds, iters=args.iters, device_ops=ops[p], peak_MB=round(peak / 2 ** 20, 2))
            if p.startswith("bare"):
                nbytes = (8 + (4 if p.endswith("_1") else 8)) * n_el
                floor_ms = nbytes / STREAM_BYTES_PER_S * 1e3
                rec.update(byte_floor_ms=round(floor_ms, 4), floor_share=round(floor_ms / med, 4),
                           achieved_TBps=round(nbytes / (med * 1e-3) / 1e12, 3))
            if p in ("criterion", "generator"):
                rec.update(torch_over_this=round(res[p + "_torch"][0] / med, 3))
            record(lines, **rec)
        del f0, f1, leaves, g0, g1
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        if not args.append:
            f.write("# tools/lpips_grad_time.py: the differentiable LPIPS term per call on the MI355X -- the bare backward "
                    "launch, the criterion forward + backward on precomputed VGG16 features and the generator branch of "
                    "LPIPSWithDiscriminator, each beside the torch lines on the same GPU; byte floor: 8 bytes per element "
                    "pair read + 4 per gradient element written at 6.3 TB/s\n")
        f.write(f"# run {args.label}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
