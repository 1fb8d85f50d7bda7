#!/usr/bin/env python3
"""Spectral normalisation of the U-Net discriminator's eight layers timed, per call: torch's per-layer hooks beside the
fused set (ssl_amd.spectral -> ssg_sn_forward / ssg_sn_backward), on the same GPU in the same run.

Paths, on UNetDiscriminatorSN(3, 64)'s eight normalised layers (4,374,528 weight elements, 17.5 MB), training mode:
    torch_forward / fused_forward     the weight refresh alone: every layer's hook (compute_weight with one power
                                      iteration, under autograd) / one refresh() of the fused set
    torch_fwd_bwd / fused_fwd_bwd     the refresh, L = sum_l <W_sn,l, C_l> and its backward into the weight_origs; the
                                      products with C_l and their sum are the same torch operations on both sides
    c_forward / c_backward            the bare ssg_sn_forward / ssg_sn_backward on preallocated blocks
    disc_torch / disc_fused           one whole discriminator forward + backward at 16 x 3 x 256 x 256
A warm-up, then `--rounds` alternating windows of `--iters` calls each, device events around a window: `ms_*` is the time
per call of a window of back-to-back calls, so the larger of the host's and the device's time.  `host_ms` is the host's
time per call alone; `device_ops` and `device_busy_us` are the device activities torch's profiler records for one call
and the sum of their durations.  The byte floor of the forward: three passes over the weights (t, s, and the division's
read; its write is a fourth), 3 x 17.5 MB at the 6.3 TB/s measured for streaming kernels.
`--tune` adds the A/B of the chunk size and grid cap on the profiling build (ssg_prof_sn_tuning).

    python tools/specnorm_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE] [--append] [--tune] [--no-disc]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from torch.nn.utils.spectral_norm import SpectralNorm  # noqa: E402

from adam_time import device_activity, host_ms  # noqa: E402
from bbl_time import compare  # noqa: E402
from ema_time import STREAM_BYTES_PER_S, record  # noqa: E402


def layers_of(net):
    return [(m, h) for m in net.modules() for h in m._forward_pre_hooks.values() if isinstance(h, SpectralNorm)]


def report(lines, what, paths, args, extra=None):
    res = compare(paths, args.iters, args.rounds, args.warmup)
    for path, fn in paths:
        med, lo, hi, peak = res[path]
        ops, busy = device_activity(fn)
        rec = dict(what=what, path=path, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                   windows=args.rounds, iters=args.iters, host_ms=round(host_ms(fn, args.iters, 3), 4), device_ops=ops,
                   device_busy_us=busy, peak_MB=round(peak / 2 ** 20, 2))
        if extra:
            rec.update(extra(path, med))
        record(lines, **rec)
    return res


def time_weights(dev, args, lines):
    from ssl_amd import _lib, archs
    torch.manual_seed(1)
    plain = archs.UNetDiscriminatorSN(3, 64, fused=False).to(dev).train()
    fused = archs.UNetDiscriminatorSN(3, 64).to(dev).train()
    fused.load_state_dict(plain.state_dict())
    pl, fl = layers_of(plain), fused.spectral.layers
    n_el = sum(m.weight_orig.numel() for m, _ in pl)
    gen = torch.Generator().manual_seed(2)
    Cs = [torch.randn(m.weight_orig.shape, generator=gen).to(dev) for m, _ in pl]
    L = _lib.lib()
    record(lines, layers=len(pl), elements=n_el, strip=L.ssg_sn_strip(), rows_a=L.ssg_sn_rows_a(),
           rows_b=L.ssg_sn_rows_b(), chunk=L.ssg_sn_chunk(), grid_cap=L.ssg_sn_grid_cap())

    def torch_forward():
        return [h.compute_weight(m, do_power_iteration=True) for m, h in pl]

    def fused_forward():
        fused.spectral.refresh()
        return [m.weight for m, _ in fl]

    def loss_backward(weights, modules):
        for m, _ in modules:
            m.weight_orig.grad = None
        sum((w * c).sum() for w, c in zip(weights, Cs)).backward()

    fused_forward()
    plan = fused.spectral._plans[0][2]
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty(plan.out_bytes // 4, device=dev)
    grad = torch.empty(plan.out_bytes // 4, device=dev)
    saved = torch.empty(plan.saved_bytes // 4, device=dev)
    ws = torch.empty(plan.ws_bytes // 8, dtype=torch.float64, device=dev)
    G = torch.randn(plan.out_bytes // 4, device=dev)
    addresses = torch.tensor([G.data_ptr() + 4 * o for o in plan.out_off], dtype=torch.int64).to(dev)

    def c_forward():
        _lib.check(L.ssg_sn_forward(plan.table.data_ptr(), plan.image.ctypes.data, 1, out.data_ptr(), plan.out_bytes,
                                    ws.data_ptr(), plan.ws_bytes, saved.data_ptr(), plan.saved_bytes, stream))

    def c_backward():
        _lib.check(L.ssg_sn_backward(plan.table.data_ptr(), plan.image.ctypes.data, addresses.data_ptr(), saved.data_ptr(),
                                     plan.saved_bytes, grad.data_ptr(), plan.out_bytes, ws.data_ptr(), plan.ws_bytes,
                                     stream))

    floor_ms = 3 * 4 * n_el / STREAM_BYTES_PER_S * 1e3

    def floors(path, med):
        if not path.startswith("c_"):
            return {}
        return dict(byte_floor_ms=round(floor_ms, 5), floor_share=round(floor_ms / med, 4))

    paths = [("torch_forward", torch_forward), ("fused_forward", fused_forward),
             ("torch_fwd_bwd", lambda: loss_backward(torch_forward(), pl)),
             ("fused_fwd_bwd", lambda: loss_backward(fused_forward(), fl)),
             ("c_forward", c_forward), ("c_backward", c_backward)]
    res = report(lines, "weights", paths, args, floors)
    record(lines, what="weights", forward_torch_over_fused=round(res["torch_forward"][0] / res["fused_forward"][0], 2),
           fwd_bwd_torch_over_fused=round(res["torch_fwd_bwd"][0] / res["fused_fwd_bwd"][0], 2),
           rebuilds=fused.spectral.rebuilds)
    return plain, fused


def time_tuning(args, lines):
    """The bare calls on the profiling build under other chunk sizes and grid caps (tables refilled per setting)."""
    from ssl_amd import _lib, archs
    dev = torch.device("cuda:0")
    with _lib.profile_build() as P:
        tune = P.ssg_prof_sn_tuning
        tune.restype, tune.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
        base = P.ssg_sn_chunk(), P.ssg_sn_grid_cap()
        try:
            for chunk, cap in ((2048, 1024), (4096, 1024), (8192, 1024), (16384, 1024), (4096, 512), (4096, 2048)):
                assert tune(chunk, cap) == 0
                net = archs.UNetDiscriminatorSN(3, 64).to(dev).train()
                with torch.no_grad():
                    net.spectral.refresh()
                plan = net.spectral._plans[0][2]

                def forward():
                    plan.forward(True)

                res = compare([("prof_forward", forward)], args.iters, args.rounds, args.warmup)
                record(lines, what="tuning", chunk=chunk, grid_cap=cap, ms_median=round(res["prof_forward"][0], 4),
                       ms_min=round(res["prof_forward"][1], 4))
        finally:
            torch.cuda.synchronize()
            tune(*base)


def time_discriminator(plain, fused, dev, args, lines):
    x = torch.randn(16, 3, 256, 256, device=dev)

    def step(net):
        def run():
            for p in net.parameters():
                p.grad = None
            net(x).mean().backward()
        return run

    res = report(lines, "discriminator 16x3x256x256", [("disc_torch", step(plain)), ("disc_fused", step(fused))], args)
    record(lines, what="discriminator 16x3x256x256", torch_over_fused=round(res["disc_torch"][0] / res["disc_fused"][0], 3),
           saved_ms=round(res["disc_torch"][0] - res["disc_fused"][0], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specnorm_time.txt"))
    ap.add_argument("--append", action="store_true", help="a further run of the tool into the same file")
    ap.add_argument("--tune", action="store_true")
    ap.add_argument("--no-disc", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specnorm_time.py needs the MI355X")
    dev = torch.device("cuda:0")
    lines = []
    plain, fused = time_weights(dev, args, lines)
    if args.tune:
        time_tuning(args, lines)
    if not args.no_disc:
        time_discriminator(plain, fused, dev, args, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = ("# tools/specnorm_time.py: spectral normalisation of UNetDiscriminatorSN's eight layers per call on the MI355X: "
            "torch's per-layer hooks and the fused set, forward alone and forward + backward, the bare C calls against the "
            "3 x 17.5 MB byte floor at 6.3 TB/s, and one whole discriminator forward + backward at 16 x 3 x 256 x 256\n")
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("# a second run of the tool\n" if args.append else head) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
