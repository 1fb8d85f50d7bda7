#!/usr/bin/env python3
"""The Adam step of a parameter set timed, per call: torch.optim.Adam in its three forms beside the one-launch step
(ssl_amd.optim.Adam -> ssg_adam_apply), on the same GPU in the same run.

Paths, Adam with lr 2e-4, betas (0.9, 0.99), weight_decay 0 (the reference's options/train/*SSL/*.yml):
    torch_default   torch.optim.Adam with its defaults (the reference's setting): on a GPU the _foreach_ implementation
    torch_fused     torch.optim.Adam(fused=True)
    torch_single    torch.optim.Adam(foreach=False): the per-tensor loop
    native          ssl_amd.optim.Adam.step: _init_group, the per-call pointer check and one ssg_adam_apply per group
    c_call          the bare ssg_adam_apply on the prebuilt tables
Sets: RRDBNet's parameter shapes (702 tensors, tools/ema_time.py's list) and the U-Net discriminator's
(UNetDiscriminatorSN, num_feat 64: 12 tensors), each path on its own copy of the parameters with fixed gradients.
A warm-up, then `--rounds` alternating windows of `--iters` calls each, device events around a window: `ms_*` is the time
per call of a window of back-to-back calls, so the larger of the host's and the device's time.  `host_ms` is the host's
time per call alone (time.perf_counter around a window's calls, before the wait for the device); `device_ops` and
`device_busy_us` are the device activities torch's profiler records for one call and the sum of their durations.  The
byte floor: p, m and v read and written, g read: 28 bytes per element at the 6.3 TB/s measured for streaming kernels.

    python tools/adam_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE] [--append]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bbl_time import compare  # noqa: E402
from ema_time import STREAM_BYTES_PER_S, module_of, record, rrdbnet_shapes  # noqa: E402

LR, BETAS = 2e-4, (0.9, 0.99)


def unet_discriminator_shapes(num_in_ch=3, num_feat=64):
    """The parameter shapes of UNetDiscriminatorSN in named_parameters() order (spectral norm keeps each weight's shape)."""
    f = num_feat
    return [(f, num_in_ch, 3, 3), (f,), (2 * f, f, 4, 4), (4 * f, 2 * f, 4, 4), (8 * f, 4 * f, 4, 4), (4 * f, 8 * f, 3, 3),
            (2 * f, 4 * f, 3, 3), (f, 2 * f, 3, 3), (f, f, 3, 3), (f, f, 3, 3), (1, f, 3, 3), (1,)]


def device_activity(fn):
    """(count, summed duration in us) of the device activities of one call; (None, None) without the profiler.  The
    optimizers wrap step() in a record_function range, which the profiler mirrors on the device as an annotation
    spanning the step's kernels: that is no operation and is left out."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA and not getattr(e, "is_user_annotation", False)]
        return len(ev), round(sum(e.time_range.elapsed_us() for e in ev), 1)
    except Exception:       # noqa: BLE001 -- reported as null, the timings stand
        return None, None


def host_ms(fn, iters, rounds):
    """The host's time per call: a window's calls without the wait for the device (the wait comes after the clock)."""
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        times.append((time.perf_counter() - t0) / iters * 1e3)
        torch.cuda.synchronize()
    return statistics.median(times)


def time_set(name, shapes, dev, args, lines):
    from ssl_amd import _lib, optim
    L = _lib.lib()
    makers = [("torch_default", lambda ps: torch.optim.Adam(ps, LR, betas=BETAS)),
              ("torch_fused", lambda ps: torch.optim.Adam(ps, LR, betas=BETAS, fused=True)),
              ("torch_single", lambda ps: torch.optim.Adam(ps, LR, betas=BETAS, foreach=False)),
              ("native", lambda ps: optim.Adam(ps, LR, betas=BETAS))]
    opts, nets = {}, {}
    for path, make in makers:
        net = module_of(shapes, dev, 1)
        gen = torch.Generator().manual_seed(2)
        for p in net.parameters():
            p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
        nets[path], opts[path] = net, make(list(net.parameters()))
        opts[path].step()
    n_el = sum(p.numel() for p in nets["native"].parameters())
    record(lines, set=name, tensors=len(shapes), elements=n_el, chunk=L.ssg_multi_chunk(), grid_cap=L.ssg_multi_grid_cap())
    plan = opts["native"]._plans[(0, 0)]
    assert plan.native
    stream = torch.cuda.current_stream().cuda_stream
    s = optim.scalars(LR, BETAS[0], BETAS[1], 1e-8, 0.0, False, 100.0)

    def c_call():
        _lib.check(L.ssg_adam_apply(plan.table.data_ptr(), plan.grads.data_ptr(), plan.n_chunks, ctypes.addressof(s), stream))

    paths = [(path, opts[path].step) for path, _ in makers] + [("c_call", c_call)]
    res = compare(paths, args.iters, args.rounds, args.warmup)
    activity = {path: device_activity(fn) for path, fn in paths}
    ops, busy = {k: v[0] for k, v in activity.items()}, {k: v[1] for k, v in activity.items()}
    host = {path: host_ms(fn, args.iters, 3) for path, fn in paths}
    floor_ms = 28 * n_el / STREAM_BYTES_PER_S * 1e3
    for path, (med, lo, hi, peak) in res.items():
        rec = dict(set=name, path=path, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                   windows=args.rounds, iters=args.iters, host_ms=round(host[path], 4), device_ops=ops[path],
                   device_busy_us=busy[path], peak_MB=round(peak / 2 ** 20, 2))
        if path == "c_call":
            rec.update(byte_floor_ms=round(floor_ms, 5), floor_share=round(floor_ms / med, 4), peak_used_TBps=6.3,
                       achieved_TBps=round(28 * n_el / (med * 1e-3) / 1e12, 3))
        if path != "native":
            rec.update(over_native=round(med / res["native"][0], 2))
        if path.startswith("torch") and busy[path] and busy["native"]:
            rec.update(device_over_native=round(busy[path] / busy["native"], 2))
        record(lines, **rec)
    # the host time of the per-call validation alone
    lists = ([], [], [], [], [], [])
    opt = opts["native"]
    opt._init_group(opt.param_groups[0], *lists)
    checks = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.iters):
            assert plan.validate(lists[0], lists[1], lists[2], lists[3])
        checks.append((time.perf_counter() - t0) / args.iters * 1e3)
    # and of a moved gradient set (zero_grad(set_to_none=True)): the address array refilled and uploaded, no wait
    sets, moves = [lists[1], [g.clone() for g in lists[1]]], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for i in range(args.iters):
            assert plan._move_grads(sets[(i + 1) % 2])
        moves.append((time.perf_counter() - t0) / args.iters * 1e3)
    torch.cuda.synchronize()
    record(lines, set=name, pointer_check_ms=round(statistics.median(checks), 4), tensors_checked=4 * len(shapes),
           grad_move_ms=round(statistics.median(moves), 4), rebuilds=plan.rebuilds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_time.txt"))
    ap.add_argument("--append", action="store_true", help="a further run of the tool into the same file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_time.py needs the MI355X")
    dev = torch.device("cuda:0")
    lines = []
    time_set("rrdbnet", rrdbnet_shapes(), dev, args, lines)
    time_set("unet_discriminator", unet_discriminator_shapes(), dev, args, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = ("# tools/adam_time.py: the Adam step of a parameter set per call on the MI355X: torch.optim.Adam with its defaults, "
            "with fused=True and with foreach=False, ssl_amd.optim.Adam.step and the bare ssg_adam_apply (RRDBNet's 702 shapes, "
            "the U-Net discriminator's 12); host time per call, device operations and device time of one call; the per-call "
            "pointer check's host time.  byte floor: 28 bytes per element at 6.3 TB/s\n")
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("# a second run of the tool\n" if args.append else head) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
