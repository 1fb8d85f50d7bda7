#!/usr/bin/env python3
"""The perceptual loss's criterion timed, loss and gradient per call: the reference's per-layer loop of torch operations
beside the one-launch multi-tensor criterion (engine.multi_pixel_loss -> ssg_mcrit_sums / ssg_mcrit_grad), on the same
GPU in the same run.

Shape: the five vgg19 features (conv1_2, conv2_2, conv3_4, conv4_4, conv5_4) of a 16 x 3 x 256 x 256 batch, 127.9 M
elements a side, L1 with KAIR's weights 0.1, 0.1, 1, 1, 1.  The features are random tensors: the network is not timed.
    loop     (a) `loss += F.l1_loss(x_k, g_k) * w_k` per layer and loss.backward(): the reference's criterion lines
    native   (b) engine.multi_pixel_loss(...) and .backward(): allocation of the K gradients and autograd included
    c_call   (c) the three bare launches on preallocated buffers: ssg_mcrit_sums (chunk sums, fold), ssg_mcrit_grad
A warm-up, then `--rounds` alternating windows of `--iters` calls each, device events around a window; the median window
and the min / max.  `device_ops` are the device activities torch's profiler records for one call (null if the profiler
is not available), `peak_MB` the peak of torch's allocator above what was allocated before a call that starts without
gradients, `temporaries_MB` that peak less the K gradients themselves (which (c) is handed preallocated).  The byte floor:
x and g read twice (the sums, the gradient) and the gradient written once, 20 bytes per element, at the 6.3 TB/s the
kernel guide gives for element-wise streams on the MI355X (its HBM3E peak is 8 TB/s).
`--sweep` times (c) on the profiling build for the chunk sizes 4,096, 8,192 and 16,384 (ssg_prof_mcrit_tuning): the A/B
behind ssg_mcrit_chunk().

    python tools/perceptual_time.py [--iters N] [--rounds R] [--warmup W] [--sweep] [--label TEXT] [--append] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bbl_time import compare, peak_bytes, window  # noqa: E402
from gan_time import device_ops  # noqa: E402

STREAM_BYTES_PER_S = 6.3e12   # element-wise streams on the MI355X (HBM3E peak: 8 TB/s)
FLOOR_BYTES = 20              # per element: x and g read twice, the gradient written once
SWEEP = (4096, 8192, 16384)
WEIGHTS = (0.1, 0.1, 1.0, 1.0, 1.0)


def feature_shapes(batch=16, side=256):
    return [(batch, c, side >> s, side >> s) for s, c in enumerate((64, 128, 256, 512, 512))]


def record(lines, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perceptual_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_time.py needs the MI355X")
    from ssl_amd import _lib, engine
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []
    shapes = feature_shapes()
    gen = torch.Generator(device=dev).manual_seed(1)
    gs = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    xs = [(g + 0.25 * torch.randn(s, device=dev, generator=gen)).requires_grad_(True) for g, s in zip(gs, shapes)]
    n_el = sum(g.numel() for g in gs)
    record(lines, shapes=shapes, elements=n_el, kind="l1", chunk=L.ssg_mcrit_chunk(), grid_cap=L.ssg_mcrit_grid_cap())
    stream = torch.cuda.current_stream().cuda_stream
    K = len(xs)
    px = np.asarray([t.data_ptr() for t in xs], dtype=np.uintp)
    pg = np.asarray([t.data_ptr() for t in gs], dtype=np.uintp)
    counts = np.asarray([t.numel() for t in xs], dtype=np.uintp)
    w = np.asarray([v / t.numel() for v, t in zip(WEIGHTS, xs)], dtype=np.float64)
    grads = [torch.empty_like(t) for t in gs]
    po = np.asarray([t.data_ptr() for t in grads], dtype=np.uintp)
    sums = torch.empty(K + 1, dtype=torch.float64, device=dev)
    coef = torch.ones(1, dtype=torch.float64, device=dev)
    kind = _lib.CONSTANTS["SSG_PIX_L1"]

    def loop():
        for t in xs:
            t.grad = None
        loss = 0
        for x, g, v in zip(xs, gs, WEIGHTS):
            loss += F.l1_loss(x, g) * v
        loss.backward()

    def native():
        for t in xs:
            t.grad = None
        engine.multi_pixel_loss(xs, gs, WEIGHTS, "l1").backward()

    def bare(lib):
        nbytes = lib.ssg_mcrit_workspace_bytes(K, counts.ctypes.data)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def run():
            _lib.check(lib.ssg_mcrit_sums(K, px.ctypes.data, pg.ctypes.data, counts.ctypes.data, w.ctypes.data, kind, 0.0,
                                          work.data_ptr(), nbytes, sums.data_ptr(), stream))
            _lib.check(lib.ssg_mcrit_grad(K, px.ctypes.data, pg.ctypes.data, po.ctypes.data, counts.ctypes.data,
                                          w.ctypes.data, kind, 0.0, sums.data_ptr(), coef.data_ptr(), stream))
        return run

    paths = [("loop", loop), ("native", native), ("c_call", bare(L))]
    res = compare(paths, args.iters, args.rounds, args.warmup)
    ops = {name: device_ops(fn) for name, fn in paths}
    peaks = {}
    for name, fn in paths:                        # (from a state without gradients: what one call adds at its peak)
        for t in xs:
            t.grad = None
        peaks[name] = peak_bytes(fn)
    grad_bytes = 4 * n_el
    floor_ms = FLOOR_BYTES * n_el / STREAM_BYTES_PER_S * 1e3
    for name, (med, lo, hi, peak) in res.items():
        rec = dict(path=name, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), windows=args.rounds,
                   iters=args.iters, device_ops=ops[name], peak_MB=round(peaks[name] / 2 ** 20, 2),
                   temporaries_MB=round(max(peaks[name] - (grad_bytes if name != "c_call" else 0), 0) / 2 ** 20, 2),
                   byte_floor_ms=round(floor_ms, 4), floor_share=round(floor_ms / med, 4),
                   achieved_TBps=round(FLOOR_BYTES * n_el / (med * 1e-3) / 1e12, 3))
        if name != "loop":
            rec.update(loop_over_this=round(res["loop"][0] / med, 2))
        record(lines, **rec)

    # the two results side by side, an observation: the native loss against the loop's, the largest gradient difference
    loop()
    torch.cuda.synchronize()
    ref_grads = [t.grad.clone() for t in xs]
    with torch.no_grad():
        ref_loss = sum(F.l1_loss(x, g) * v for x, g, v in zip(xs, gs, WEIGHTS))
    native()
    torch.cuda.synchronize()
    with torch.no_grad():
        nat_loss = engine.multi_pixel_loss(xs, gs, WEIGHTS, "l1")
    record(lines, observation="native against the loop on the same tensors", loss_loop=float(ref_loss),
           loss_native=float(nat_loss),
           max_grad_diff=max(float((t.grad - r).abs().max()) for t, r in zip(xs, ref_grads)),
           max_grad=max(float(r.abs().max()) for r in ref_grads))

    if args.sweep:
        P = _lib.lib_prof()
        P.ssg_prof_mcrit_tuning.restype, P.ssg_prof_mcrit_tuning.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
        cap = L.ssg_mcrit_grid_cap()
        runners = {}
        for chunk in SWEEP:
            _lib.check(P.ssg_prof_mcrit_tuning(chunk, cap))
            inner = bare(P)                       # (its workspace is sized under the candidate's chunk)

            def run(chunk=chunk, inner=inner):
                P.ssg_prof_mcrit_tuning(chunk, cap)
                inner()
            runners[chunk] = run
        for fn in runners.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {chunk: [] for chunk in SWEEP}
        for _ in range(args.rounds):
            for chunk, fn in runners.items():
                times[chunk].append(window(fn, args.iters))
        for chunk, t in times.items():
            record(lines, sweep="c_call", chunk=chunk, grid_cap=cap, chunks=int(sum(-(-int(c) // chunk) for c in counts)),
                   ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                   floor_share=round(floor_ms / statistics.median(t), 4))
        P.ssg_prof_mcrit_tuning(L.ssg_mcrit_chunk(), cap)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        if not args.append:
            f.write("# tools/perceptual_time.py: the criterion of the perceptual loss per call (loss and gradient) on the "
                    "MI355X over the five vgg19 features of a 16 x 3 x 256 x 256 batch: the reference's per-layer loop of "
                    "torch operations, engine.multi_pixel_loss with autograd, and the three bare launches; with --sweep "
                    "the chunk candidates on the profiling build.  byte floor: 20 bytes per element at 6.3 TB/s\n")
        f.write(f"# run {args.label}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
