#!/usr/bin/env python3
"""The LPIPS and DISTS criteria timed per call beside the packages' torch lines, on the same GPU, the same features and
in the same run, and their share of the whole metric call with its network.

Shapes: 1 x 3 x 2040 x 1356 (a DIV2K validation image) and 16 x 3 x 256 x 256.  Networks: LPIPS('alex'), LPIPS('vgg'),
DISTS with random weights (the timings do not depend on the values).  Per network and shape:
    c_call       the two bare launches on a preallocated workspace (ssg_lpips_layers / ssg_dists_score)
    torch_lines  the packages' criterion lines (metrics_feat.lpips_torch_lines / dists_torch_lines) on the same features
    module       the whole metric call, both network passes included, with the kernels
    module_torch the same with set_native_criteria(False)
A warm-up, then `--rounds` alternating windows, device events around a window; the median window and the min / max.  A
window holds as many calls of its path as fill `--window-ms` of device time (at least `--iters`, at most 2,000; the
count is recorded as `iters`), sized from a trial window after the warm-up: the short paths take 0.16 ms a call, and a
window of five such calls would be read off a sub-millisecond interval.  `device_ops` are the device activities
torch's profiler records for one call (null if the profiler is not available), `peak_MB` the peak of torch's allocator above what was allocated before the call: the criterion's
temporaries for the first two paths.  The byte floor of the criterion: both maps read once, 8 bytes per element pair, at
the 6.3 TB/s the kernel guide gives for element-wise streams on the MI355X (its HBM3E peak is 8 TB/s).

    python tools/featmetric_time.py [--iters N] [--window-ms T] [--rounds R] [--warmup W] [--label TEXT] [--append] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bbl_time import peak_bytes, window  # noqa: E402
from gan_time import device_ops  # noqa: E402

STREAM_BYTES_PER_S = 6.3e12
FLOOR_BYTES = 8
SHAPES = ((1, 3, 2040, 1356), (16, 3, 256, 256))


def record(lines, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def compare(paths, min_iters, window_ms, rounds, warmup):
    """paths: [(name, fn)].  Alternating windows of about window_ms each; {name: (median, min, max, peak bytes, calls
    per window)}."""
    peaks = {name: peak_bytes(fn) for name, fn in paths}
    iters = {}
    for name, fn in paths:
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(min_iters, min(2000, math.ceil(window_ms / window(fn, min_iters))))
    times = {name: [] for name, _ in paths}
    for _ in range(rounds):
        for name, fn in paths:
            times[name].append(window(fn, iters[name]))
    return {name: (statistics.median(t), min(t), max(t), peaks[name], iters[name]) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="the fewest calls in a window")
    ap.add_argument("--window-ms", type=float, default=50.0, help="device time a window is filled to")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "featmetric_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("featmetric_time.py needs the MI355X")
    import featmetric_cases as cases
    from ssl_amd import _lib, metrics_feat as MF
    from ssl_amd.engine import address_array
    from ssl_amd.losses import set_native_criteria
    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    record(lines, unit=L.ssg_featmetric_unit(), chunk=L.ssg_featmetric_chunk(), grid_cap=L.ssg_featmetric_grid_cap(),
           device=torch.cuda.get_device_name(0))
    nets = {"lpips_alex": MF.LPIPS("alex", cases.lpips_state("alex")[0]).to(dev),
            "lpips_vgg": MF.LPIPS("vgg", cases.lpips_state("vgg")[0]).to(dev),
            "dists": MF.DISTS(cases.dists_state()[0]).to(dev)}
    for shape in SHAPES:
        sr, gt = (t.to(dev) for t in cases.images(shape))
        for name, net in nets.items():
            is_lpips = name.startswith("lpips")
            with torch.no_grad():
                f0, f1 = (net.features(sr * 2 - 1), net.features(gt * 2 - 1)) if is_lpips else (net.features(gt), net.features(sr))
            f0, f1 = [t.contiguous() for t in f0], [t.contiguous() for t in f1]
            K, N = len(f0), shape[0]
            n_el = sum(t.numel() for t in f0)
            C, H, W = (np.ascontiguousarray([t.shape[i] for t in f0], dtype=np.int32) for i in (1, 2, 3))
            a0, a1 = (address_array([t.data_ptr() for t in ts]) for ts in (f0, f1))
            if is_lpips:
                lins = [p.detach() for p in net.lins]
                aw = address_array([t.data_ptr() for t in lins])
                nb = L.ssg_lpips_workspace_bytes(K, N, C.ctypes.data, H.ctypes.data, W.ctypes.data)
                out = torch.empty((N, K + 1), dtype=torch.float64, device=dev)
            else:
                alpha, beta = net.alpha.detach(), net.beta.detach()
                nb = L.ssg_dists_workspace_bytes(K, N, C.ctypes.data, H.ctypes.data, W.ctypes.data)
                out = torch.empty((N, 3), dtype=torch.float64, device=dev)
            work = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)

            def c_call():
                if is_lpips:
                    _lib.check(L.ssg_lpips_layers(K, N, a0.ctypes.data, a1.ctypes.data, aw.ctypes.data, C.ctypes.data,
                                                  H.ctypes.data, W.ctypes.data, work.data_ptr(), nb, out.data_ptr(), stream))
                else:
                    _lib.check(L.ssg_dists_score(K, N, a0.ctypes.data, a1.ctypes.data, C.ctypes.data, H.ctypes.data,
                                                 W.ctypes.data, alpha.data_ptr(), beta.data_ptr(), work.data_ptr(), nb,
                                                 out.data_ptr(), stream))

            def torch_lines():
                with torch.no_grad():
                    return MF.lpips_torch_lines(f0, f1, lins) if is_lpips else MF.dists_torch_lines(f0, f1, alpha, beta)

            def module():
                with torch.no_grad():
                    return net(sr, gt, normalize=True) if is_lpips else net(gt, sr)

            def module_torch():
                prev = set_native_criteria(False)
                try:
                    return module()
                finally:
                    set_native_criteria(prev)

            paths = [("c_call", c_call), ("torch_lines", torch_lines), ("module", module), ("module_torch", module_torch)]
            res = compare(paths, args.iters, args.window_ms, args.rounds, args.warmup)
            ops = {p: device_ops(fn) for p, fn in paths}
            floor_ms = FLOOR_BYTES * n_el / STREAM_BYTES_PER_S * 1e3
            native, lines_value = module().reshape(-1).double(), module_torch().reshape(-1).double()
            record(lines, net=name, shape=list(shape), layers=[list(t.shape[1:]) for t in f0], element_pairs=n_el,
                   workspace_bytes=nb, byte_floor_ms=round(floor_ms, 4),
                   value_native=float(native[0]), value_torch_lines=float(lines_value[0]),
                   max_abs_diff=float((native - lines_value).abs().max()))
            for p, (med, lo, hi, peak, calls) in res.items():
                rec = dict(net=name, shape=list(shape), path=p, ms_median=round(med, 4), ms_min=round(lo, 4),
                           ms_max=round(hi, 4), windows=args.rounds, iters=calls, device_ops=ops[p],
                           peak_MB=round(peak / 2 ** 20, 2))
                if p in ("c_call", "torch_lines"):
                    rec.update(floor_share=round(floor_ms / med, 4), achieved_TBps=round(FLOOR_BYTES * n_el / (med * 1e-3) / 1e12, 3))
                if p == "c_call":
                    rec.update(torch_lines_over_this=round(res["torch_lines"][0] / med, 2),
                               share_of_module=round(med / res["module"][0], 4))
                if p == "torch_lines":
                    rec.update(share_of_module_torch=round(med / res["module_torch"][0], 4))
                if p == "module":
                    rec.update(module_torch_over_this=round(res["module_torch"][0] / med, 3))
                record(lines, **rec)
            del f0, f1, work
            torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        if not args.append:
            f.write("# tools/featmetric_time.py: the LPIPS and DISTS criteria per call on the MI355X -- the bare launches, the "
                    "packages' torch lines on the same features, and the whole metric call with its network either way; "
                    "byte floor: 8 bytes per element pair at 6.3 TB/s\n")
        f.write(f"# run {args.label}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
