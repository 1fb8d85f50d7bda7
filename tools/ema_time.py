#!/usr/bin/env python3
"""The EMA of a generator's weights timed, per call: the reference's per-tensor loop beside the one-launch multi-tensor
update (ssl_amd.ema.ModelEma -> ssg_multi_apply), on the same GPU in the same run.

Paths, model_ema's form e <- e * decay + (1 - decay) * p with decay 0.999:
    loop        (a) the reference's loop: e.mul_(decay).add_(p, alpha=1 - decay) per parameter (base_model.py:75-82)
    foreach     (b) torch._foreach_mul_(es, decay); torch._foreach_add_(es, ps, alpha=1 - decay): the alternative that
                    needs no kernel of this library
    native      (c) ModelEma.update: the per-call pointer check and one ssg_multi_apply
    c_call      (d) the bare ssg_multi_apply on the prebuilt table
and for LitEma, on a second set: `lit_loop` (the reference's forward restated: Python min on device scalars, then
shadow.sub_(w * (shadow - p)) per parameter) beside `lit_native` (ssl_amd.ema.LitEma.forward).
Sets: RRDBNet's parameter shapes (num_feat 64, num_block 23, num_grow_ch 32: 702 tensors), written out below, and a few
hundred tensors of mixed size for LitEma.  A warm-up, then `--rounds` alternating windows of `--iters` calls each, device
events around a window; the median window and the min / max.  `ms_*` is the time per call of a window of back-to-back
calls, so the larger of the host's and the device's time; `device_ops` and `device_busy_us` are the device activities
torch's profiler records for one call and the sum of their durations (null if the profiler is not available).  The byte floor: two reads and one store, 12 bytes per
element, at the 6.3 TB/s the kernel guide gives for element-wise streams on the MI355X (its HBM3E peak is 8 TB/s); the
RRDBNet set's 134 MB of weights can sit in the 256 MB Infinity Cache, so a share above 1 is not an error.
`pointer_check_ms` is the host time of ModelEma's per-call validation alone (time.perf_counter, no device work).
`--sweep` times (d) on the profiling build for a few chunk sizes and grid caps (ssg_prof_multi_tuning): the A/B behind
ssg_multi_chunk() and ssg_multi_grid_cap().

    python tools/ema_time.py [--iters N] [--rounds R] [--warmup W] [--sweep] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from bbl_time import compare, window  # noqa: E402
from gan_time import device_ops  # noqa: E402

STREAM_BYTES_PER_S = 6.3e12   # element-wise streams on the MI355X (HBM3E peak: 8 TB/s)
SWEEP = ((1024, 1024), (2048, 1024), (4096, 1024), (8192, 1024), (16384, 1024), (4096, 512), (4096, 2048), (4096, 4096))


def rrdbnet_shapes(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32):
    """The parameter shapes of RRDBNet in named_parameters() order (weight, bias per convolution)."""
    conv = lambda o, i: [(o, i, 3, 3), (o,)]  # noqa: E731
    shapes = conv(num_feat, num_in_ch)
    for _ in range(num_block * 3):                      # three residual dense blocks per RRDB, five convolutions each
        for k in range(4):
            shapes += conv(num_grow_ch, num_feat + k * num_grow_ch)
        shapes += conv(num_feat, num_feat + 4 * num_grow_ch)
    for _ in range(4):                                  # conv_body, conv_up1, conv_up2, conv_hr
        shapes += conv(num_feat, num_feat)
    return shapes + conv(num_out_ch, num_feat)


def mixed_shapes(n=300):
    gen = torch.Generator().manual_seed(3)
    sizes = torch.randint(1, 65, (n,), generator=gen).tolist()
    return [(s,) if i % 3 else (s, 1 + s % 9, 3, 3) for i, s in enumerate(sizes)]


def module_of(shapes, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    m = nn.Module()
    for i, s in enumerate(shapes):
        m.register_parameter(f"p{i}", nn.Parameter((torch.randn(s, generator=gen) * 0.05).to(dev)))
    return m


def device_busy_us(fn):
    """The sum of the durations of the device activities of one call (null if the profiler is not available)."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return round(sum(e.time_range.elapsed_us() for e in prof.events() if e.device_type == DeviceType.CUDA), 1)
    except Exception:       # noqa: BLE001 -- reported as null, the timings stand
        return None


def record(lines, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_time.py needs the MI355X")
    from ssl_amd import _lib, ema
    dev = torch.device("cuda:0")
    L = _lib.lib()
    decay = 0.999
    lines = []
    shapes = rrdbnet_shapes()
    net, avg = module_of(shapes, dev, 1), module_of(shapes, dev, 2)
    ps, es = [p.data for p in net.parameters()], [p.data for p in avg.parameters()]
    n_el = sum(p.numel() for p in ps)
    record(lines, set="rrdbnet", tensors=len(ps), elements=n_el, chunk=L.ssg_multi_chunk(), grid_cap=L.ssg_multi_grid_cap())
    m = ema.ModelEma(net, avg)
    m.update(decay)
    table, n_chunks = m._ema._tables[0][1], m._ema._tables[0][2]
    stream = torch.cuda.current_stream().cuda_stream
    d, a = float(decay), 1 - float(decay)

    def loop():
        for e, p in zip(es, ps):
            e.mul_(decay).add_(p, alpha=1 - decay)

    def foreach():
        torch._foreach_mul_(es, decay)
        torch._foreach_add_(es, ps, alpha=1 - decay)

    def native():
        m.update(decay)

    def c_call():
        _lib.check(L.ssg_multi_apply(table.data_ptr(), n_chunks, ema.EMA, d, a, None, stream))

    paths = [("loop", loop), ("foreach", foreach), ("native", native), ("c_call", c_call)]
    res = compare(paths, args.iters, args.rounds, args.warmup)
    ops = {name: device_ops(fn) for name, fn in paths}
    busy = {name: device_busy_us(fn) for name, fn in paths}
    floor_ms = 12 * n_el / STREAM_BYTES_PER_S * 1e3
    for name, (med, lo, hi, peak) in res.items():
        rec = dict(set="rrdbnet", path=name, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                   windows=args.rounds, iters=args.iters, device_ops=ops[name], device_busy_us=busy[name],
                   peak_MB=round(peak / 2 ** 20, 2))
        if name == "c_call":
            rec.update(byte_floor_ms=round(floor_ms, 5), floor_share=round(floor_ms / med, 4), peak_used_TBps=6.3,
                       achieved_TBps=round(12 * n_el / (med * 1e-3) / 1e12, 3))
        if name != "native":
            rec.update(over_native=round(med / res["native"][0], 2))
        record(lines, **rec)
    # (d) again on the same set with every src ONE FLOAT past dst's alignment: dst is still stored 16 bytes wide, src is
    # read element by element (the pairs of a view into a flat buffer)
    pos, offs = 0, []
    for p in ps:
        pos = -(-pos // 4) * 4 + 1
        offs.append(pos)
        pos += p.numel()
    buf = torch.randn(pos, device=dev) * 0.05
    t1, nc1, _host1 = ema.build_table([e.data_ptr() for e in es], [buf.data_ptr() + 4 * o for o in offs],
                                      [e.numel() for e in es], dev)

    def c_call_src_off1():
        _lib.check(L.ssg_multi_apply(t1.data_ptr(), nc1, ema.EMA, d, a, None, stream))

    res1 = compare([("c_call", c_call), ("c_call_src_off1", c_call_src_off1)], args.iters, args.rounds, args.warmup)
    for name, (med, lo, hi, _) in res1.items():
        record(lines, set="rrdbnet, src off by one float", path=name, ms_median=round(med, 4), ms_min=round(lo, 4),
               ms_max=round(hi, 4), windows=args.rounds, iters=args.iters, floor_share=round(floor_ms / med, 4))
    # the host time of the per-call validation alone
    flat = m.dst + m.src
    checks = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.iters):
            assert m._ema.signature(flat) == m._ema._sig
        checks.append((time.perf_counter() - t0) / args.iters * 1e3)
    record(lines, set="rrdbnet", pointer_check_ms=round(statistics.median(checks), 4), tensors_checked=len(flat))

    # an observation, not a requirement: torch's own GPU result for the reference's expression against the kernel's, from
    # the same start (whether torch's ROCm kernel contracts a + alpha * b into an fma decides it)
    start = [torch.randn(e.shape, device=dev) for e in es]
    results = []
    for fn in (native, loop, foreach):
        for e, s0 in zip(es, start):
            e.copy_(s0)
        fn()
        results.append(torch.cat([e.flatten().view(torch.int32) for e in es]))
    torch.cuda.synchronize()
    record(lines, observation="elements of torch's GPU result equal to the kernel's (same start, one update)", elements=n_el,
           loop_equal=int((results[1] == results[0]).sum()), foreach_equal=int((results[2] == results[0]).sum()))

    # LitEma on a few hundred tensors of mixed size
    lshapes = mixed_shapes()
    model = module_of(lshapes, dev, 4)
    lit = ema.LitEma(model).to(dev)
    names = [(n, n.replace(".", "")) for n, _ in model.named_parameters()]
    ref_decay = torch.tensor(0.9999, dtype=torch.float32, device=dev)
    ref_num = torch.tensor(0, dtype=torch.int, device=dev)
    ref_shadow = {s: p.detach().clone() for (n, s), p in zip(names, model.parameters())}

    def lit_loop():
        nonlocal ref_num
        ref_num += 1
        dec = min(ref_decay, (1 + ref_num) / (10 + ref_num))          # (a host read, as in the reference)
        w = 1.0 - dec
        with torch.no_grad():
            params = dict(model.named_parameters())
            for n, s in names:
                ref_shadow[s].sub_(w * (ref_shadow[s] - params[n]))

    def lit_native():
        lit(model)

    paths = [("lit_loop", lit_loop), ("lit_native", lit_native)]
    res = compare(paths, args.iters, args.rounds, args.warmup)
    ops = {name: device_ops(fn) for name, fn in paths}
    for name, (med, lo, hi, peak) in res.items():
        rec = dict(set="mixed", tensors=len(lshapes), elements=sum(p.numel() for p in model.parameters()), path=name,
                   ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), windows=args.rounds,
                   iters=args.iters, device_ops=ops[name])
        if name == "lit_loop":
            rec.update(over_native=round(med / res["lit_native"][0], 2))
        record(lines, **rec)

    if args.sweep:
        # (d) on the profiling build per candidate: a table filled under the candidate's chunk, launched under its cap
        P = _lib.lib_prof()
        P.ssg_prof_multi_tuning.restype, P.ssg_prof_multi_tuning.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
        cands = {}
        for chunk, cap in SWEEP:
            _lib.check(P.ssg_prof_multi_tuning(chunk, cap))
            with _lib.profile_build():
                t, nc, host = ema.build_table([e.data_ptr() for e in es], [p.data_ptr() for p in ps],
                                              [e.numel() for e in es], dev)
            cands[(chunk, cap)] = (t, nc, host)
        _lib.check(P.ssg_prof_multi_tuning(L.ssg_multi_chunk(), L.ssg_multi_grid_cap()))

        def runner(chunk, cap):
            t, nc, _ = cands[(chunk, cap)]

            def run():
                P.ssg_prof_multi_tuning(chunk, cap)
                _lib.check(P.ssg_multi_apply(t.data_ptr(), nc, ema.EMA, d, a, None, stream))
            return run

        paths = [(f"chunk{c}_cap{g}", runner(c, g)) for c, g in SWEEP]
        for _, fn in paths:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                times[name].append(window(fn, args.iters))
        for (c, g), (name, _) in zip(SWEEP, paths):
            t = times[name]
            record(lines, sweep="c_call", chunk=c, grid_cap=g, chunks=cands[(c, g)][1], ms_median=round(statistics.median(t), 4),
                   ms_min=round(min(t), 4), ms_max=round(max(t), 4), floor_share=round(floor_ms / statistics.median(t), 4))
        P.ssg_prof_multi_tuning(L.ssg_multi_chunk(), L.ssg_multi_grid_cap())

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/ema_time.py: the EMA of a parameter set per call on the MI355X: the reference's per-tensor loop, "
                "torch._foreach_*, ModelEma.update and the bare ssg_multi_apply (RRDBNet's 702 shapes); LitEma's loop and "
                "the native forward (300 mixed tensors); the per-call pointer check's host time; with --sweep the chunk / "
                "grid-cap candidates on the profiling build.  byte floor: 12 bytes per element at 6.3 TB/s\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
