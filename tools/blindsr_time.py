#!/usr/bin/env python3
"""BSRGAN's degradation chain per call of `BlindSRDegradation.feed` at the training file's values -- batch 48,
lq_patchsize 72, sf 4, H inputs of H_size x H_size as data/dataset_blindsr.py crops them (288 = lq_patchsize sf unless
--h-size says otherwise) -- in two forms on the same GPU, on the SAME programs (the decisions are drawn once, seeded):

    ragged     feed(images): slot by slot, one launch per operation family present in a slot
    per_image  the same chain issued image by image through the single-image path (a feed of one image each)

with the ragged launch counts of both and the device activities of one call of each (torch's profiler), then every kernel
family alone on a batch of 48 H-sized images (the 9 x 9 convolution, the three resizes by 1/2 and by 0.53, colour Gaussian
noise), its device time between events against the byte floor of its input plus output (plus field) at 8 TB/s.  Host
clock around calls that end in a device synchronise; a warm-up, then the median of `--rounds` windows of `--iters` calls.
The reference's own CPU time is not taken here (OpenCV is not installed where this runs): no ratio to it is quoted.

With --parity the tool writes profiles/blindsr_parity.txt instead: the share of each derived bound the live float32
oracles use (tests/blindsr_cases.py) and, on the GPU, the shares the kernels use (the GPU tests' own cases).

    python tools/blindsr_time.py [--iters N] [--rounds R] [--warmup W] [--h-size S] [--parity] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gan_time import HBM_BYTES_PER_S, device_ops  # noqa: E402

BATCH, PATCH, SF = 48, 72, 4


def windows(fn, iters, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(out), min(out), max(out)


def event_ms(fn, iters, rounds, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)


def parity(out):
    import blindsr_cases as cases
    import blindsr_reference as R
    lines = ["# The ragged degradation kernels (ssl_amd/csrc/ssg_blindsr.hip) and their restatement tests/blindsr_reference.py:",
             "# the largest share of the derived first-order bound that each comparison uses (every element is held to it).",
             "# Live float32 oracles (CPU, tests/test_cpu_blindsr.py::test_every_float32_oracle_meets_the_derived_bound):"]
    for name, share in cases.oracle_shares().items():
        lines.append(f"{name}: {share:.3e}")
    if torch.cuda.is_available():
        import test_gpu_blindsr as tg
        dev = torch.device("cuda:0")
        lines.append("# The kernels on the MI355X against the restatement (the cases of tests/test_gpu_blindsr.py); the noise")
        lines.append("# stages are held bit for bit and have no share:")
        for k in cases.CONV_KS:
            images, stages = cases.conv_cases(k)
            got = tg._apply(dev, "conv", images, stages)
            share = max(tg._within(y, *R.conv(x, s.params["kernel"], s.params["stride"], s.params["clip"]), k)
                        for x, s, y in zip(images, stages, got))
            lines.append(f"ssg_blindsr_conv k={k} ({len(images)} images): {share:.3e}")
        for interp, name in ((R.LINEAR, "LINEAR"), (R.CUBIC, "CUBIC"), (R.AREA, "AREA")):
            images, stages = cases.resize_cases(interp)
            got = tg._apply(dev, "resize", images, stages)
            share = max(tg._within(y, *R.resize(x, s.oh, s.ow, interp, s.params["clip"]), name)
                        for x, s, y in zip(images, stages, got))
            lines.append(f"ssg_blindsr_resize {name} ({len(images)} images): {share:.3e}")
    else:
        lines.append("# The kernels' shares: not yet measured (no MI355X run of this tool)")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--h-size", type=int, default=PATCH * SF)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parity:
        return parity(args.out or os.path.join(ROOT, "profiles", "blindsr_parity.txt"))
    if not torch.cuda.is_available():
        raise SystemExit("blindsr_time.py needs the MI355X")
    import blindsr_cases as cases
    from ssl_amd import blindsr
    dev = torch.device("cuda:0")
    S = args.h_size
    gen = torch.Generator().manual_seed(35)
    images = [torch.rand(S, S, 3, generator=gen).to(dev) for _ in range(BATCH)]
    lines = [f"# BlindSRDegradation.feed, batch {BATCH}, lq_patchsize {PATCH}, sf {SF}, H inputs {S} x {S} x 3 on the GPU; "
             f"median (min .. max) of {args.rounds} windows of {args.iters} calls, host clock to a device synchronise"]
    for variant in ("bsrgan", "plus"):
        # the decisions from seeded generators, once; the noise fields of every call from the GPU's generator
        planner = blindsr.BlindSRDegradation(sf=SF, lq_patchsize=PATCH, variant=variant, draws=cases.seeded_draws(35))
        progs = planner.draw_programs([(S, S, 3)] * BATCH)
        deg = blindsr.BlindSRDegradation(sf=SF, lq_patchsize=PATCH, variant=variant)
        stages = sum(len(p.stages) for p in progs)
        ragged = lambda: deg.feed(images, programs=progs)
        one = blindsr.BlindSRDegradation(sf=SF, lq_patchsize=PATCH, variant=variant)
        count = [0]

        def per_image():
            count[0] = 0
            for x, p in zip(images, progs):
                one.feed([x], programs=[p])
                count[0] += one.launches
        ragged()
        per_image()
        lines.append(f"{variant}: {stages} stages in the batch's programs")
        for name, fn, launches in (("ragged", ragged, lambda: deg.launches), ("per_image", per_image, lambda: count[0])):
            med, lo, hi = windows(fn, args.iters, args.rounds, args.warmup)
            lines.append(f"  {name:9s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})   ragged-kernel launches {launches()}   "
                         f"device activities of one call {device_ops(fn)}")
    lines.append(f"# every family alone, {BATCH} images of 3 x {S} x {S}, device events, against its byte floor at 8 TB/s")
    planar = [x.permute(2, 0, 1).contiguous() for x in images]
    n_in = BATCH * 3 * S * S
    rng = np.random.default_rng(1)
    kern = cases.asymmetric_kernel(rng, 9)
    jobs = [("conv 9x9", blindsr.CONV, [blindsr.Stage("conv", S, S, S, S, dict(kernel=kern, stride=1, clip=True))] * BATCH, None)]
    for name, interp in (("LINEAR", 1), ("CUBIC", 2), ("AREA", 3)):
        for r in (0.5, 0.53):
            o = int(r * S)
            jobs.append((f"resize {name} x{r}", blindsr.RESIZE,
                         [blindsr.Stage("resize", S, S, o, o, dict(interp=interp, clip=True))] * BATCH, None))
    field = [torch.randn(3, S, S, device=dev) for _ in range(BATCH)]
    jobs.append(("noise GAUSS_COLOR", blindsr.NOISE,
                 [blindsr.Stage("noise", S, S, S, S, dict(op="GAUSS_COLOR", scale=0.04, matrix=None, clip=True, lead_clip=False))] * BATCH,
                 field))
    for name, fam, stages, fields in jobs:
        # the bare launch on prebuilt buffers: what ragged_apply does, without its concatenations
        pool, recs = blindsr._Pool(), np.zeros(BATCH, dtype=blindsr._REC)
        n_out = 0
        for i, st in enumerate(stages):
            blindsr._set_stage(recs[i], st, 3, pool)
            recs[i]["in_off"], recs[i]["out_off"], recs[i]["field_off"] = i * 3 * S * S, n_out, i * 3 * S * S
            n_out += 3 * st.oh * st.ow
        ph = pool.array()
        table, n_tiles = blindsr.fill_table(fam, recs, n_in, n_out, n_in if fields else 0, ph.size)
        blob = torch.from_numpy(np.concatenate([table, ph.view(np.uint8)])).to(dev)
        src, dst = torch.cat([x.reshape(-1) for x in planar]), torch.empty(n_out, device=dev)
        fld = torch.cat([f.reshape(-1) for f in fields]) if fields else None
        call = lambda: blindsr._launch_family(dev, fam, blob.data_ptr(), n_tiles, src.data_ptr(), dst.data_ptr(),
                                              None if fld is None else fld.data_ptr(), blob.data_ptr() + table.size)
        ms = event_ms(call, 20, args.rounds, 3)
        floor = 4 * (n_in + n_out + (n_in if fields else 0)) / HBM_BYTES_PER_S * 1e3
        lines.append(f"  {name:22s} {ms * 1e3:8.1f} us   floor {floor * 1e3:6.1f} us   {100 * floor / ms:5.1f} % of the floor's rate")
    out = args.out or os.path.join(ROOT, "profiles", "blindsr_time.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
