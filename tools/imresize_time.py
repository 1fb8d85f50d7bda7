#!/usr/bin/env python
"""Times ssl_amd.prep.imresize (ssg_imresize.hip) with the tables cached, against the bytes each call must move:

    python tools/imresize_time.py [--reps 20] [--lds-pref BYTES ...]

  1 / 4 of one 3 x 2040 x 1356 byte image, x 4 of the result, 1 / 4 of 16 x 3 x 256 x 256 floats.
Per call: the median of `reps` event-timed launches after a warm-up, and the floor input bytes + output bytes at
6.29 TB/s (the kernel reads each input pixel more than once across tiles, so the floor is not its traffic).  The
reference's own seconds for the same inputs on a CPU are in tests/golden/imresize_cpu_timing.json; the two machines are
not compared.

--lds-pref runs the same three calls on the profiling build once per value of its SSG_IMRESIZE_LDS_PREF switch: the
kernel takes the first tile of its list whose LDS is at most that many bytes (the product build's constant is 49152),
else the tile with the least LDS.  The tile A/B of profiles/imresize_tile_ab.txt."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssl_amd import _lib, prep  # noqa: E402

PEAK = 6.29e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return y, statistics.median(ms), min(ms)


def tile_at(s):
    import ctypes
    buf, chosen = (ctypes.c_int * 16)(), ctypes.c_int(-1)
    _lib.lib().ssg_imresize_tiles(s, 1, buf, 8, ctypes.byref(chosen))
    return f"{buf[2 * chosen.value]} x {buf[2 * chosen.value + 1]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lds-pref", type=int, nargs="*", default=[])
    args = ap.parse_args()
    if args.lds_pref:
        for pref in args.lds_pref:
            os.environ["SSG_IMRESIZE_LDS_PREF"] = str(pref)
            with _lib.profile_build():
                print(f"--- profiling build, LDS preference {pref} B")
                run(args.reps)
        return
    run(args.reps)


def run(reps):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)
    img = torch.randint(0, 256, (2040, 1356, 3), dtype=torch.uint8, generator=g).to(dev)
    batch = torch.rand((16, 3, 256, 256), generator=g).to(dev)
    print(f"{torch.cuda.get_device_name(0)}; median (min) of {reps} launches, tables cached")
    lr = None
    for what, x, s in (("1/4 of 2040 x 1356 x 3 bytes", img, 1 / 4), ("x4 of the result", None, 4),
                       ("1/4 of 16 x 3 x 256 x 256 floats", batch, 1 / 4)):
        x = lr if x is None else x
        y, med, best = timed(lambda: prep.imresize(x, s), reps)
        lr = y if lr is None else lr
        moved = x.numel() * x.element_size() + y.numel() * y.element_size()
        floor_us = moved / PEAK * 1e6
        print(f"{what:34s} {tuple(x.shape)} -> {tuple(y.shape)}  tile {tile_at(s):7s} {med * 1e3:9.1f} us ({best * 1e3:.1f})  "
              f"{moved / 1e6:7.2f} MB in + out, floor {floor_us:6.2f} us, {med * 1e3 / floor_us:6.1f} x the floor")


if __name__ == "__main__":
    main()
