#!/usr/bin/env python
"""Times the JPEG round trip (ssg_jpeg_roundtrip, ssl_amd/csrc/ssg_jpegcodec.hip) against the bytes a call must move:

    python tools/jpeg_codec_time.py [--reps 11] [--calls 50] [--ab] [--parity]

  16 x 3 x 72 x 72 (BSRGAN's LQ patch), 16 x 3 x 256 x 256 and 1 x 3 x 2040 x 1356, bytes in and bytes out.
Per call: `calls` calls of the C ABI back to back between two device events (output and workspace allocated once),
divided by `calls`; the median (min) of `reps` such windows after a warm-up.  A call shorter than its issue on the host
(a few microseconds a launch) shows the host's time.  The floor is input bytes + output bytes at 6.29 TB/s: the kernel is bound by its integer
arithmetic (the VALU), not by HBM, and the figure says how far.  On the same machine: Pillow's encode + decode of the
same images on one CPU core (the codec the reference calls through cv2), and the existing `jpeg_kernel` behind
`datapath.DiffJPEG`, the float simulation, on the same shapes as floats (it computes something else; the row is there
for scale).

--ab runs these shapes, other batches of them and images of one tile on the profiling build under both values of its
SSG_JPEG_FUSED switch (1 = one launch with recomputed chroma halos, 0 = two launches through the workspace) and of its
SSG_JPEG_TM switch (tiles of 4 x 4 or 2 x 2 MCUs), alternating (profiles/jpeg_codec_tile_ab.txt).
--parity counts the bytes that differ from Pillow over the case sets of tests/jpeg_codec_cases.py
(profiles/jpeg_codec_parity.txt)."""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssl_amd import _lib, datapath  # noqa: E402

PEAK = 6.29e12
SHAPES = [(16, 72, 72), (16, 256, 256), (1, 2040, 1356)]
AB_SHAPES = SHAPES + [(64, 72, 72), (256, 72, 72), (4, 256, 256), (64, 256, 256), (4, 2040, 1356), (16, 128, 128),
                      (128, 128, 128), (16, 64, 64), (256, 64, 64), (16, 32, 32), (256, 32, 32), (1, 72, 72)]


def windows(fn, reps, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(us), min(us)


def images(shape, dev):
    B, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    q = [int(v) for v in torch.randint(30, 96, (B,), generator=g)]
    return x.to(dev), q


def codec_call(x, q):
    """the C call alone: output, workspace and qualities made once (re-made when the profiling build's switches move
    the call to the other path); returns (call, output)"""
    B, H, W, _ = x.shape
    L = _lib.lib()
    qs = np.ascontiguousarray(q, dtype=np.int32)
    out = torch.empty_like(x)
    nbytes = L.ssg_jpeg_roundtrip_workspace_bytes(B, H, W, 3)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    st = torch.cuda.current_stream().cuda_stream
    args = (x.data_ptr(), out.data_ptr(), B, H, W, 3, qs.ctypes.data, 0, 0, ws.data_ptr(), nbytes, st)

    def call(keep=(qs, ws)):
        _lib.check(L.ssg_jpeg_roundtrip(*args))
    return call, out


def path_of(shape):
    return "two launches" if _lib.lib().ssg_jpeg_roundtrip_workspace_bytes(shape[0], shape[1], shape[2], 3) else "one launch"


def run(reps, calls):
    from PIL import Image
    dev = torch.device("cuda:0")
    print(f"{torch.cuda.get_device_name(0)}; per call over windows of {calls} launches, median (min) of {reps} windows")
    for shape in SHAPES:
        x, q = images(shape, dev)
        med, best = windows(codec_call(x, q)[0], reps, calls)
        wrapped = windows(lambda: datapath.jpeg_roundtrip(x, q), reps, calls)[0]
        moved = 2 * x.numel()
        floor_us = moved / PEAK * 1e6
        print(f"ssg_jpeg_roundtrip {shape[0]:3d} x 3 x {shape[1]} x {shape[2]:<5d} {path_of(shape):12s} {med:9.1f} us ({best:.1f})  "
              f"{moved / 1e6:6.2f} MB in + out, floor {floor_us:5.2f} us (HBM; the kernel is VALU-bound), "
              f"{med / floor_us:6.1f} x the floor")
        print(f"  datapath.jpeg_roundtrip (allocates the output and the workspace, checks the qualities) {wrapped:9.1f} us")
        f = (x.permute(0, 3, 1, 2).float() / 255).contiguous()
        qd = torch.tensor(q, dtype=torch.float32, device=dev)
        m = datapath.DiffJPEG(differentiable=False)
        med, best = windows(lambda: m(f, qd), reps, calls)
        print(f"  DiffJPEG (float simulation), same shape as floats {med:9.1f} us ({best:.1f})")
        host = x.cpu().numpy()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            for b in range(shape[0]):
                buf = io.BytesIO()
                Image.fromarray(host[b]).save(buf, format="JPEG", quality=q[b])
                np.asarray(Image.open(io.BytesIO(buf.getvalue())))
            t.append(time.perf_counter() - t0)
        print(f"  Pillow encode + decode, one CPU core of the same machine {min(t) * 1e6:9.1f} us (best of 3)")


def ab(reps, calls):
    dev = torch.device("cuda:0")
    print(f"{torch.cuda.get_device_name(0)}; profiling build, per call over windows of {calls} launches, "
          f"median of {reps} windows, the configurations alternating window by window")
    print("tile: MCUs a side (4 = 64 x 64 pixels, 2 = 32 x 32); 1L = one launch with recomputed chroma halos, "
          "2L = two launches through the workspace")
    configs = [(tm, fused) for tm in ("4", "2") for fused in ("1", "0")]

    def select(cfg):
        os.environ["SSG_JPEG_TM"], os.environ["SSG_JPEG_FUSED"] = cfg

    with _lib.profile_build():
        for shape in AB_SHAPES:
            x, q = images(shape, dev)
            B, H, W, _ = x.shape
            fns, outs, us = {}, [], {c: [] for c in configs}
            for cfg in configs:
                select(cfg)
                fns[cfg], out = codec_call(x, q)
                windows(fns[cfg], 1, calls)
                outs.append(out)
            assert all(torch.equal(o, outs[0]) for o in outs)
            for _ in range(reps):
                for cfg in configs:
                    select(cfg)
                    us[cfg].append(windows(fns[cfg], 1, calls)[0])
            row = "  ".join(f"tile {tm} {'1L' if fused == '1' else '2L'} {statistics.median(us[(tm, fused)]):7.1f} us"
                            for tm, fused in configs)
            print(f"{B:4d} x 3 x {H} x {W:<5d} {row}")
        os.environ.pop("SSG_JPEG_FUSED", None)
        os.environ.pop("SSG_JPEG_TM", None)


def parity():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_codec_cases as K
    dev = torch.device("cuda:0")
    print(f"{torch.cuda.get_device_name(0)}; bytes that differ between datapath.jpeg_roundtrip and Pillow's "
          f"save(format='JPEG', quality=q) + open, per case set (tests/jpeg_codec_cases.py)")
    for name, sizes in (("SIZES", K.SIZES), ("SMALL_SIZES (a side below 8 or a width up to 4)", K.SMALL_SIZES),
                        ("two tiles an axis and more: 130 x 70, 65 x 65, 200 x 333", [(130, 70), (65, 65), (200, 333)])):
        n = bad = total = 0
        for (H, W) in sizes:
            for C in (1, 3):
                for q in K.QUALITIES:
                    for kind in K.CONTENTS:
                        a = K.content(kind, H, W, C, seed=7)
                        got = datapath.jpeg_roundtrip(torch.from_numpy(a).to(dev), q).cpu().numpy()
                        d = int((got != K.pillow_roundtrip(a, q)).sum())
                        n, bad, total = n + 1, bad + d, total + a.size
        print(f"{name}: {n} cases ({len(sizes)} sizes x L, RGB x qualities {K.QUALITIES} x {len(K.CONTENTS)} contents), "
              f"{total} bytes, {bad} differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--parity", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_codec_time.py times HIP kernels: no GPU visible")
    if args.ab:
        ab(args.reps, args.calls)
    elif args.parity:
        parity()
    else:
        run(args.reps, args.calls)


if __name__ == "__main__":
    main()
