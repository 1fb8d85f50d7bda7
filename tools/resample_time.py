#!/usr/bin/env python3
"""The Pillow-exact resize timed and compared (ssl_amd.prep.resize -> ssg_resample, one launch per call).

Timing: the four multiscale LANCZOS resizes of one 2040 x 1356 RGB image (0.75, 0.6, 1 / 3 and the 512-pixel shortest
edge: generate_multiscale_DF2K.py's set) and load_img at 787 x 531 -> 768 x 512 with the float epilogue.  A warm-up, then
`--rounds` windows of `--iters` back-to-back calls, device events around a window; the median window per call and the
min / max.  Two figures per workload: with the coefficient tables cached on the device (the launches alone), and with the
cache emptied before every call (the host's fp64 tables and their upload included).  Beside them Pillow's time for the
same resizes on this machine's CPU (median of `--rounds` runs), and the byte floor: input plus output bytes once over
HBM at the 6.29 TB/s a float4 copy reaches on the MI355X.

Parity (--parity FILE): a list of cases against Pillow itself on this machine, with the number of differing bytes each.

    python tools/resample_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE] [--parity FILE] [--trace]

--trace runs every timed call a few times and nothing else (for a kernel trace taken from outside)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy on the MI355X (8.0 TB/s on the datasheet)
SRC_W, SRC_H = 2040, 1356
LOAD_W, LOAD_H = 787, 531


def image(h, w, c, seed):
    """A smooth field with texture and a few hard edges, uint8 (h,w,c)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 120 + 70 * np.sin(x / 37.0) * np.cos(y / 23.0)
    a = base[..., None] + rng.normal(0, 12, (h, w, c)) + 60 * ((x // 64 + y // 48) % 2)[..., None]
    return np.clip(a, 0, 255).astype(np.uint8)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def timed(fn, iters, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = [window(fn, iters) for _ in range(rounds)]
    return statistics.median(t), min(t), max(t)


def cpu_timed(fn, rounds):
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def parity(path, dev):
    from PIL import Image
    from ssl_amd import prep
    cases = []
    src = image(SRC_H, SRC_W, 3, 1)
    for suffix, size in prep.multiscale_plan(SRC_W, SRC_H, 'dm', 512)[0]:
        cases.append((f"multiscale {suffix}", src, size, 'lanczos'))
    cases.append(("load_img", image(LOAD_H, LOAD_W, 3, 2), (LOAD_W - LOAD_W % 32, LOAD_H - LOAD_H % 32), 'lanczos'))
    small = image(211, 307, 3, 3)
    for f in prep.FILTERS:
        cases.append((f"{f} down", small, (100, 77), f))
        cases.append((f"{f} up", small, (500, 390), f))
    cases.append(("L 1/3", image(600, 900, 1, 4)[..., 0], (300, 200), 'lanczos'))
    cases.append(("8 : 1 both axes", image(800, 1200, 3, 5), (150, 100), 'lanczos'))
    cases.append(("8 : 1 rows, columns kept", image(800, 300, 3, 6), (300, 100), 'lanczos'))
    cases.append(("blocks of 0 / 255", np.kron(np.random.default_rng(7).integers(0, 2, (90, 130, 3), dtype=np.uint8) * 255,
                                               np.ones((4, 4, 1), np.uint8)), (390, 270), 'lanczos'))
    lines, total = [], 0
    for what, a, size, f in cases:
        want = np.array(Image.fromarray(a).resize(size, resample=prep.FILTERS[f]))
        got = prep.resize(torch.from_numpy(a).to(dev), size, f).cpu().numpy()
        diff = int((got != want).sum()) if got.shape == want.shape else -1
        total += diff != 0
        lines.append(json.dumps(dict(case=what, filter=f, in_hw=list(a.shape[:2]), out_wh=list(size),
                                     channels=1 if a.ndim == 2 else a.shape[2], bytes=int(want.size),
                                     differing_bytes=diff)))
        print(lines[-1], flush=True)
    import PIL
    with open(path, "w") as fh:
        fh.write(f"# tools/resample_time.py --parity: ssl_amd.prep.resize on the MI355X against Pillow {PIL.__version__} "
                 f"on the same machine; cases with differing bytes: {total}\n" + "\n".join(lines) + "\n")
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.txt"))
    ap.add_argument("--parity")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_time.py needs the MI355X")
    from PIL import Image
    from ssl_amd import prep
    dev = torch.device("cuda:0")
    if args.parity:
        os.makedirs(os.path.dirname(os.path.abspath(args.parity)), exist_ok=True)
        if parity(args.parity, dev):
            raise SystemExit("resample_time.py: the kernel and Pillow differ")

    src = image(SRC_H, SRC_W, 3, 1)
    small = image(LOAD_H, LOAD_W, 3, 2)
    x, s = torch.from_numpy(src).to(dev), torch.from_numpy(small).to(dev)
    sizes = [size for _, size in prep.multiscale_plan(SRC_W, SRC_H, 'dm', 512)[0]]
    lsize = (LOAD_W - LOAD_W % 32, LOAD_H - LOAD_H % 32)
    pil_src, pil_small = Image.fromarray(src), Image.fromarray(small)

    def pil_load():
        a = np.array(pil_small.resize(lsize, resample=Image.LANCZOS)).astype(np.float32) / 255.0
        return 2. * torch.from_numpy(a[None].transpose(0, 3, 1, 2)) - 1.

    work = [
        ("four multiscale resizes of 3 x 2040 x 1356", lambda: [prep.resize(x, size) for size in sizes],
         lambda: [pil_src.resize(size, resample=Image.LANCZOS) for size in sizes],
         sum(src.size + size[0] * size[1] * 3 for size in sizes)),
        ("load_img 1 x 3 x 531 x 787 -> 512 x 768, float epilogue", lambda: prep.resize(s, lsize, out='signed'), pil_load,
         small.size + lsize[0] * lsize[1] * 3 * 4),
    ]
    if args.trace:
        for _, fn, _, _ in work:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return

    def uncached(fn):
        def run():
            prep._tables.clear()
            return fn()
        return run

    lines = []
    for what, fn, pil_fn, nbytes in work:
        cached = timed(fn, args.iters, args.rounds, args.warmup)
        upload = timed(uncached(fn), max(args.iters // 5, 1), args.rounds, 1)
        cpu = cpu_timed(pil_fn, args.rounds)
        rec = dict(what=what, ms_tables_cached=round(cached[0], 4), ms_tables_cached_min_max=[round(v, 4) for v in cached[1:]],
                   ms_with_table_build_and_upload=round(upload[0], 4),
                   ms_with_table_build_and_upload_min_max=[round(v, 4) for v in upload[1:]],
                   pillow_cpu_ms=round(cpu[0], 2), pillow_cpu_ms_min_max=[round(v, 2) for v in cpu[1:]],
                   pillow_over_gpu_cached=round(cpu[0] / cached[0], 1), io_bytes=int(nbytes),
                   byte_floor_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 5),
                   share_of_byte_floor=round(nbytes / HBM_BYTES_PER_S * 1e3 / cached[0], 4),
                   windows=args.rounds, iters=args.iters)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import PIL
    with open(args.out, "w") as fh:
        fh.write("# tools/resample_time.py: ssl_amd.prep.resize per workload on the MI355X (device events around windows of "
                 "back-to-back calls: launches included), Pillow " + PIL.__version__ + " on the same machine's CPU, and "
                 "the byte floor (input + output once at 6.29 TB/s)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
