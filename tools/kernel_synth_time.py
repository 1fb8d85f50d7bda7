"""Time of datapath.synth_kernels for one training batch's kernels: B = 16 samples, 48 records of mixed kinds, padded
to 9 x 9 (this fork's dataset) and to 21 x 21 (stock Real-ESRGAN), beside the time the reference's CPU code took for the
same 16 samples when fixture F23 was generated (tests/golden/make_golden_kernels.py stores it).  Recorded, not gated.

    python tools/kernel_synth_time.py            (on the GPU box; writes profiles/kernel_synth_time.txt)

Two numbers per padded size, each the median of 7 windows of 2,000 calls after a warm-up window, with the windows'
range: the whole call as a user pays for it (records packed on the host, one host-to-device copy, one launch, ended by
a device synchronise; host clock) and the device side alone (events around the window; it contains the copy and the
launch gaps, not only the kernel)."""
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssl_amd import datapath  # noqa: E402

B, CALLS, WINDOWS = 16, 2000, 7


def records(opt, pad, seed):
    random.seed(seed)
    np.random.seed(seed)
    recs = [datapath.draw_kernels(opt, pad_to=pad) for _ in range(B)]
    return [r[j] for j in range(3) for r in recs]


def window(recs, pad, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(CALLS):
        datapath.synth_kernels(recs, pad, dev)
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e6, a.elapsed_time(b) / CALLS * 1e3      # microseconds per call


def main():
    assert torch.cuda.is_available(), "kernel_synth_time needs the MI355X (a CPU run says nothing about it)"
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(ROOT, "tests", "golden", "f23_blur_kernels.npz"))
    lines = [f"datapath.synth_kernels, B = {B} samples = {3 * B} records per call, {torch.cuda.get_device_name(0)}",
             f"median of {WINDOWS} windows of {CALLS} calls [min .. max], microseconds per call"]
    for tag in ("all", "wide"):
        opt = eval(str(g[f"b_{tag}_opt"][0]), {"__builtins__": {}}, {})
        pad = int(g[f"b_{tag}_pad"])
        recs = records(opt, pad, int(g[f"b_{tag}_seed"]))
        kinds = sorted({r.kind for r in recs})
        window(recs, pad, dev)                                   # warm-up: code object, allocator
        runs = [window(recs, pad, dev) for _ in range(WINDOWS)]
        host, devt = [r[0] for r in runs], [r[1] for r in runs]
        cpu = float(g[f"b_{tag}_cpu_seconds"]) * 1e6
        lines.append(f"pad_to {pad:2d} (options '{tag}', kinds {kinds}):")
        lines.append(f"    whole call, host clock to synchronise : {statistics.median(host):8.1f}  [{min(host):.1f} .. {max(host):.1f}]")
        lines.append(f"    device events around the window       : {statistics.median(devt):8.1f}  [{min(devt):.1f} .. {max(devt):.1f}]")
        lines.append(f"    reference on the CPU, same 16 samples : {cpu:8.1f}  (one run in the build container when the "
                     f"fixture was made; per dataloader worker)")
    lines.append("(where the two clocks agree, the host's issue of the calls -- packing the records, the copy, the launch -- is the "
                 "bound and the device keeps up with it)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "kernel_synth_time.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
