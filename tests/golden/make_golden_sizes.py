"""Fixture F21: every size and offset the C ABI's host arithmetic reports, recorded from the built library.

    python tests/golden/make_golden_sizes.py        (writes tests/golden/f21_host_sizes.json)

Host-only calls (no GPU): workspace, scratch, plan and fixed-point buffer sizes and the nine words of
ssg_loss_workspace_layout for fused = 0 and 1, over batch sizes, image sizes at and off the tile edges, the three kernel
sizes and capacities around the 128-pixel slot of the tile-major regions.  tests/test_cpu_host.py demands that the
library reports exactly these numbers: the file is regenerated only when a change MEANS to move a size or an offset.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

BATCHES = (1, 2, 16)
IMAGES = ((26, 26), (64, 64), (70, 100), (250, 330), (256, 256))
KERNELS = (11, 25, 49)
CHANNELS = 3
COLUMNS = ("loss_workspace_bytes", "loss_rows_bytes", "loss_tm_bytes", "loss_scratch_bytes", "backward_scratch_bytes",
           "forward_plan_bytes", "edge_scratch_bytes", "grad_fix_bytes", "layout_fused0", "layout_fused1")


def capacities(B, H, W):
    return (1, 100, 127, 128, 129, 5000, B * H * W)


def cases():
    for B in BATCHES:
        for H, W in IMAGES:
            for ks in KERNELS:
                for cap in capacities(B, H, W):
                    yield B, H, W, ks, cap


def measure(L, B, H, W, ks, cap):
    """One row of the fixture: the values of COLUMNS for a case, as the loaded library reports them."""
    lay = (ctypes.c_size_t * 9)()
    layouts = []
    for fused in (0, 1):
        assert L.ssg_loss_workspace_layout(B, H, W, cap, ks, fused, lay) == 0
        layouts.append(list(lay))
    return [L.ssg_loss_workspace_bytes(B, H, W, cap, ks), L.ssg_loss_rows_bytes(cap, ks), L.ssg_loss_tm_bytes(cap, ks),
            L.ssg_loss_scratch_bytes(B, H, W, cap, ks), L.ssg_backward_scratch_bytes(cap, ks),
            L.ssg_forward_plan_bytes(B, H, W, cap), L.ssg_edge_scratch_bytes(B, H, W),
            L.ssg_grad_fix_bytes(B, CHANNELS, H, W)] + layouts


def main():
    from ssl_amd import _lib
    L = _lib.lib()
    rows = [[B, H, W, ks, cap] + measure(L, B, H, W, ks, cap) for B, H, W, ks, cap in cases()]
    out = os.path.join(HERE, "f21_host_sizes.json")
    with open(out, "w") as f:
        f.write('{"abi_version": %d, "channels": %d,\n "columns": %s,\n "rows": [\n' % (
            L.ssg_abi_version(), CHANNELS, json.dumps(["B", "H", "W", "ks", "capacity"] + list(COLUMNS))))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"{out}: {len(rows)} cases")


if __name__ == "__main__":
    main()
