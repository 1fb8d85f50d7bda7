"""Fixture F22: the workspace sizes of the three pixel-loss families, recorded from the built library.

    python tests/golden/make_golden_loss_sizes.py        (writes tests/golden/f22_loss_sizes.json)

Host-only calls (no GPU): ssg_ldl_workspace_bytes, ssg_bbl_workspace_bytes and ssg_bp_workspace_bytes over batch sizes,
the image sizes of fixture F21 plus sizes one below, at and one above the edges of the 32 x 16 tile (ldl_map, flat_mask),
the 16 x 8 output tile (bp_fwd) and the 1,024-pixel block of ldl_residual, and the shapes the functions refuse with 0.
Recorded before the three workspaces were laid out by one carver; tests/test_cpu_host.py demands exactly these numbers:
the file is regenerated only when a change MEANS to move a size.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), HERE]

from make_golden_sizes import BATCHES, IMAGES  # noqa: E402  (F21's batch and image sizes)

TILE_EDGES = ((15, 31), (16, 32), (17, 33),      # the 32 x 16 tile
              (7, 15), (8, 16), (9, 17),         # the 16 x 8 tile
              (31, 33), (32, 32), (25, 41))      # 1,023 / 1,024 / 1,025 pixels: the residual kernel's block
SIZES = IMAGES + TILE_EDGES
BBL_KS = ((3, 3), (3, 4), (2, 2))
BBL_CHANNELS = (1, 3)
BP_FACTORS = (2, 3, 4)
BP_CHANNELS = (1, 3)      # planes = B * channels; 16 * 3 planes of 256 x 256 at s = 2 are 6,144 forward tiles (> 4,096)

# shapes every function refuses: the size is 0
LDL_REFUSED = ((0, 64, 64), (1, 0, 64), (1, 64, 0), (-1, 64, 64))
BBL_REFUSED = ((0, 3, 64, 64, 3, 3), (1, 0, 64, 64, 3, 3), (1, 3, 0, 64, 3, 3), (1, 3, 64, 0, 3, 3), (1, 3, 64, 64, 0, 3),
               (1, 3, 64, 64, 3, 2),                 # stride < ksize
               (1, 4, 64, 64, 3, 3),                 # C k^2 = 36 > 31
               (65536, 1, 16, 16, 2, 2),             # B > 65,535
               (16, 3, 8192, 8192, 3, 3),            # 2^31 elements and more
               (1, 3, 11, 64, 3, 3), (1, 3, 64, 11, 3, 3))   # the 1/4 level holds no patch
BP_REFUSED = ((0, 64, 64, 2), (1, 0, 64, 2), (1, 64, 0, 2), (1, 64, 64, 1), (1, 64, 64, 5), (2, 32768, 32768, 2),
              (1, 0, 64, 4), (1, 5, 64, 4), (1, 64, 5, 4), (1, 3, 64, 3))   # a side below the padding (6 at s = 4, 4 at s = 3)


def ldl_cases():
    for B in BATCHES:
        for H, W in SIZES:
            yield B, H, W
    yield from LDL_REFUSED


def bbl_cases():
    for B in BATCHES:
        for C in BBL_CHANNELS:
            for H, W in SIZES:
                for k, s in BBL_KS:
                    yield B, C, H, W, k, s
    yield from BBL_REFUSED


def bp_cases():
    for B in BATCHES:
        for C in BP_CHANNELS:
            for H, W in SIZES:
                for s in BP_FACTORS:
                    yield B * C, H, W, s
                    if (H, W) in TILE_EDGES[3:6]:   # the same edge in OUTPUT pixels: an image s times the size
                        yield B * C, H * s, W * s, s
    yield from BP_REFUSED


FAMILIES = (("ldl", "ssg_ldl_workspace_bytes", ldl_cases), ("bbl", "ssg_bbl_workspace_bytes", bbl_cases),
            ("bp", "ssg_bp_workspace_bytes", bp_cases))


def main():
    from ssl_amd import _lib
    L = _lib.lib()
    out = os.path.join(HERE, "f22_loss_sizes.json")
    with open(out, "w") as f:
        f.write('{"abi_version": %d' % L.ssg_abi_version())
        for name, fn, cases in FAMILIES:
            rows = [list(c) + [getattr(L, fn)(*c)] for c in cases()]
            f.write(',\n "%s": [\n' % name + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]")
        f.write("}\n")
    print(out)


if __name__ == "__main__":
    main()
