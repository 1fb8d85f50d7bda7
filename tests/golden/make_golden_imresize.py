"""Generate f30_imresize.npz (+ f30_imresize_b.npz) FROM THE REFERENCE ITSELF: its Python restatement of MATLAB's imresize.

Needs the reference tree (which never travels with this repository) and runs on the CPU:

    python tests/golden/make_golden_imresize.py <reference root> [--timing]

It loads GAN-Based-SR/basicsr/utils/matlab_functions.py by file path (importing the `basicsr` package would pull in
OpenCV) and calls its `imresize` on (C,H,W) float32 tensors.  The inputs are stored as BYTES (`in_<name>`, (C,H,W) uint8);
the float input of every case is np.float32(byte) / np.float32(255), formed here exactly as tests/imresize_reference.py's
`fixture_input` forms it.  The outputs are the reference's float32 tensors, stored as their four byte planes
(`out_<tag>`, uint8 (4,C,h,w), little-endian byte i of every float: zlib packs the exponent planes well and the mantissa
planes not at all) and read back by `load_fixture`.  The cases the issue lists take about 1.3 MB that way, so they are
written to two files, each under the limit for a committed file; `cases` in the first file lists every tag, `part_b`
those whose output is in the second (the two largest: imresize_reference.FIXTURE_PART_B).

Cases: scales 1/2, 1/3, 1/4, 1/8, 0.3, 0.7, 1.5, 2, 3, 4 with antialiasing and 1/2, 1/3 without on 3 x 19 x 23 and
3 x 37 x 101; 1/4 and 0.7 with antialiasing on 3 x 300 x 255.  One more candidate, 1/4 WITHOUT antialiasing on
3 x 64 x 48, is there to be skipped: the reference raises on it (no padding is needed at the far end, and its slice
`img[:, -0:, :]` is then the whole image, which does not fit the padding it is copied into).  `skipped` records every
candidate that raised, with the exception's text.  Only DATA is stored; no reference source text.

--timing also times the reference on this machine's CPU for the three inputs of tools/imresize_time.py and writes
imresize_cpu_timing.json beside the fixture (shape, scale, seconds, core count)."""
import argparse
import importlib.util
import json
import os
import sys
import time
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import imresize_reference as R  # noqa: E402

OUT_A = os.path.join(HERE, "f30_imresize.npz")
OUT_B = os.path.join(HERE, "f30_imresize_b.npz")
TIMING = os.path.join(HERE, "imresize_cpu_timing.json")


def synthetic(rng, c, h, w):
    """4 x 4 blocks of two levels under a ramp and a little noise, as bytes (C,H,W)."""
    blocks = np.kron(rng.integers(0, 2, (c, (h + 3) // 4, (w + 3) // 4)) * 180, np.ones((1, 4, 4)))[:, :h, :w]
    ramp = np.linspace(0, 50, w)[None, None, :] + np.linspace(0, 20, h)[None, :, None]
    return np.clip(blocks + ramp + rng.integers(0, 6, (c, h, w)), 0, 255).astype(np.uint8)


def load_reference(root):
    path = os.path.join(root, "GAN-Based-SR", "basicsr", "utils", "matlab_functions.py")
    spec = importlib.util.spec_from_file_location("reference_matlab_functions", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.imresize


def timing(imresize):
    rng = np.random.default_rng(30)
    big = torch.from_numpy(synthetic(rng, 3, 2040, 1356).astype(np.float32) / np.float32(255))
    batch = torch.from_numpy(rng.random((48, 256, 256), dtype=np.float32))
    rows = []

    def run(what, x, scale):
        t0 = time.perf_counter()
        y = imresize(x, scale)
        rows.append({"what": what, "shape": list(x.shape), "scale": scale, "seconds": time.perf_counter() - t0})
        return y

    lr = run("1/4 of one 3 x 2040 x 1356 image (float32 of the bytes / 255)", big, 0.25)
    run("x4 of the result", lr, 4)
    run("1/4 of 16 x 3 x 256 x 256 floats (as 48 planes)", batch, 0.25)
    doc = {"what": "the reference's imresize (basicsr/utils/matlab_functions.py), CPU, one call each, seconds",
           "cores": os.cpu_count(), "torch_threads": torch.get_num_threads(), "torch": torch.__version__, "calls": rows}
    with open(TIMING, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference_root")
    ap.add_argument("--timing", action="store_true")
    args = ap.parse_args()
    imresize = load_reference(args.reference_root)
    rng = np.random.default_rng(30)
    inputs = {name: synthetic(rng, 3, h, w) for name, (h, w) in R.FIXTURE_INPUTS.items()}
    parts = ({"in_" + k: v for k, v in inputs.items()}, {})
    cases, part_b, skipped = [], [], []
    for name, scale_name, aa in R.FIXTURE_CANDIDATES:
        tag = R.case_tag(name, scale_name, aa)
        x = torch.from_numpy(R.fixture_input(inputs[name]))
        try:
            y = imresize(x, R.SCALES[scale_name], antialiasing=aa).numpy()
        except Exception as exc:                                           # noqa: BLE001 (whatever the reference raises)
            skipped.append(f"{tag}: {type(exc).__name__}: {exc}")
            continue
        assert y.dtype == np.float32 and np.isfinite(y).all()
        in_b = tag in R.FIXTURE_PART_B
        parts[in_b]["out_" + tag] = np.ascontiguousarray(y).view(np.uint8).reshape(y.shape + (4,)).transpose(3, 0, 1, 2)
        cases.append(tag)
        if in_b:
            part_b.append(tag)
    assert [c for c in R.FIXTURE_CASE_TAGS if c not in cases] == [], "a case the tests need was skipped"
    parts[0].update(cases=np.array(cases), part_b=np.array(part_b), skipped=np.array(skipped))
    np.savez_compressed(OUT_A, **parts[0])
    np.savez_compressed(OUT_B, **parts[1])
    for p in (OUT_A, OUT_B):
        print(p, os.path.getsize(p), "bytes")
        assert os.path.getsize(p) < 1024 * 1024
    print("skipped:", *skipped, sep="\n  ")
    if args.timing:
        timing(imresize)


if __name__ == "__main__":
    main()
