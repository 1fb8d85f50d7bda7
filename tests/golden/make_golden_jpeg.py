"""Generate f25_jpeg_sweep.npz FROM THE REFERENCE ITSELF: DiffJPEG(differentiable=False) on every case of
tests/jpeg_cases.py.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_jpeg.py <reference root>

It imports the reference's GAN-Based-SR/basicsr/utils/diffjpeg.py by path (pure torch, like F14 in make_golden.py) and
runs the module on the CPU in fp32 -- the quantisers' `image.float()` rules out a .double() run -- with the case's
quality: a (B,) float32 tensor (a copy: the module overwrites it with its factors) or a Python int / float.

Stored: `tags` (the case names, in order), `out_<tag>` (B,3,H,W) float32 per case, and `f14_scalar50_fp64`, the
oracle's own float64 output (oracle/datapath_oracle.diffjpeg, default arguments) on sample 0 of fixture F14 at scalar
quality 50 as of the revision that gave the oracle its `flips` and `dtype` arguments, where it was checked to be bit-equal to
the revision before.  The inputs are NOT stored: tests/jpeg_cases.py rebuilds them from their seeds.

Only DATA is stored (expected outputs, names); no reference source text.
"""
import importlib.util
import os
import sys
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import jpeg_cases as jc
    from oracle import datapath_oracle as dp
    spec = importlib.util.spec_from_file_location(
        "ref_diffjpeg", os.path.join(sys.argv[1], "GAN-Based-SR", "basicsr", "utils", "diffjpeg.py"))
    dj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dj)
    module = dj.DiffJPEG(differentiable=False)
    out = dict(tags=np.array(jc.TAGS))
    for tag in jc.TAGS:
        x, quality = jc.case(tag)
        q = torch.as_tensor(quality.copy()) if np.ndim(quality) else quality
        with torch.no_grad():
            y = module(torch.as_tensor(x.copy()), quality=q).contiguous().numpy()
        assert y.dtype == np.float32 and y.shape == x.shape and np.isfinite(y).all(), tag
        out["out_" + tag] = y
        print(f"{tag:26s} {str(x.shape):18s} |out - in| max {np.abs(y - x).max():.3f}")
    f14 = np.load(os.path.join(HERE, "f14_diffjpeg.npz"))
    out["f14_scalar50_fp64"] = dp.diffjpeg(f14["img"][:1], 50)
    path = os.path.join(HERE, "f25_jpeg_sweep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
