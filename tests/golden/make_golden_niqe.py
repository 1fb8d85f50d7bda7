"""Generate f26_niqe.npz FROM THE REFERENCE ITSELF: calculate_niqe and the stages inside it.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_niqe.py <reference root> [--timing]

It imports the reference's GAN-Based-SR/basicsr/utils/color_util.py, utils/matlab_functions.py, metrics/metric_util.py
and metrics/niqe.py by path, with the `basicsr` packages around them stubbed in sys.modules (a registry whose
register() returns the function unchanged) and `cv2` stubbed EMPTY: only convert_to='gray' touches it, which no case
here uses.  calculate_niqe reads its niqe_pris_params.npz beside niqe.py, as it always does.

The stages are recorded from the reference's own calls: its compute_feature and imresize are wrapped, so every block
it fits (the MSCN planes, put back together), every feature row and the scale-2 plane are exactly what ran inside
calculate_niqe; the rounded plane is what its own to_y_channel / reorder_image, crop and round give.

Per case (prefix cN_): `img` the input as calculate_niqe receives it, `order` / `crop` its arguments, `x` (the float
RGB tensor a case starts from, of which img is tensor2img's result restated here), `plane` the rounded plane (before
the block crop; uint8, checked exact), `mscn1`, `mscn2`, `plane2` (float32; whole for a case with stages 'full', their
last 16 / 8 / 8 rows `_bottom` and columns `_right` for 'band', absent otherwise: the file stays small), `distparam`
(nblk, 36), `score` (NaN where the reference's fit has fewer than two NaN-free rows: its pinv raises or returns NaN
there; `raised` says which) and `seconds` (CPU).  With --timing
also `timing_shapes` / `timing_seconds`: calculate_niqe's CPU seconds on 1 x 2040 x 1356 x 3 and on 16 images of
256 x 256 x 3 (the sum), kept from the previous file otherwise.

Only DATA is stored (inputs, expected outputs); no reference source text.
"""
import importlib.util
import os
import sys
import time
import types
import warnings
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f26_niqe.npz")


def load_reference(root):
    base = os.path.join(root, "GAN-Based-SR", "basicsr")
    for name in ("basicsr", "basicsr.utils", "basicsr.utils.registry", "basicsr.metrics", "cv2"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod

    class _Registry:
        def register(self, *a, **k):
            return lambda obj: obj

    sys.modules["basicsr.utils.registry"].METRIC_REGISTRY = _Registry()

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    color = load("basicsr.utils.color_util", ("utils", "color_util.py"))
    sys.modules["basicsr.utils"].bgr2ycbcr = color.bgr2ycbcr
    load("basicsr.utils.matlab_functions", ("utils", "matlab_functions.py"))
    util = load("basicsr.metrics.metric_util", ("metrics", "metric_util.py"))
    return load("basicsr.metrics.niqe", ("metrics", "niqe.py")), util


def tensor2img(x):
    x = np.clip(x.astype(np.float32), np.float32(0), np.float32(1)).transpose(1, 2, 0)
    return (np.ascontiguousarray(x[..., ::-1]) * 255.0).round().astype(np.uint8)


def smooth_noise(rng, H, W, sigma):
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c) + 20 * np.sin((xx + yy) / 23.0)
                     for c in range(3)], -1)
    return np.clip(base + rng.normal(0, sigma, base.shape), 0, 255).round().astype(np.uint8)


def hard_edges(rng, H, W):
    img = np.full((H, W, 3), 60.0)
    for _ in range(60):
        y, x = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
        h, w = int(rng.integers(6, 60)), int(rng.integers(6, 60))
        img[y:y + h, x:x + w] = rng.integers(0, 256, 3)
    # (noise of sigma 3 on the flat parts: on flatter ones the reference's float32 E[I^2] - mu^2 loses so many digits
    # that its alpha leaves the fp64 value by a grid step further than 1e-6 from a midpoint)
    return np.clip(img + rng.normal(0, 3.0, img.shape), 0, 255).round().astype(np.uint8)


def make_cases():
    rng = np.random.default_rng(26)
    cases = []
    cases.append(dict(img=smooth_noise(rng, 96, 192, 6.0), order='HWC', crop=0, stages='full'))   # c0 two blocks, one row
    cases.append(dict(img=rng.integers(0, 256, (192, 96, 3), dtype=np.uint8), order='HWC', crop=0))   # c1 one column
    # c2 2 x 3 blocks, remainders on both sides.  Its own generator: on hard-edged content the reference's float32 planes
    # move rhatnorm by up to 3e-6 (relative) against fp64 at scale 2, so a fit that close to a midpoint of the r(gam)
    # table can land one grid step away; the seed is one where no fit lies in that band (tests/test_cpu_niqe.py excuses
    # 1e-6 only)
    cases.append(dict(img=hard_edges(np.random.default_rng(2603), 200, 300), order='HWC', crop=4, stages='band'))
    cases.append(dict(img=np.ascontiguousarray(smooth_noise(rng, 100, 200, 12.0).transpose(2, 0, 1)), order='CHW',
                      crop=2))                                                                  # c3 CHW
    yy, xx = np.mgrid[0:100, 0:200]
    plane = 120 + 70 * np.sin(xx / 6.0) * np.sin(yy / 11.0) + rng.normal(0, 9, (100, 200))
    plane = (np.clip(plane, 0, 255) * 8).round() / 8          # eighths (ties to round among them): exact in float16
    cases.append(dict(img=plane.astype(np.float16), order='HW', crop=2))                        # c4 a float plane
    x = (smooth_noise(rng, 96, 192, 10.0).astype(np.float32) / 255 * 1.3 - 0.15).transpose(2, 0, 1)
    x = np.ascontiguousarray(x[::-1]).astype(np.float16)      # RGB; float16 values, handed on as float32
    cases.append(dict(x=x, img=tensor2img(x.astype(np.float32)), order='HWC', crop=0))          # c5 floats beyond [0, 1]
    grey = rng.integers(0, 256, (192, 192, 1), dtype=np.uint8)
    grey[:112, :112] = 0                      # block (0, 0) and everything its windows and resize taps reach: n == 0
    cases.append(dict(img=grey, order='HWC', crop=0))                                           # c6 a NaN row
    cases.append(dict(img=smooth_noise(rng, 96, 96, 8.0), order='HWC', crop=0))                 # c7 one block: NaN
    return cases


def run_case(ref, util, c):
    """calculate_niqe with its compute_feature and imresize wrapped: returns the stages it went through."""
    blocks, rows, halves = [], [], []
    feature, resize = ref.compute_feature, ref.imresize

    def rec_feature(block):
        blocks.append(np.array(block))
        rows.append(np.array(feature(block), dtype=np.float64))
        return rows[-1].tolist()

    def rec_resize(img, scale, antialiasing=True):
        halves.append(resize(img, scale=scale, antialiasing=antialiasing))
        return halves[-1]

    ref.compute_feature, ref.imresize = rec_feature, rec_resize
    raised = 0
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t0 = time.process_time()
            try:
                score = ref.calculate_niqe(np.asarray(c["img"]), c["crop"], input_order=c["order"], convert_to='y')
            except np.linalg.LinAlgError:
                score, raised = float('nan'), 1
            seconds = time.process_time() - t0
    finally:
        ref.compute_feature, ref.imresize = feature, resize
    # the rounded plane by the reference's own functions
    img = np.asarray(c["img"]).astype(np.float32)
    if c["order"] != 'HW':
        img = np.squeeze(util.to_y_channel(util.reorder_image(img, input_order=c["order"])))
    if c["crop"]:
        img = img[c["crop"]:-c["crop"], c["crop"]:-c["crop"]]
    plane = img.round()
    nbh, nbw = plane.shape[0] // 96, plane.shape[1] // 96
    nblk = nbh * nbw
    assert len(blocks) == 2 * nblk and len(halves) == 1

    def assemble(bl, bs):
        out = np.empty((nbh * bs, nbw * bs), dtype=bl[0].dtype)
        for i, b in enumerate(bl):                    # block column outer
            bx, by = divmod(i, nbh)
            out[by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs] = b
        return out

    assert np.array_equal(plane, plane.astype(np.uint8))
    res = dict(plane=plane.astype(np.uint8), distparam=np.concatenate([np.array(rows[:nblk]), np.array(rows[nblk:])], 1),
               score=np.float64(score), raised=np.int32(raised), seconds=np.float64(seconds))
    stages = dict(mscn1=assemble(blocks[:nblk], 96), mscn2=assemble(blocks[nblk:], 48),
                  plane2=np.asarray(halves[0]) * np.float32(255.))
    if c.get("stages") == 'full':
        res.update(stages)
    elif c.get("stages") == 'band':         # the bottom rows and right columns: where 'nearest' meets the block crop
        for k, w in (("mscn1", 16), ("mscn2", 8), ("plane2", 8)):
            res[k + "_bottom"], res[k + "_right"] = stages[k][-w:], np.ascontiguousarray(stages[k][:, -w:])
    return res


def timing(ref):
    rng = np.random.default_rng(2601)
    big = smooth_noise(rng, 2040, 1356, 6.0)
    small = [smooth_noise(rng, 256, 256, 6.0) for _ in range(16)]
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for imgs in ([big], small):
            t0 = time.process_time()
            for im in imgs:
                ref.calculate_niqe(im, 0, input_order='HWC', convert_to='y')
            out.append(time.process_time() - t0)
    return np.array([[1, 3, 2040, 1356], [16, 3, 256, 256]], np.int32), np.array(out)


def main():
    ref, util = load_reference(sys.argv[1])
    out = {}
    cases = make_cases()
    for i, c in enumerate(cases):
        res = run_case(ref, util, c)
        out[f"c{i}_img"] = c["img"]
        out[f"c{i}_order"] = np.array(c["order"])
        out[f"c{i}_crop"] = np.int32(c["crop"])
        if "x" in c:
            out[f"c{i}_x"] = c["x"]
        for k, v in res.items():
            out[f"c{i}_{k}"] = v
        print(f"c{i} {c['img'].shape} {c['order']} crop {c['crop']}: score {float(res['score']):.7f} "
              f"raised {int(res['raised'])} nan rows {int(np.isnan(res['distparam']).any(1).sum())} "
              f"{float(res['seconds']):.2f} s")
    out["n_cases"] = np.int32(len(cases))
    if "--timing" in sys.argv:
        out["timing_shapes"], out["timing_seconds"] = timing(ref)
        print("timing", out["timing_seconds"])
    elif os.path.exists(OUT):
        old = np.load(OUT)
        if "timing_seconds" in old.files:
            out["timing_shapes"], out["timing_seconds"] = old["timing_shapes"], old["timing_seconds"]
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
