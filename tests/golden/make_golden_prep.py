"""Generate f29_prep.npz FROM THE REFERENCE ITSELF: the two multiscale preparation scripts run on small synthetic PNGs.

Needs the reference tree (which never travels with this repository) and Pillow, and runs on the CPU:

    python tests/golden/make_golden_prep.py <reference root>

It loads GAN-Based-SR/scripts/data_preparation/generate_multiscale_img.py and
Diffusion-Based-SR/scripts/data_preparation/generate_multiscale_DF2K.py by path and calls their `main` on a temporary
folder of PNGs: modes 'L' and 'RGB', sides between 3 and 90 pixels, among them multiples of 5 and of 3, whose products
with 0.6 and 1 / 3 (inexact in fp64) the scripts truncate.  The GAN script runs with --shortest_edge 24; the DM script's
hard-coded `shortest_edge = 512` is replaced by 24 in its source text as it is loaded (nothing else is touched).

Recorded: `in_<name>` the decoded inputs; `gan_<file stem>` / `dm_<file stem>` every PNG the scripts wrote, decoded;
`gan_kept` / `dm_kept` the names whose source file the script copied / linked beside them.  Only DATA is stored; no
reference source text.  extract_subimages.py needs OpenCV and is not run: its grid is pinned by hand-derived values in
tests/test_cpu_prep.py.
"""
import argparse
import os
import sys
import tempfile
import types
sys.dont_write_bytecode = True

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f29_prep.npz")
SHORTEST_EDGE = 24
# (name, channels, width, height).  0.6 and 1 / 3 are not fp64 numbers, so nearly every product below is inexact; the
# multiples of 5 and of 3 (45, 57, 65, 85, 87, 90) are where a product that fell short of a whole number would truncate
# one pixel lower (for every side below 2,100 it does not: int(w * 0.6) == 6 * w // 10 and int(w * (1 / 3)) == w // 3)
INPUTS = (("a", 3, 90, 61), ("b", 1, 45, 87), ("c", 3, 3, 5), ("d", 1, 24, 24), ("e", 3, 33, 24), ("f", 3, 85, 40),
          ("g", 1, 57, 75), ("h", 3, 23, 50), ("i", 1, 65, 29), ("j", 3, 87, 43), ("k", 1, 5, 3), ("m", 3, 40, 72))


def synthetic(rng, c, w, h):
    """4 x 4 blocks of two levels (the clip's both ends) under a ramp and a little noise: textured, and compressible."""
    blocks = np.kron(rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4, c)) * 200, np.ones((4, 4, 1)))[:h, :w]
    ramp = np.linspace(0, 40, w)[None, :, None] + np.linspace(0, 15, h)[:, None, None]
    a = np.clip(blocks + ramp + rng.integers(0, 4, (h, w, c)), 0, 255).astype(np.uint8)
    return a[..., 0] if c == 1 else a


def load_main(path, patch=None):
    text = open(path).read()
    if patch:
        assert text.count(patch[0]) == 1, patch
        text = text.replace(*patch)
    mod = types.ModuleType("reference_" + os.path.basename(path)[:-3])
    exec(compile(text, path, "exec"), mod.__dict__)
    return mod.main


def written(folder, sources):
    out, kept = {}, []
    for f in sorted(os.listdir(folder)):
        stem = os.path.splitext(f)[0]
        if stem in sources:
            kept.append(stem)
        else:
            out[stem] = np.array(Image.open(os.path.join(folder, f)))
    return out, kept


def main(root):
    rng = np.random.default_rng(29)
    prep = "scripts/data_preparation"
    gan = load_main(os.path.join(root, "GAN-Based-SR", prep, "generate_multiscale_img.py"))
    dm = load_main(os.path.join(root, "Diffusion-Based-SR", prep, "generate_multiscale_DF2K.py"),
                   ("shortest_edge = 512", f"shortest_edge = {SHORTEST_EDGE}"))
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "src")
        os.makedirs(src)
        for name, c, w, h in INPUTS:
            data[f"in_{name}"] = synthetic(rng, c, w, h)
            Image.fromarray(data[f"in_{name}"]).save(os.path.join(src, f"{name}.png"))
        names = {n for n, *_ in INPUTS}
        gan(argparse.Namespace(input=src, save=os.path.join(tmp, "gan"), shortest_edge=SHORTEST_EDGE))
        dm(argparse.Namespace(input=src, output=os.path.join(tmp, "dm")))
        for tag in ("gan", "dm"):
            out, kept = written(os.path.join(tmp, tag), names)
            data.update({f"{tag}_{k}": v for k, v in out.items()})
            data[f"{tag}_kept"] = np.array(kept)
            print(f"{tag}: {len(out)} images, kept {kept}")
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    assert os.path.getsize(OUT) < 300 * 1000


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
