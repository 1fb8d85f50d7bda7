#!/usr/bin/env python
"""Dataset preparation on the GPU, source folder to sub-images (and edge masks) in one pass: the reference's
generate_multiscale_img.py (--variant gan) or generate_multiscale_DF2K.py (--variant dm), then extract_subimages.py,
then -- with --masks -- generate_mask.py / generate_mask_simmatrix.py, chained in memory.

    python scripts/prepare_dataset.py --input <dir of images> --save <dir for the sub-images>
        [--variant gan|dm] [--shortest-edge 512] [--crop-size 512] [--step 256] [--thresh-size 0]
        [--masks <dir>] [--threshold 20] [--keep-multiscale <dir>]

For every source image (sorted, as the scripts list them): the LANCZOS resizes of ssl_amd.prep.multiscale (the HIP kernel
behind `ssg_resample`, Pillow's bytes exactly), the source itself where the script keeps it, and of each of those the
crop_size crops at `step` in row-major order, written as <save>/{name}_s{index:03d}{ext} with the reference's names
({base}T{i}.png, {base}S.png, 'x2' / 'x3' / 'x4' / 'x8' stripped before the index).  With --masks every sub-image also
goes through the Laplacian mask kernel (`ssg_edge_mask_laplacian`) and <masks>/mat/{name}.mat, <masks>/png/{name}.png
and <masks>/statis.txt are written as scripts/generate_mask.py --statis writes them.  No intermediate folder is written
unless --keep-multiscale names one.  PNG is lossless, so for PNG sources the pixels are those of the three reference
scripts run one after the other; a kept source of another format is re-encoded by PIL under its own extension.

Decoding and encoding the image files stay on the CPU (PIL); the resizes, the crops and the masks run on the MI355X, and
there is no CPU path.  Images of mode 'L' and 'RGB' only; an image smaller than the crop is an error (the reference
crashes on it)."""
import argparse
import glob
import os
import shutil
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssl_amd import engine, maskio, prep  # noqa: E402


def masks_of(crops, threshold):
    """(n,h,w) or (n,h,w,3) uint8 on the GPU -> (mask, grad > 0), each (n,h,w) uint8 numpy, from the HIP kernel."""
    x = crops[..., None].expand(-1, -1, -1, 3) if crops.dim() == 3 else crops
    x = x.permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous()
    return (engine.edge_mask_laplacian(x, lap_threshold=threshold).cpu().numpy(),
            engine.edge_mask_laplacian(x, lap_threshold=0.0).cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True)
    ap.add_argument("--save", required=True, help="folder of the sub-images")
    ap.add_argument("--variant", choices=("gan", "dm"), default="gan")
    ap.add_argument("--shortest-edge", type=int, default=512)
    ap.add_argument("--crop-size", type=int, default=512)
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--thresh-size", type=int, default=0)
    ap.add_argument("--masks", help="also write mat/, png/ and statis.txt of every sub-image's edge mask here")
    ap.add_argument("--threshold", type=float, default=20.0)
    ap.add_argument("--keep-multiscale", help="also write the multiscale images (the reference's intermediate folder) here")
    args = ap.parse_args(argv)
    from PIL import Image
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/prepare_dataset.py runs the HIP resize and mask kernels: no GPU visible")
    dev = torch.device("cuda:0")
    os.makedirs(args.save, exist_ok=True)
    if args.keep_multiscale:
        os.makedirs(args.keep_multiscale, exist_ok=True)
    report = None
    if args.masks:
        os.makedirs(os.path.join(args.masks, "mat"), exist_ok=True)
        os.makedirs(os.path.join(args.masks, "png"), exist_ok=True)
        report = maskio.DensityReport(os.path.join(args.masks, "statis.txt"))
    n_sub = 0
    for path in sorted(glob.glob(os.path.join(args.input, '*'))):
        basename, ext = os.path.splitext(os.path.basename(path))
        img = prep.from_pil(Image.open(path), dev)
        scaled, keep = prep.multiscale(img, args.variant, args.shortest_edge)
        items = [(basename + suffix, ".png", im) for suffix, im in scaled] + ([(basename, ext, img)] if keep else [])
        for name, e, im in items:
            if args.keep_multiscale:
                if im is img:
                    shutil.copy(path, args.keep_multiscale)
                else:
                    Image.fromarray(im.cpu().numpy()).save(os.path.join(args.keep_multiscale, name + e))
            subs = prep.extract_subimages(im, args.crop_size, args.step, args.thresh_size)
            crops = torch.stack([c for _, c in subs])
            host = crops.cpu().numpy()
            m = g = None
            if report:
                m, g = masks_of(crops, args.threshold)
            for k, (index, _) in enumerate(subs):
                fname = prep.subimage_name(name, index, e)
                Image.fromarray(host[k]).save(os.path.join(args.save, fname))
                n_sub += 1
                if report:
                    stem = os.path.splitext(fname)[0]
                    maskio.save_mask_png(os.path.join(args.masks, "png", f"{stem}.png"), m[k])
                    maskio.save_mask_mat(os.path.join(args.masks, "mat", f"{stem}.mat"), m[k])
                    report.add(stem, m[k].size, int(g[k].sum()), int(m[k].sum()))
    if report:
        for line in report.close():
            print(line)
    print(f"{n_sub} sub-images written to {args.save}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
