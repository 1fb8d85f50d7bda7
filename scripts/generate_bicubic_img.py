#!/usr/bin/env python
"""The reference's generate_bicubic_img.m without MATLAB: mod-cropped GT, bicubic LR and bicubic upsample folders.

    python scripts/generate_bicubic_img.py --input <dir of images> [--save-mod DIR] [--save-lr DIR] [--save-bic DIR]
        [--mod-scale 4] [--up-scale 4] [--bic-from-double]

For every source image (sorted) it writes <name>.png into each folder that is named:
  --save-mod  the image cut down to sides that are multiples of --mod-scale (the .m script's modcrop);
  --save-lr   imresize of that by 1 / up_scale with antialiasing, rounded to bytes as MATLAB's imwrite rounds
              (ssl_amd.prep.imresize on the bytes: the HIP kernel behind `ssg_imresize`, fp64 sums);
  --save-bic  imresize of the LR BYTES by up_scale: what a MATLAB user gets who reads the written LR folder back.
              The .m script itself resizes the double-precision LR before it is rounded; --bic-from-double does that
              (the LR is kept as float32 of its fp64 value, not rounded to bytes; the upsample is rounded to float32 and
              then to bytes).

Decoding and encoding the image files stay on the CPU (PIL); the resizes run on the MI355X, and there is no CPU path.
Images of mode 'L' and 'RGB' only, as scripts/prepare_dataset.py."""
import argparse
import glob
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssl_amd import prep  # noqa: E402


def to_bytes(y):
    """MATLAB's uint8 of a double: round half away from zero, saturate (y >= -0.5 here rounds to 0 either way)."""
    return torch.where(y >= 0, torch.floor(y + 0.5).clamp_(max=255.0), torch.zeros_like(y)).to(torch.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True)
    ap.add_argument("--save-mod", help="folder of the mod-cropped GT images")
    ap.add_argument("--save-lr", help="folder of the bicubic-downsampled images")
    ap.add_argument("--save-bic", help="folder of the bicubic-upsampled LR images")
    ap.add_argument("--mod-scale", type=int, default=4)
    ap.add_argument("--up-scale", type=int, default=4)
    ap.add_argument("--bic-from-double", action="store_true",
                    help="upsample the unrounded LR as the .m script does, not the LR bytes")
    args = ap.parse_args(argv)
    from PIL import Image
    if args.mod_scale < 1 or args.up_scale < 1:
        raise ValueError("scripts/generate_bicubic_img.py takes --mod-scale, --up-scale >= 1")
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/generate_bicubic_img.py runs the HIP imresize kernel: no GPU visible")
    dev = torch.device("cuda:0")
    for folder in (args.save_mod, args.save_lr, args.save_bic):
        if folder:
            os.makedirs(folder, exist_ok=True)
    n = 0
    for path in sorted(glob.glob(os.path.join(args.input, '*'))):
        name = os.path.splitext(os.path.basename(path))[0]
        image = Image.open(path)
        if image.mode not in ('L', 'RGB'):
            raise NotImplementedError(f"scripts/generate_bicubic_img.py takes 8-bit 'L' and 'RGB' images; {path} has "
                                      f"mode {image.mode!r}")
        img = prep.modcrop(prep.from_pil(image, dev), args.mod_scale)

        def save(folder, t):
            Image.fromarray(t.cpu().numpy()).save(os.path.join(folder, name + ".png"))

        if args.save_mod:
            save(args.save_mod, img)
        if not (args.save_lr or args.save_bic):
            n += 1
            continue
        lr = prep.imresize(img, 1 / args.up_scale)
        if args.save_lr:
            save(args.save_lr, lr)
        if args.save_bic:
            if args.bic_from_double:
                planes = (img[None] if img.dim() == 2 else img.permute(2, 0, 1)).to(torch.float32)
                up = to_bytes(prep.imresize(prep.imresize(planes, 1 / args.up_scale), args.up_scale).double())
                bic = up[0] if img.dim() == 2 else up.permute(1, 2, 0).contiguous()
            else:
                bic = prep.imresize(lr, args.up_scale)
            save(args.save_bic, bic)
        n += 1
    print(f"{n} images read from {args.input}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
