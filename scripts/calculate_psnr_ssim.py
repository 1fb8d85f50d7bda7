#!/usr/bin/env python
"""Offline PSNR / SSIM of restored images against their ground truth on the GPU: the reference's
GAN-Based-SR/scripts/metrics/calculate_psnr_ssim.py (without --correct_mean_var) on the HIP metric kernels.

    python scripts/calculate_psnr_ssim.py --gt <GT dir> [...] --restored <restored dir> [...] \
        [--suffix _x4] [--crop_border 4] [--test_y_channel true|false]

For every file under a GT folder (recursive, sorted, hidden files skipped) the restored image is
<restored>/<basename><suffix><ext>.  Images are decoded with PIL (no OpenCV), turned from RGB into the BGR order the
metrics are defined on by index, and uploaded as uint8 (H,W,C); `ssl_amd.metrics.calculate_psnr` / `calculate_ssim`
do the rest.  Per GT folder it writes, beside the restored folder, PSNR_SSIM_<name of the GT folder's parent>.txt with
the reference's lines:

    <basename:25>. \tPSNR: <x.6f> dB, \tSSIM: <y.6f>
    Average: PSNR: <x.6f> dB, SSIM: <y.6f>

The reference converts to Y itself (bgr2ycbcr on uint8 / 255) and passes floats; test_y_channel on the uint8 image is
the same arithmetic.  Needs the MI355X: there is no CPU path.
"""
import argparse
import os
import sys
from os import path as osp

import numpy as np

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from ssl_amd import metrics  # noqa: E402


def scandir(root):
    """Full paths of the files under root, recursive, names starting with '.' skipped (basicsr.utils.scandir)."""
    for entry in os.scandir(root):
        if entry.name.startswith('.'):
            continue
        if entry.is_file():
            yield entry.path
        elif entry.is_dir():
            yield from scandir(entry.path)


def read_bgr(path):
    """uint8 (H,W) or (H,W,3) in BGR order, as cv2.imread(path, IMREAD_UNCHANGED) returns an 8-bit file."""
    from PIL import Image
    im = Image.open(path)
    if im.mode not in ("L", "RGB"):
        im = im.convert("RGB")
    arr = np.array(im)
    return arr if arr.ndim == 2 else arr[..., [2, 1, 0]]


def _bool(text):
    if text.lower() in ("1", "true", "yes", "y"):
        return True
    if text.lower() in ("0", "false", "no", "n"):
        return False
    raise argparse.ArgumentTypeError(f"expected true or false, got {text!r}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gt', nargs='+', required=True, help='Path to gt (Ground-Truth)')
    ap.add_argument('--restored', nargs='+', required=True, help='Path to restored images')
    ap.add_argument('--crop_border', type=int, default=4, help='Crop border for each side')
    ap.add_argument('--suffix', type=str, default='', help='Suffix for restored images')
    ap.add_argument('--test_y_channel', type=_bool, nargs='?', const=True, default=True,
                    help='If true, test Y channel (In MatLab YCbCr format). If false, test RGB channels.')
    args = ap.parse_args(argv)
    if len(args.gt) != len(args.restored):
        ap.error("--gt and --restored take the same number of folders")

    for idx, dataset in enumerate(args.gt):
        psnr_all, ssim_all = [], []
        img_list_gt = sorted(scandir(dataset))
        save_txt_path = osp.join(osp.dirname(args.restored[idx]),
                                 f"PSNR_SSIM_{osp.basename(osp.dirname(dataset))}.txt")
        print('Testing Y channel.' if args.test_y_channel else 'Testing RGB channels.')
        with open(save_txt_path, mode='w', encoding='utf-8') as save_txt:
            for i, img_path in enumerate(img_list_gt):
                basename, ext = osp.splitext(osp.basename(img_path))
                img_gt = read_bgr(img_path)
                img_restored = read_bgr(osp.join(args.restored[idx], basename + args.suffix + ext))
                psnr = metrics.calculate_psnr(img_gt, img_restored, crop_border=args.crop_border, input_order='HWC',
                                              test_y_channel=args.test_y_channel)
                ssim = metrics.calculate_ssim(img_gt, img_restored, crop_border=args.crop_border, input_order='HWC',
                                              test_y_channel=args.test_y_channel)
                print(f'{i+1:3d}: {basename:25}. \tPSNR: {psnr:.6f} dB, \tSSIM: {ssim:.6f}')
                save_txt.write(f"{basename:25}. \tPSNR: {psnr:.6f} dB, \tSSIM: {ssim:.6f}\n")
                psnr_all.append(psnr)
                ssim_all.append(ssim)
            print(args.gt)
            print(args.restored)
            average = (f'Average: PSNR: {sum(psnr_all) / len(psnr_all):.6f} dB, '
                       f'SSIM: {sum(ssim_all) / len(ssim_all):.6f}')
            print(average)
            save_txt.write(average)
    return 0


if __name__ == '__main__':
    sys.exit(main())
