#!/usr/bin/env python
"""Offline LPIPS (v0.1, AlexNet) of restored images against their ground truth: the reference's
GAN-Based-SR/scripts/metrics/calculate_lpips.py on ssl_amd.metrics.calculate_lpips.

    python scripts/calculate_lpips.py --gt <GT dir> [...] --restored <dir> [...] [--crop_border 4] [--suffix _x4] [--correct_mean_var]
                                      [--weights FILE [FILE]]

For every file of a ground-truth folder (sorted) the image and `<restored>/<basename><suffix><ext>` are decoded with
Pillow (no OpenCV) and handed over as BGR uint8 (H,W,3).  Per dataset it writes, beside the restored folder,
LPIPS_<name of the folder above the ground-truth folder>.txt with the reference's lines:

    <basename:25>. \tLPIPS: <x.6f>.
    Average: LPIPS: <x.6f>

--weights names the weights (a state_dict in the package's layout, or a torchvision AlexNet checkpoint and the package's
alex.pth); without it ssl_amd.metrics_feat.load_lpips_weights looks in SSL_AMD_LPIPS_WEIGHTS and at an installed lpips
package.  Nothing is downloaded.  Runs on the GPU where there is one, on the CPU otherwise.
"""
import argparse
import glob
import sys
from os import path as osp

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from calculate_psnr_ssim import read_bgr  # noqa: E402
from ssl_amd import metrics  # noqa: E402


def weights_argument(values):
    if not values:
        return None
    return values[0] if len(values) == 1 else tuple(values)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gt', nargs='+', required=True, help='Path to gt (Ground-Truth)')
    ap.add_argument('--restored', nargs='+', required=True, help='Path to restored images')
    ap.add_argument('--crop_border', type=int, default=4, help='Crop border for each side')
    ap.add_argument('--suffix', type=str, default='', help='Suffix for restored images')
    ap.add_argument('--correct_mean_var', action='store_true', help='Accepted as the reference accepts it; it reads it nowhere.')
    ap.add_argument('--weights', nargs='+', default=None, help='LPIPS weights (default: see load_lpips_weights)')
    args = ap.parse_args(argv)
    weights = weights_argument(args.weights)

    for idx, dataset in enumerate(args.gt):
        save_txt_path = osp.join(osp.dirname(args.restored[idx]), f"LPIPS_{osp.basename(osp.dirname(dataset))}.txt")
        lpips_all = []
        with open(save_txt_path, mode='w', encoding='utf-8') as save_txt:
            for i, img_path in enumerate(sorted(glob.glob(osp.join(dataset, '*')))):
                basename, ext = osp.splitext(osp.basename(img_path))
                img_gt = read_bgr(img_path)
                img_restored = read_bgr(osp.join(args.restored[idx], basename + args.suffix + ext))
                value = metrics.calculate_lpips(img_restored, img_gt, args.crop_border, lpips_weights=weights)
                print(f'{i+1:3d}: {basename:25}. \tLPIPS: {value:.6f}.')
                save_txt.write(f"{basename:25}. \tLPIPS: {value:.6f}.\n")
                lpips_all.append(value)
            print(f'Average: LPIPS: {sum(lpips_all) / len(lpips_all):.6f}')
            save_txt.write(f"Average: LPIPS: {sum(lpips_all) / len(lpips_all):.6f}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
