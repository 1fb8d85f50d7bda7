#!/usr/bin/env python
"""Offline DISTS of restored images against their ground truth: the reference's
GAN-Based-SR/scripts/metrics/calculate_dists.py on ssl_amd.metrics.calculate_dists.

    python scripts/calculate_dists.py --gt <GT dir> [...] --restored <dir> [...] [--crop_border 4] [--suffix _x4]
                                      [--weights FILE [FILE]]

For every file of a ground-truth folder (sorted) the image and `<restored>/<basename><suffix><ext>` are decoded with
Pillow as RGB, as the reference does.  Per dataset it writes, beside the restored folder, DISTS_<name of the folder
above the ground-truth folder>.txt with the reference's lines:

    <basename:25>. \tDISTS: <x.6f>.
    DISTS for <GT dir> is: <x.6f>

--weights names the weights (a state_dict in the package's layout, or a torchvision VGG16 checkpoint and the package's
weights.pt); without it ssl_amd.metrics_feat.load_dists_weights looks in SSL_AMD_DISTS_WEIGHTS and at an installed
DISTS_pytorch package.  Nothing is downloaded.  The reference's --device is accepted: the index of the GPU to use.
"""
import argparse
import glob
import sys
from os import path as osp

import numpy as np

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from calculate_lpips import weights_argument  # noqa: E402
from ssl_amd import metrics  # noqa: E402


def read_rgb(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gt', nargs='+', required=True, help='Path to gt (Ground-Truth)')
    ap.add_argument('--restored', nargs='+', required=True, help='Path to restored images')
    ap.add_argument('--crop_border', type=int, default=4, help='Crop border for each side')
    ap.add_argument('--suffix', type=str, default='', help='Suffix for restored images')
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--weights', nargs='+', default=None, help='DISTS weights (default: see load_dists_weights)')
    args = ap.parse_args(argv)
    weights = weights_argument(args.weights)
    import torch
    if torch.cuda.is_available():
        torch.cuda.set_device(args.device)

    for idx, dataset in enumerate(args.gt):
        save_txt_path = osp.join(osp.dirname(args.restored[idx]), f"DISTS_{osp.basename(osp.dirname(dataset))}.txt")
        dists_list = []
        with open(save_txt_path, mode='w', encoding='utf-8') as save_txt:
            for i, img_path in enumerate(sorted(glob.glob(osp.join(dataset, '*')))):
                basename, ext = osp.splitext(osp.basename(img_path))
                img_sr = read_rgb(osp.join(args.restored[idx], basename + args.suffix + ext))
                img_gt = read_rgb(img_path)
                # (calculate_dists calls model(img2, img): the ground truth first, as the reference's script does)
                dists = metrics.calculate_dists(img_sr, img_gt, args.crop_border, color_order='RGB', dists_weights=weights)
                print(f'{i+1:3d}: {basename:25}. \tDISTS: {dists:.6f}.')
                save_txt.write(f"{basename:25}. \tDISTS: {dists:.6f}.\n")
                dists_list.append(dists)
            dists_avg = sum(dists_list) / len(dists_list)
            print(f"DISTS for {dataset} is: {dists_avg:.6f}")
            save_txt.write(f"DISTS for {dataset} is: {dists_avg:.6f}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
