#!/usr/bin/env python
"""Offline NIQE of the images under one or more folders on the GPU: the reference's
GAN-Based-SR/scripts/metrics/calculate_niqe.py on the HIP NIQE kernels.

    python scripts/calculate_niqe.py --input <image dir> [...] [--crop_border 4] [--params niqe_pris_params.npz]

For every file under an input folder (recursive, sorted, hidden files skipped) the image is decoded with PIL (no
OpenCV), turned from RGB into the BGR order the metric is defined on by index, and uploaded as uint8 (H,W,C);
`ssl_amd.metrics.calculate_niqe(img, crop_border, input_order='HWC', convert_to='y')` does the rest.  Per folder it
writes, beside the folder, NIQE_<folder name>.txt with the reference's lines:

    <basename>. \tNIQE: <x.6f>
    Average NIQE for <folder name>: <x.6f>

--params names the pristine model (niqe_pris_params.npz, the reference's data, which this repository does not ship);
without it ssl_amd.metrics.load_niqe_params looks in SSL_AMD_NIQE_PARAMS and beside an installed basicsr.metrics.
Needs the MI355X: there is no CPU path.
"""
import argparse
import os
import sys
from os import path as osp

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from calculate_psnr_ssim import read_bgr, scandir  # noqa: E402
from ssl_amd import metrics  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--input', nargs='+', required=True, help='Input path')
    ap.add_argument('--crop_border', type=int, default=4, help='Crop border for each side')
    ap.add_argument('--params', type=str, default=None, help='niqe_pris_params.npz (default: see load_niqe_params)')
    args = ap.parse_args(argv)

    for dataset in args.input:
        name = osp.basename(dataset)
        save_txt_path = osp.join(osp.dirname(dataset), f"NIQE_{name}.txt")
        niqe_all = []
        with open(save_txt_path, mode='w', encoding='utf-8') as save_txt:
            for i, img_path in enumerate(sorted(scandir(dataset))):
                basename, _ = osp.splitext(osp.basename(img_path))
                score = metrics.calculate_niqe(read_bgr(img_path), args.crop_border, input_order='HWC', convert_to='y',
                                               niqe_pris_params=args.params)
                print(f'{i+1:3d}: {basename:25}. \tNIQE: {score:.6f}')
                save_txt.write(f"{basename}. \tNIQE: {score:.6f}\n")
                niqe_all.append(score)
            print(args.input)
            average = f"Average NIQE for {name}: {sum(niqe_all) / len(niqe_all):.6f}"
            print(average)
            save_txt.write(average)
    return 0


if __name__ == '__main__':
    sys.exit(main())
