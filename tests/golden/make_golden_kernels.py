"""Generate f23_blur_kernels.npz FROM THE REFERENCE ITSELF: the blur, sinc and pulse kernels its dataset makes per
sample for the degradation chain.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_kernels.py <reference root>

It imports the reference's GAN-Based-SR/basicsr/data/degradations.py by path, with `cv2` (unused by the kernel
functions) and `torchvision.transforms.functional_tensor` (not installed; unused here too) stubbed in sys.modules, and
stores

(a) explicit-parameter cases (prefix a_): `a_params` one row per case (kind, K, pad_to, sig_x, sig_y, theta, beta,
    omega_c, isotropic flag; kind numbered as ssl_amd.datapath.KERNEL_KINDS) and `a_ref_<i>`, what the reference's
    circular_lowpass_kernel / bivariate_Gaussian / bivariate_generalized_Gaussian / bivariate_plateau return for it,
    padded as the dataset pads (np.pad by (pad_to - K) // 2) and converted as the dataset converts
    (torch.FloatTensor).  A pulse is the dataset's pulse_tensor construction (zeros with a 1 at the centre).
(b) seeded runs (prefix b_<tag>_): random.seed / np.random.seed, then the dataset's three-kernel sequence for 16
    samples -- the text of my_realesrgan_image_mask_dataset.py's __getitem__ between its "Generate kernels" banner
    and its "BGR to RGB" comment, read from the reference at generation time and executed as it stands on an object
    that carries the attributes its __init__ derives from the options.  Tags: `shipped` (the values of
    options/train/RealESRGANSSL/train_RealESRGANSSL_x4.yml), `all` (all six kernel types, sinc_prob 0.3,
    final_sinc_prob 0.8), and `wide` (kernel sizes 7 .. 21 with the fork's literal padded size 9 replaced by stock
    Real-ESRGAN's 21 in the executed text, so that the K >= 13 cutoff range is drawn).  Stored: the seed, repr(options),
    the (16, 3, pad, pad) float32 kernels and both generators' next draw after the run (where their streams ended).
(c) `b_<tag>_cpu_seconds`: the wall time of the 16 samples of (b) on the CPU of the build container.

Only DATA is stored (parameters, options, expected outputs); no reference source text.
"""
import importlib.util
import math
import os
import random
import re
import sys
import textwrap
import time
import types
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"pulse": 0, "sinc": 1, "gaussian": 2, "generalized": 3, "plateau": 4}
PI = math.pi


def load_degradations(root):
    names = ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional_tensor")
    saved = {k: sys.modules.get(k) for k in names}
    for k in names:
        sys.modules[k] = types.ModuleType(k)
    sys.modules["torchvision.transforms.functional_tensor"].rgb_to_grayscale = None
    spec = importlib.util.spec_from_file_location(
        "ref_degradations_kernels", os.path.join(root, "GAN-Based-SR", "basicsr", "data", "degradations.py"))
    deg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(deg)
    for k, v in saved.items():
        if v is not None:
            sys.modules[k] = v
        else:
            sys.modules.pop(k, None)
    return deg


def explicit_cases():
    """(kind, K, pad_to, sig_x, sig_y, theta, beta, omega_c, isotropic)"""
    sizes = [(3, 9), (9, 9), (7, 9), (3, 21), (9, 21), (19, 21), (21, 21)]     # K = pad_to, K = pad_to - 2, small in large
    c = []
    for K, P in sizes:
        c.append(("pulse", K, P, 0, 0, 0, 0, 0, 0))
        c.append(("sinc", K, P, 0, 0, 0, 0, 0.4 * PI + 0.01 * K, 0))
        c.append(("gaussian", K, P, 1.3, 1.3, 0, 0, 0, 1))
        c.append(("gaussian", K, P, 2.1, 0.7, 0.6, 0, 0, 0))
        c.append(("generalized", K, P, 1.7, 1.7, 0, 1.6, 0, 1))
        c.append(("generalized", K, P, 0.9, 2.4, -1.1, 0.6, 0, 0))
        c.append(("plateau", K, P, 1.5, 1.5, 0, 1.8, 0, 1))
        c.append(("plateau", K, P, 2.6, 1.1, 2.2, 0.7, 0, 0))
    for K, P in ((3, 9), (9, 9), (21, 21)):
        for kind, beta in (("gaussian", 0), ("generalized", 2.0), ("plateau", 2.0)):
            c.append((kind, K, P, 0.1, 0.1, 0, beta, 0, 1))            # sigma 0.1: the tails underflow to 0
            c.append((kind, K, P, 5.0, 5.0, 0, beta, 0, 1))            # sigma 5
            c.append((kind, K, P, 0.1, 5.0, 0.3, beta, 0, 0))          # both corners in one anisotropic kernel
            c.append((kind, K, P, 5.0, 0.1, -2.0, beta, 0, 0))
            c.append((kind, K, P, 1.4, 1.4, 0.9, beta, 0, 0))          # sig_x = sig_y with a rotation
            c.append((kind, K, P, 2.0, 0.8, PI, beta, 0, 0))           # theta = +- pi
            c.append((kind, K, P, 2.0, 0.8, -PI, beta, 0, 0))
        for kind in ("generalized", "plateau"):
            for beta in (0.1, 1.0, 8.0):
                c.append((kind, K, P, 1.2, 1.2, 0, beta, 0, 1))
                c.append((kind, K, P, 0.6, 3.0, 0.75, beta, 0, 0))
                c.append((kind, K, P, 0.1, 5.0, 1.9, beta, 0, 0))
    c.append(("sinc", 3, 9, 0, 0, 0, 0, PI, 0))                        # the cutoff range's ends
    c.append(("sinc", 3, 21, 0, 0, 0, 0, PI, 0))
    c.append(("sinc", 21, 21, 0, 0, 0, 0, PI / 5, 0))
    c.append(("sinc", 9, 9, 0, 0, 0, 0, PI / 3, 0))
    c.append(("sinc", 21, 21, 0, 0, 0, 0, PI, 0))
    c.append(("sinc", 13, 21, 0, 0, 0, 0, PI / 5, 0))
    return c


def reference_kernel(deg, case):
    kind, K, P, sx, sy, th, beta, om, iso = case
    if kind == "pulse":
        t = torch.zeros(P, P).float()
        t[P // 2, P // 2] = 1
        return t.numpy()
    if kind == "sinc":
        k = deg.circular_lowpass_kernel(om, K, pad_to=False)
    elif kind == "gaussian":
        k = deg.bivariate_Gaussian(K, sx, sy, th, isotropic=bool(iso))
    elif kind == "generalized":
        k = deg.bivariate_generalized_Gaussian(K, sx, sy, th, beta, isotropic=bool(iso))
    else:
        k = deg.bivariate_plateau(K, sx, sy, th, beta, isotropic=bool(iso))
    p = (P - K) // 2
    return torch.FloatTensor(np.pad(k, ((p, p), (p, p)))).numpy()


SHIPPED = dict(blur_kernel_size_min=1, blur_kernel_size_max=3, kernel_list=['iso', 'aniso'], kernel_prob=[0.7, 0.3],
               sinc_prob=0.01, blur_sigma=[0.1, 0.6], betag_range=[0.1, 2.0], betap_range=[0.1, 1.0],
               blur_kernel_size_min2=1, blur_kernel_size_max2=2, kernel_list2=['iso', 'aniso'], kernel_prob2=[0.7, 0.3],
               sinc_prob2=0.01, blur_sigma2=[0.1, 0.4], betag_range2=[0.1, 2.0], betap_range2=[0.1, 1.0],
               final_sinc_prob=0.1)
SIX = ['iso', 'aniso', 'generalized_iso', 'generalized_aniso', 'plateau_iso', 'plateau_aniso']
ALL = dict(blur_kernel_size_min=1, blur_kernel_size_max=4, kernel_list=SIX, kernel_prob=[0.2, 0.2, 0.15, 0.15, 0.15, 0.15],
           sinc_prob=0.3, blur_sigma=[0.2, 3.0], betag_range=[0.5, 4.0], betap_range=[1.0, 2.0],
           blur_kernel_size_min2=1, blur_kernel_size_max2=3, kernel_list2=SIX, kernel_prob2=[0.1, 0.1, 0.2, 0.2, 0.2, 0.2],
           sinc_prob2=0.3, blur_sigma2=[0.2, 1.5], betag_range2=[0.5, 4.0], betap_range2=[1.0, 2.0],
           final_sinc_prob=0.8)
WIDE = dict(ALL, blur_kernel_size_min=3, blur_kernel_size_max=10, blur_kernel_size_min2=3, blur_kernel_size_max2=10)
RUNS = [("shipped", SHIPPED, 9, 2301), ("all", ALL, 9, 2302), ("wide", WIDE, 21, 2303)]
SAMPLES = 16


def dataset_sequence(root, pad):
    """The dataset's own kernel-making statements as a function of `self`, returning its three kernels."""
    src = open(os.path.join(root, "GAN-Based-SR", "basicsr", "data", "my_realesrgan_image_mask_dataset.py")).read()
    m = re.search(r"\n( *)# -+ Generate kernels \(used in the first degradation\).*?\n(.*?)\n *# BGR to RGB", src, re.S)
    body = textwrap.dedent(m.group(2))
    if pad != 9:                 # the padded size is the only literal 9 of that text: twice for np.pad, once as pad_to
        body, n = re.subn(r"\b9\b", str(pad), body)
        assert n == 3, n
    code = compile("def sequence(self):\n" + textwrap.indent(body, "    ") + "\n    return kernel, kernel2, sinc_kernel\n",
                   "<dataset kernel sequence>", "exec")
    return code


def seeded_run(deg, code, opt, pad, seed):
    ns = dict(random=random, np=np, math=math, torch=torch, circular_lowpass_kernel=deg.circular_lowpass_kernel,
              random_mixed_kernels=deg.random_mixed_kernels)
    exec(code, ns)
    me = types.SimpleNamespace(opt=opt)
    for sfx in ("", "2"):                  # what the dataset's __init__ derives from the options
        for key in ("kernel_list", "kernel_prob", "blur_sigma", "betag_range", "betap_range"):
            setattr(me, key + sfx, opt[key + sfx])
        setattr(me, "kernel_range" + sfx, [2 * v + 1 for v in range(opt["blur_kernel_size_min" + sfx],
                                                                    opt["blur_kernel_size_max" + sfx] + 1)])
    me.pulse_tensor = torch.zeros(pad, pad).float()
    me.pulse_tensor[pad // 2, pad // 2] = 1
    random.seed(seed)
    np.random.seed(seed)
    out = np.zeros((SAMPLES, 3, pad, pad), np.float32)
    t0 = time.perf_counter()
    for i in range(SAMPLES):
        k1, k2, sk = ns["sequence"](me)
        for j, k in enumerate((torch.FloatTensor(k1), torch.FloatTensor(k2), sk)):   # (:139,147-148)
            out[i, j] = k.numpy()
    seconds = time.perf_counter() - t0
    return out, seconds, random.random(), float(np.random.uniform())


def main():
    root = sys.argv[1]
    deg = load_degradations(root)
    out = {}
    cases = explicit_cases()
    out["a_params"] = np.array([[KINDS[c[0]]] + [float(v) for v in c[1:]] for c in cases], np.float64)
    for i, c in enumerate(cases):
        out[f"a_ref_{i}"] = reference_kernel(deg, c)
        assert out[f"a_ref_{i}"].shape == (c[2], c[2]) and out[f"a_ref_{i}"].dtype == np.float32
    print(f"(a) {len(cases)} explicit cases")
    for tag, opt, pad, seed in RUNS:
        code = dataset_sequence(root, pad)
        k, seconds, next_py, next_np = seeded_run(deg, code, opt, pad, seed)
        out[f"b_{tag}_seed"], out[f"b_{tag}_opt"], out[f"b_{tag}_pad"] = np.int64(seed), np.array([repr(opt)]), np.int32(pad)
        out[f"b_{tag}_kernels"], out[f"b_{tag}_cpu_seconds"] = k, np.float64(seconds)
        out[f"b_{tag}_next_random"], out[f"b_{tag}_next_numpy"] = np.float64(next_py), np.float64(next_np)
        pulses = int((k[:, 2].max(axis=(1, 2)) == 1).sum())
        print(f"(b) {tag}: seed {seed} pad {pad}: {SAMPLES} samples in {seconds * 1e3:.2f} ms, {pulses} pulses, "
              f"{int((k < 0).any(axis=(2, 3)).sum())} kernels with negative lobes")
    path = os.path.join(HERE, "f23_blur_kernels.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
