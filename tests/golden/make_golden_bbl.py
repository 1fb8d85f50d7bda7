"""Generate f19_bbl.npz FROM THE REFERENCE ITSELF: BebyGAN's best-buddy search, its loss and the flat mask.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_bbl.py <reference root>

It imports the reference's GAN-Based-SR/basicsr/models/bebyganssl_model.py by path.  That file pulls in the whole
basicsr package at import time; none of it is used by BBL or get_flat_mask, so basicsr.archs, .losses,
.losses.loss_util, .metrics, .utils, .utils.registry, .models.base_model and tqdm are replaced by empty stub modules
(MODEL_REGISTRY.register() returns an identity decorator).  Then, on CPU in fp32, it runs BBL(alpha, beta).forward,
the caller's loss (bebyganssl_model.py:723-724: L1Loss(p1, sel_p2), i.e. F.l1_loss(.., 'mean')), the autograd gradient
of that loss with respect to the output, and get_flat_mask.

Cases (prefix cN_): 1x3x24x24; 1x3x25x22 (odd sides, not divisible by 3 or 4); 1x3x20x16 with alpha = 0.7,
beta = 0.3; 1x1x13x14.  The inputs are tests/bbl_reference.py's textured GT and its blurred, noisy output.  Flat mask
(prefix m_): a 1x3x40x36 8-bit image with exactly flat regions at kernel_size 11 and 3, and every 3-channel GT above.

Only DATA is stored (inputs, expected outputs); no reference source text.
"""
import os
import sys
sys.dont_write_bytecode = True
import types
import importlib.util

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bbl_reference as R  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "GAN-Based-SR", "basicsr", "models", "bebyganssl_model.py")
    for name in ("basicsr", "basicsr.archs", "basicsr.losses", "basicsr.losses.loss_util", "basicsr.metrics",
                 "basicsr.utils", "basicsr.utils.registry", "basicsr.models", "basicsr.models.base_model", "tqdm"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod

    class _Registry:
        def register(self, *a, **k):
            return lambda obj: obj

    sys.modules["basicsr.archs"].build_network = None
    sys.modules["basicsr.losses"].build_loss = None
    sys.modules["basicsr.losses.loss_util"].similarity_map = None
    sys.modules["basicsr.metrics"].calculate_metric = None
    for name in ("get_root_logger", "imwrite", "tensor2img"):
        setattr(sys.modules["basicsr.utils"], name, None)
    sys.modules["basicsr.utils.registry"].MODEL_REGISTRY = _Registry()
    sys.modules["basicsr.models.base_model"].BaseModel = object
    sys.modules["tqdm"].tqdm = None
    spec = importlib.util.spec_from_file_location("basicsr.models.bebyganssl_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(ref, rng, shape, alpha=1.0, beta=1.0, radius=1, noise=0.05):
    gt = R.textured_gt(rng, shape)
    x = R.degraded(rng, gt, radius, noise)
    out = x.clone().requires_grad_(True)
    p1, sel = ref.BBL(alpha=alpha, beta=beta).forward(x=out, gt=gt)
    loss = F.l1_loss(p1, sel, reduction="mean")
    loss.backward()
    d = dict(x=x.numpy(), gt=gt.numpy(), alpha=np.float32(alpha), beta=np.float32(beta), p1=p1.detach().numpy(),
             sel_p2=sel.detach().numpy(), loss=np.float32(loss.item()), grad=out.grad.numpy())
    if shape[1] == 3:
        d["mask"] = ref.get_flat_mask(gt, kernel_size=11, std_thresh=0.025, scale=1).numpy()
    return d


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(19)
    cases = [case(ref, rng, (1, 3, 24, 24)),
             case(ref, rng, (1, 3, 25, 22), radius=2, noise=0.1),
             case(ref, rng, (1, 3, 20, 16), alpha=0.7, beta=0.3),
             case(ref, rng, (1, 1, 13, 14))]
    out = {}
    for i, d in enumerate(cases):
        for key, v in d.items():
            out[f"c{i}_{key}"] = v
        print(f"c{i}: shape {d['x'].shape} N {d['p1'].shape[1]} alpha {float(d['alpha'])} beta {float(d['beta'])} "
              f"loss {float(d['loss']):.6g}" + (f" flat {float(d['mask'].mean()):.3f}" if "mask" in d else ""))
    out["n_cases"] = np.int32(len(cases))
    img = R.natural_like_u8(rng, 1, 40, 36)
    out["m_img"] = img.numpy()
    for k in (11, 3):
        m = ref.get_flat_mask(img, kernel_size=k, std_thresh=0.025, scale=1).numpy()
        out[f"m_mask_k{k}"] = m
        print(f"mask k={k}: flat share {float(m.mean()):.3f}")
    path = os.path.join(HERE, "f19_bbl.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
