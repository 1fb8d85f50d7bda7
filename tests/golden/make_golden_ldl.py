"""Generate f18_ldl_artifact.npz FROM THE REFERENCE ITSELF: LDL's artifact map and loss.

Run only in the build container (needs the reference tree, which never travels to the GPU box):

    python tests/golden/make_golden_ldl.py

It imports the reference's GAN-Based-SR/basicsr/losses/loss_util.py by path with the same stub as make_golden.py
(the CUDA-only similaritywrapper module replaced in sys.modules) and runs, on CPU in fp32, its get_local_weights,
get_artifact_map and get_refined_artifact_map, then the caller's loss (ldlssl_model.py:220-224):
L1Loss(pixel_weight * output, pixel_weight * gt), i.e. basic_loss.py's loss_weight * F.l1_loss(.., 'mean'), and the
autograd gradient of that loss with respect to the output.

Cases (prefix cN_): k = 7 at 2x3x24x20 with pixels where r == r_e exactly; 1x1x9x11 at k = 3; 1x3x4x5 at k = 7 (the
smallest image reflect padding allows); 2x3x16x13 at k = 9; 2x3x12x10 at k = 7 whose second image has output == GT
(constant residual: the reference's gradient for that image is what this fixture records, NaN or not).

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
REF = "/root/reference/GAN-Based-SR/basicsr/losses/loss_util.py"


def load_reference():
    for name in ("basicsr", "basicsr.losses", "basicsr.losses.similarity"):
        sys.modules.setdefault(name, types.ModuleType(name))
    stub = types.ModuleType("basicsr.losses.similarity.similaritywrapper")

    def compute_similarity(*a, **k):  # never reached here
        raise RuntimeError("CUDA op is not available in the build container")

    stub.compute_similarity = compute_similarity
    sys.modules["basicsr.losses.similarity.similaritywrapper"] = stub
    spec = importlib.util.spec_from_file_location("ref_loss_util", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(ref, rng, shape, k, lam=1.0, same_img=None, tie_frac=0.0):
    B, C, H, W = shape
    g = rng.random(shape, dtype=np.float32)
    o = np.clip(g + rng.normal(0, 0.08, shape).astype(np.float32), 0, 1).astype(np.float32)
    e = np.clip(g + rng.normal(0, 0.06, shape).astype(np.float32), 0, 1).astype(np.float32)
    if tie_frac:   # EMA equal to the output at some pixels: r == r_e exactly there (not masked: the test is strict)
        sel = rng.random((B, 1, H, W)) < tie_frac
        e = np.where(sel, o, e).astype(np.float32)
    if same_img is not None:
        o[same_img] = g[same_img]
    gt, ema = torch.from_numpy(g), torch.from_numpy(e)
    out = torch.from_numpy(o.copy()).requires_grad_(True)
    w = ref.get_refined_artifact_map(gt, out, ema, k)
    loss = lam * F.l1_loss(w * out, w * gt, reduction="mean")
    loss.backward()
    with torch.no_grad():
        w_plain = ref.get_artifact_map(gt, out, k)
        r = torch.sum(torch.abs(gt - out), 1, keepdim=True)
        lw = ref.get_local_weights(r.clone(), k)
        r_e = torch.sum(torch.abs(gt - ema), 1, keepdim=True)
    d = dict(o=o, g=g, e=e, k=np.int32(k), lam=np.float32(lam), w=w.detach().numpy(), w_plain=w_plain.numpy(),
             r=r.numpy(), local=lw.numpy(), mask=(r < r_e).numpy(), ties=(r == r_e).numpy(),
             loss=np.float32(loss.item()), grad=out.grad.numpy())
    return d


def main():
    ref = load_reference()
    rng = np.random.default_rng(18)
    cases = [case(ref, rng, (2, 3, 24, 20), 7, tie_frac=0.05),
             case(ref, rng, (1, 1, 9, 11), 3, lam=0.5),
             case(ref, rng, (1, 3, 4, 5), 7),
             case(ref, rng, (2, 3, 16, 13), 9),
             case(ref, rng, (2, 3, 12, 10), 7, same_img=1)]
    out = {}
    for i, d in enumerate(cases):
        for key, v in d.items():
            out[f"c{i}_{key}"] = v
        nan = np.isnan(d["grad"]).reshape(d["grad"].shape[0], -1)
        print(f"c{i}: shape {d['o'].shape} k {int(d['k'])} loss {float(d['loss']):.6g} masked {int(d['mask'].sum())} "
              f"ties {int(d['ties'].sum())} NaN grad per image {nan.mean(1).tolist()}")
    out["n_cases"] = np.int32(len(cases))
    path = os.path.join(HERE, "f18_ldl_artifact.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
