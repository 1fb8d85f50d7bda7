"""Generate f33_spsr.npz FROM THE REFERENCE ITSELF: its Get_gradient / Get_gradient_nopadding and its pixel criteria.

Needs the reference tree (which never travels with this repository) and runs on the CPU:

    python tests/golden/make_golden_spsr.py <reference root>

It imports GAN-Based-SR/basicsr/models/spsrssl_model.py (Get_gradient, Get_gradient_nopadding) and
GAN-Based-SR/basicsr/losses/basic_loss.py (MSELoss, CharbonnierLoss, L1Loss, with loss_util.py's weighted_loss under
them) by path; the packages around them (registries, networks, metrics, the CUDA similarity operator, tqdm, einops) are
stood in for by empty modules, nothing of them is used.  The two map classes call .cuda() on their kernels in the
constructor; nn.Parameter.cuda is neutralised while they are constructed, here only.

Stored, all fp32 from the reference on the CPU, numbers only:
  sr, gt, branch, cot, weight          the inputs (spsr_reference.fixture_inputs)
  map_sr, map_gt, nopad_gt             Get_gradient(sr), Get_gradient(gt), Get_gradient_nopadding(gt)
  map_grad, nopad_grad                 autograd's gradient of <class(sr), cot> with respect to sr, for either class
  sr_loss, sr_grad                     line 363, MSELoss(1e-2)(Get_gradient(sr), Get_gradient(gt)), and d / d sr
  sr_loss_map, sr_grad_map             the same line with <Get_gradient(sr), cot> added to the loss (the map's second
                                       consumer, the gradient discriminator, stood in for by a fixed cotangent)
  br_loss, br_grad                     line 368, L1Loss(5e-1)(branch, Get_gradient_nopadding(gt)), and d / d branch
  c{n}_loss, c{n}_grad                 case n of spsr_reference.PIXEL_CASES: the criterion on (sr, gt) and d / d sr; a
                                       'none' reduction is summed before backward
Before writing, every result that has a bound in tests/spsr_reference.py is held to it and the script fails if one is
outside; tests/test_cpu_spsr.py does so again.  Only DATA is stored; no reference source text.
"""
import importlib.util
import os
import sys
import types
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f33_spsr.npz")
sys.path.insert(0, os.path.dirname(HERE))
import spsr_reference as R  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    class _Registry:
        def register(self):
            return lambda cls: cls
    names = ("tqdm", "einops", "basicsr", "basicsr.archs", "basicsr.archs.vgg_arch", "basicsr.losses", "basicsr.metrics",
             "basicsr.utils", "basicsr.utils.registry", "basicsr.models", "basicsr.models.base_model",
             "basicsr.losses.similarity", "basicsr.losses.similarity.similaritywrapper")
    for name in names:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].__path__ = []
    attrs = {"tqdm": ["tqdm"], "einops": ["rearrange"], "basicsr.archs": ["build_network"],
             "basicsr.archs.vgg_arch": ["VGGFeatureExtractor"], "basicsr.losses": ["build_loss"],
             "basicsr.metrics": ["calculate_metric"], "basicsr.utils": ["get_root_logger", "imwrite", "tensor2img"],
             "basicsr.losses.similarity.similaritywrapper": ["compute_similarity"]}
    for name, members in attrs.items():
        for m in members:
            if not hasattr(sys.modules[name], m):
                setattr(sys.modules[name], m, None)
    sys.modules["basicsr.utils.registry"].LOSS_REGISTRY = _Registry()
    sys.modules["basicsr.utils.registry"].MODEL_REGISTRY = _Registry()
    sys.modules["basicsr.models.base_model"].BaseModel = object
    base = os.path.join(root, "GAN-Based-SR", "basicsr")
    _load(os.path.join(base, "losses", "loss_util.py"), "basicsr.losses.loss_util")
    losses = _load(os.path.join(base, "losses", "basic_loss.py"), "basicsr.losses.basic_loss")
    model = _load(os.path.join(base, "models", "spsrssl_model.py"), "basicsr.models.spsrssl_model")
    return model, losses


def map_classes(model):
    keep = torch.nn.Parameter.cuda
    torch.nn.Parameter.cuda = lambda self, *a, **k: self
    try:
        return model.Get_gradient(), model.Get_gradient_nopadding()
    finally:
        torch.nn.Parameter.cuda = keep


def main(root):
    model, losses = load_reference(root)
    get_grad, get_grad_nopadding = map_classes(model)
    I = R.fixture_inputs()
    out = {k: v.numpy() for k, v in I.items()}
    worst = {}

    def hold(name, got, want, bound):
        s = R.share(got, want, bound)
        assert s <= 1.0, (name, s)
        worst[name] = max(worst.get(name, 0.0), s)

    def leaf(t):
        return t.clone().requires_grad_(True)

    # the maps and their gradients
    for key, cls in (("map", get_grad), ("nopad", get_grad_nopadding)):
        x = leaf(I["sr"])
        m = cls(x)
        (m * I["cot"]).sum().backward()
        hold("map", m, R.gmap(I["sr"]), R.map_bound(I["sr"]))
        hold("map gradient", x.grad, R.adjoint(I["sr"], I["cot"])[0], R.adjoint_bound(I["sr"], I["cot"]))
        out[key + "_grad"] = x.grad.numpy()
        if key == "map":
            out["map_sr"] = m.detach().numpy()
    out["map_gt"], out["nopad_gt"] = get_grad(I["gt"]).numpy(), get_grad_nopadding(I["gt"]).numpy()
    hold("map", out["map_gt"], R.gmap(I["gt"]), R.map_bound(I["gt"]))
    hold("map", out["nopad_gt"], R.gmap(I["gt"]), R.map_bound(I["gt"]))
    n = I["sr"].numel()
    # line 363, alone and with a second consumer of the SR map
    for key, cot in (("", None), ("_map", I["cot"])):
        x = leaf(I["sr"])
        m = get_grad(x)
        loss = losses.MSELoss(loss_weight=R.W_GRADSR)(m, get_grad(I["gt"]))
        (loss if cot is None else loss + (m * cot).sum()).backward()
        want = R.gradient_loss(I["sr"], I["gt"], "mse", 0.0, R.W_GRADSR / n, g_map=cot)
        hold("line 363 loss", loss, want.loss, want.loss_bound(reference_sum=True))
        hold("line 363 gradient", x.grad, want.grad, want.grad_bound)
        out["sr_loss" + key], out["sr_grad" + key] = loss.detach().numpy(), x.grad.numpy()
    # line 368
    b = leaf(I["branch"])
    loss = losses.L1Loss(loss_weight=R.W_BRANCH)(b, get_grad_nopadding(I["gt"]))
    loss.backward()
    want = R.branch_loss(I["branch"], I["gt"], "l1", 0.0, R.W_BRANCH / n)
    hold("line 368 loss", loss, want.loss, want.loss_bound(reference_sum=True))
    hold("line 368 gradient", b.grad, want.grad, want.grad_bound)
    out["br_loss"], out["br_grad"] = loss.detach().numpy(), b.grad.numpy()
    # the criteria
    for k, (name, reduction, weighted) in enumerate(R.PIXEL_CASES):
        kw = dict(eps=R.PIXEL_EPS) if name == "CharbonnierLoss" else {}
        crit = getattr(losses, name)(loss_weight=R.PIXEL_WEIGHT, reduction=reduction, **kw)
        x = leaf(I["sr"])
        loss = crit(x, I["gt"], weight=I["weight"] if weighted else None)
        loss.sum().backward()
        if reduction != "none" and not weighted:
            want = R.pixel(I["sr"], I["gt"], R.PIXEL_KIND[name], R.PIXEL_EPS, R.scale_of(reduction, R.PIXEL_WEIGHT, n))
            hold("criterion loss", loss, want.loss, want.loss_bound(reference_sum=True))
            hold("criterion gradient", x.grad, want.grad, want.grad_bound)
        out[f"c{k}_loss"], out[f"c{k}_grad"] = loss.detach().numpy(), x.grad.numpy()
    assert all(v.dtype == np.float32 for v in out.values())
    np.savez_compressed(OUT, **out)
    for name, s in worst.items():
        print(f"{name}: the reference uses at most {s:.3e} of the bound")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
