"""Generate f32_gan.npz FROM THE REFERENCE ITSELF: its two GANLoss classes and MultiScaleGANLoss.

Needs the reference tree (which never travels with this repository) and runs on the CPU:

    python tests/golden/make_golden_gan.py <reference root>

It imports GAN-Based-SR/basicsr/losses/gan_loss.py (GANLoss, MultiScaleGANLoss) and
GAN-Based-SR/train_BSGRAN/models/loss.py (KAIR's GANLoss) by path; the registry decorator of the first and the
torchvision import of the second (its VGG loss) are stood in for by empty modules, nothing of either is used.

Stored, all fp32 from the reference on the CPU, numbers only:
  x, real, fake, kreal, kfake, s0, s1, s2      the inputs (gan_reference.fixture_inputs)
  p{n}_loss, p{n}_grad                         case n of gan_reference.fixture_plain_cases(): criterion(x, target_is_real
                                               [, is_disc]) and autograd's gradient of it
  r{n}_loss, r{n}_greal, r{n}_gfake            case n of gan_reference.fixture_rel_cases(): the relativistic line as the
                                               models write it (gan_reference.rel_form) and the gradients of the leaves
                                               that require one (the others are stored as zeros)
  m{n}_loss, m{n}_g0, m{n}_g1, m{n}_g2         MultiScaleGANLoss on [s0, s1, s2] (n = 0, 1: vanilla generator real, hinge
                                               discriminator fake) and on [[x, s0], [real, s1], [s2]] (n = 2, vanilla)
Before writing, the plain results are held to the bound of the fp64 restatement tests/gan_reference.py and the script
fails if one is outside; tests/test_cpu_gan.py holds every stored result to it.  Only DATA is stored; no reference
source text.
"""
import importlib.util
import os
import sys
import types
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f32_gan.npz")
sys.path.insert(0, os.path.dirname(HERE))
import gan_reference as R  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    class _Registry:
        def register(self):
            return lambda cls: cls
    for name in ("basicsr", "basicsr.utils", "basicsr.utils.registry", "torchvision"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["basicsr.utils.registry"].LOSS_REGISTRY = _Registry()
    basicsr = _load(os.path.join(root, "GAN-Based-SR", "basicsr", "losses", "gan_loss.py"), "reference_gan_loss")
    kair = _load(os.path.join(root, "GAN-Based-SR", "train_BSGRAN", "models", "loss.py"), "reference_kair_loss")
    return basicsr, kair


def criterion(refs, source, gan_type, labels):
    if source == "basicsr":
        return refs[0].GANLoss(gan_type, labels[0], labels[1], loss_weight=R.FIXTURE_WEIGHT)
    crit = refs[1].GANLoss(gan_type, labels[0], labels[1])
    return lambda x, real, is_disc=False: crit(x, real)


def main(root):
    refs = load_reference(root)
    I = R.fixture_inputs()
    out = {k: v.numpy() for k, v in I.items()}
    worst = 0.0
    for n, (source, gan_type, real, disc, labels) in enumerate(R.fixture_plain_cases()):
        x = I["x"].clone().requires_grad_(True)
        loss = criterion(refs, source, gan_type, labels)(x, real, disc)
        loss.backward()
        w = R.FIXTURE_WEIGHT if source == "basicsr" and not disc else 1.0
        sp = R.spec(gan_type, real, disc, *labels)
        want_l, want_g = R.plain(I["x"], sp, w)
        d = R.delta(I["x"])
        s = max(R.share(loss, want_l, R.loss_bound(d, sp, w)), R.share(x.grad, want_g, R.grad_bound(d, sp, w / d.numel())))
        assert s <= 1.0, (n, source, gan_type, real, disc, labels, s)
        worst = max(worst, s)
        out[f"p{n}_loss"], out[f"p{n}_grad"] = loss.detach().numpy(), x.grad.numpy()
    for n, (source, gan_type, labels, form) in enumerate(R.fixture_rel_cases()):
        kr, kf = ("real", "fake") if source == "basicsr" else ("kreal", "kfake")
        need = R.rel_needs(form)
        real, fake = I[kr].clone().requires_grad_(need[0]), I[kf].clone().requires_grad_(need[1])
        crit = criterion(refs, source, gan_type, labels)
        mean = torch.mean if source == "basicsr" else (lambda t: torch.mean(t, 0, True))
        term = lambda p, o, is_real, is_disc: crit(p - mean(o), is_real, is_disc)   # noqa: E731
        gen = lambda r, f: (crit(r - mean(f), False, False) + crit(f - mean(r), True, False)) / 2   # noqa: E731
        loss = R.rel_form(form, real, fake, term, gen)
        loss.backward()
        out[f"r{n}_loss"] = loss.detach().numpy()
        out[f"r{n}_greal"] = (real.grad if need[0] else torch.zeros_like(real)).numpy()
        out[f"r{n}_gfake"] = (fake.grad if need[1] else torch.zeros_like(fake)).numpy()
    scales = [I["s0"], I["s1"], I["s2"]]
    nested = [[I["x"], I["s0"]], [I["real"], I["s1"]], [I["s2"]]]
    for n, (gan_type, real, disc, inputs) in enumerate((("vanilla", True, False, scales), ("hinge", False, True, scales),
                                                         ("vanilla", True, False, nested))):
        crit = refs[0].MultiScaleGANLoss(gan_type, loss_weight=R.FIXTURE_WEIGHT)
        leaves = [t.clone().requires_grad_(True) for t in scales]
        arg = leaves if inputs is scales else [[I["x"], leaves[0]], [I["real"], leaves[1]], [leaves[2]]]
        loss = crit(arg, real, disc)
        loss.backward()
        out[f"m{n}_loss"] = loss.detach().numpy()
        for k, leaf in enumerate(leaves):
            out[f"m{n}_g{k}"] = leaf.grad.numpy()
    np.savez_compressed(OUT, **out)
    print(f"plain cases: the reference uses at most {worst:.3e} of the bounds")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
