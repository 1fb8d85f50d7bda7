"""Generate f37_contperceptual.npz FROM THE REFERENCE ITSELF: its LPIPSWithDiscriminator and its
DiagonalGaussianDistribution / normal_kl, on the CPU in fp32.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_contperceptual.py <reference root>

ldm/modules/distributions/distributions.py imports directly.  ldm/modules/losses/contperceptual.py takes everything but
its class from `taming.modules.losses.vqperceptual`, which is not installed: while it loads, that module name is
answered by a stand-in that holds tests/contperceptual_cases.py's small fixed perceptual module and discriminator under
the names `LPIPS` and `NLayerDiscriminator`, an inert `weights_init` (the stored weights are copied in afterwards), and
`hinge_d_loss`, `vanilla_d_loss`, `adopt_weight` written from their published definitions (the approach of
make_golden_diffusion.py).

Stored, numbers only (no reference source text):
  in_{name}                     contperceptual_cases.make_inputs(): the inputs, the stand-ins' weights, the posterior's
                                parameters and the pieces of the `last_layer` construction
  {case}_loss, {case}_log_{key} the returned loss and every log value of contperceptual_cases.CASES
  {case}_grad_{reconstructions, logvar, last_layer}   after loss.backward(), generator cases
  {case}_grad_disc_w0           the discriminator's first weight's gradient, discriminator cases
  dist_{sample, kl, kl_other, nll, mode, std, var, det_kl, det_sample}, normal_kl   the distribution's methods on the
                                same parameters (`sample` after torch.manual_seed(5))
"""
import importlib
import os
import sys
import types
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f37_contperceptual.npz")
sys.path.insert(0, os.path.dirname(HERE))
import contperceptual_cases as C  # noqa: E402


def _stand_in_taming():
    def hinge_d_loss(logits_real, logits_fake):
        return 0.5 * (torch.mean(F.relu(1. - logits_real)) + torch.mean(F.relu(1. + logits_fake)))

    def vanilla_d_loss(logits_real, logits_fake):
        return 0.5 * (torch.mean(F.softplus(-logits_real)) + torch.mean(F.softplus(logits_fake)))

    def adopt_weight(weight, global_step, threshold=0, value=0.):
        return value if global_step < threshold else weight

    leaf = types.ModuleType("taming.modules.losses.vqperceptual")
    leaf.LPIPS, leaf.NLayerDiscriminator = C.StandInPerceptual, C.StandInDiscriminator
    leaf.weights_init = lambda m: None
    leaf.hinge_d_loss, leaf.vanilla_d_loss, leaf.adopt_weight = hinge_d_loss, vanilla_d_loss, adopt_weight
    mods = {}
    for name in ("taming", "taming.modules", "taming.modules.losses"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    mods[leaf.__name__] = leaf
    return mods


def load_reference(root):
    sys.path.insert(0, os.path.join(root, "Diffusion-Based-SR"))
    dist = importlib.import_module("ldm.modules.distributions.distributions")
    stand = _stand_in_taming()
    sys.modules.update(stand)
    try:
        cont = importlib.import_module("ldm.modules.losses.contperceptual")
    finally:
        for name in stand:
            sys.modules.pop(name, None)
    return dist, cont


def record(out, dist, t):
    """the distribution's methods: shared with the package's own by tests/test_cpu_lpips_grad.py"""
    p = dist.DiagonalGaussianDistribution(t["posterior"])
    q = dist.DiagonalGaussianDistribution(t["posterior"].flip(0) * 0.7)
    torch.manual_seed(5)
    out["dist_sample"] = p.sample().numpy()
    out["dist_kl"], out["dist_kl_other"] = p.kl().numpy(), p.kl(q).numpy()
    out["dist_nll"], out["dist_mode"] = p.nll(q.mean).numpy(), p.mode().numpy()
    out["dist_std"], out["dist_var"] = p.std.numpy(), p.var.numpy()
    out["normal_kl"] = dist.normal_kl(p.mean, p.logvar, q.mean, 0.3).numpy()
    d = dist.DiagonalGaussianDistribution(t["posterior"], deterministic=True)
    out["dist_det_kl"], out["dist_det_sample"] = d.kl().numpy(), d.sample().numpy()


def main(root):
    dist, cont = load_reference(root)
    t = C.make_inputs()
    out = {"in_" + k: v.numpy() for k, v in t.items()}
    record(out, dist, t)
    for name in C.CASES:
        loss = C.plug(C.build(cont.LPIPSWithDiscriminator, name), t)
        for key, value in C.run_case(loss, dist.DiagonalGaussianDistribution, t, name).items():
            out[f"{name}_{key}"] = value.numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
