"""The criterion of the Diffusion fork's autoencoder stage (`AutoencoderKLResi`, configs/autoencoder/
autoencoder_kl_64x64x4_resi.yaml): `LPIPSWithDiscriminator` as Diffusion-Based-SR/ldm/modules/losses/contperceptual.py
defines it -- the same constructor, the same forward(inputs, reconstructions, posteriors, optimizer_idx, global_step,
...), the same log keys, the same `calculate_adaptive_weight` -- L1 plus LPIPS as a differentiable term, a learned
`logvar`, an optional KL, the adaptive discriminator weight, a hinge or vanilla discriminator.  The arithmetic and its
order are the fork's, so on its own route the module gives the fork's bits (tests/golden/f37_contperceptual.npz is a
recording of the fork's class); the text is this package's own.

The fork takes LPIPS, the discriminator and four small functions from taming-transformers, which is no dependency of
this package and is not available to its tests; they are written here in plain torch from their published definitions
(supposed equal, not verified): `LPIPS` (ssl_amd.losses.lpips), `NLayerDiscriminator` (the PatchGAN stack, held in
`.main`; `use_actnorm=True` raises NotImplementedError), `weights_init`, `hinge_d_loss`, `vanilla_d_loss`,
`adopt_weight`, and `hinge_d_loss_with_exemplar_weights` after the fork's vqperceptual.py.

Dispatch.  fp32 tensors on one GPU with `weights is None` and the switch on (_gpu.native) take the native route: the
sum of |x - x^| from the L1 pixel criterion (engine.pixel_loss: one streaming pass each way, no |x - x^| tensor), the
perceptual term from ssl_amd.losses.lpips.LPIPS (one launch each way behind the trunk), the mean of the fork's
broadcast sum formed as S / numel + perceptual_weight * mean_n p_n, the nll / logvar / kl / d_weight arithmetic on
0-dim device tensors (fp64 up to the returned fp32 loss) without a host read, -mean(logits_fake) and the hinge / vanilla
discriminator terms through the GAN kernels (GANLoss).  Anything else -- CPU tensors, fp64, half / bf16, `weights=`
given, `inputs` requiring grad, `set_native_criteria(False)` -- takes the torch route with the fork's operations.

One thing is left out on both routes: the fork forms the reconstruction, perceptual and KL terms in the discriminator's
pass as well and reads none of them there; here that pass runs the discriminator and its criterion only.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import _gpu, engine
from .gan_loss import GANLoss
from .lpips import LPIPS

__all__ = ["LPIPSWithDiscriminator", "LPIPS", "NLayerDiscriminator", "weights_init", "hinge_d_loss", "vanilla_d_loss",
           "adopt_weight", "hinge_d_loss_with_exemplar_weights"]


class NLayerDiscriminator(nn.Module):
    """The PatchGAN discriminator of pix2pix as taming builds it: 4x4 convolutions with padding 1 -- one of stride 2
    with LeakyReLU(0.2) and no norm, n_layers - 1 of stride 2 and one of stride 1 with BatchNorm2d and LeakyReLU
    (widths ndf * min(2^n, 8), no bias under BatchNorm), and a last one to a single channel."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=False):
        super().__init__()
        if use_actnorm:
            raise NotImplementedError("ssl_amd: NLayerDiscriminator(use_actnorm=True) needs taming's ActNorm")
        layers = [nn.Conv2d(input_nc, ndf, kernel_size=4, stride=2, padding=1), nn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            layers += [nn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=2 if n < n_layers else 1, padding=1,
                                 bias=False),
                       nn.BatchNorm2d(ndf * mult), nn.LeakyReLU(0.2, True)]
        layers += [nn.Conv2d(ndf * mult, 1, kernel_size=4, stride=1, padding=1)]
        self.main = nn.Sequential(*layers)

    def forward(self, input):
        return self.main(input)


def weights_init(m):
    """Convolutions N(0, 0.02); BatchNorm weight N(1, 0.02) and bias 0 (for `module.apply`)."""
    kind = type(m).__name__
    if 'Conv' in kind:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif 'BatchNorm' in kind:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


def hinge_d_loss(logits_real, logits_fake):
    return 0.5 * (torch.mean(F.relu(1. - logits_real)) + torch.mean(F.relu(1. + logits_fake)))


def vanilla_d_loss(logits_real, logits_fake):
    return 0.5 * (torch.mean(F.softplus(-logits_real)) + torch.mean(F.softplus(logits_fake)))


def hinge_d_loss_with_exemplar_weights(logits_real, logits_fake, weights):
    """The hinge terms as per-sample means over (C, H, W), averaged over the batch with `weights` (N,)."""
    assert weights.shape[0] == logits_real.shape[0] == logits_fake.shape[0]
    per_sample = [torch.mean(F.relu(1. + sign * logits), dim=[1, 2, 3])
                  for sign, logits in ((-1., logits_real), (1., logits_fake))]
    real, fake = ((weights * term).sum() / weights.sum() for term in per_sample)
    return 0.5 * (real + fake)


def adopt_weight(weight, global_step, threshold=0, value=0.):
    """`weight` from step `threshold` on, `value` before."""
    return value if global_step < threshold else weight


# The discriminator's criteria that GANLoss expresses (ssg_gan.hip on fp32 GPU tensors), looked up by the function in
# `disc_loss` at the time of the call: hinge is relu(1 - real), relu(1 + fake); vanilla softplus(-real), softplus(fake).
# The generator's -mean(logits) is 'wgan' towards real.  GANLoss has no parameters, so these are shared.
_DISC_CRITERIA = {hinge_d_loss: GANLoss("hinge"), vanilla_d_loss: GANLoss("wgan_softplus")}
_GENERATOR_TERM = GANLoss("wgan")

# what a pass logs, in the fork's order, and the entries of `return_dic`'s third result that carry the `split/` prefix
# (the fork prefixes all of the discriminator's, none of the generator's with a KL term and two of it without one)
_GENERATOR_LOG = ("total_loss", "logvar", "kl_loss", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss")
_DISCRIMINATOR_LOG = ("disc_loss", "logits_real", "logits_fake")
_PREFIXED_WITHOUT_KL = ("total_loss", "logvar")


def _report(split, values, prefixed):
    """(log, loss_dic) of one pass from its (key, value) pairs: `log` under `split/key`, `loss_dic` under the same for
    the keys in `prefixed` and under the bare key otherwise."""
    log = {f"{split}/{key}": value for key, value in values}
    dic = {(f"{split}/{key}" if key in prefixed else key): value for key, value in values}
    return log, dic


class LPIPSWithDiscriminator(nn.Module):
    """LPIPSWithDiscriminator(disc_start, logvar_init=0.0, kl_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3,
    disc_in_channels=3, disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False,
    disc_conditional=False, disc_loss="hinge"): the fork's arguments; `lpips_weights` (keyword only) names the LPIPS
    weights where the default search finds none (ssl_amd.metrics_feat.load_lpips_weights).

    forward(..., optimizer_idx=0) is the generator's pass and returns (loss, log), optimizer_idx=1 the discriminator's
    and returns (d_loss, log); with return_dic=True a third result holds the logged values again under the fork's keys.
    """

    def __init__(self, disc_start, logvar_init=0.0, kl_weight=1.0, pixelloss_weight=1.0,
                 disc_num_layers=3, disc_in_channels=3, disc_factor=1.0, disc_weight=1.0,
                 perceptual_weight=1.0, use_actnorm=False, disc_conditional=False,
                 disc_loss="hinge", *, lpips_weights=None):
        super().__init__()
        assert disc_loss in ["hinge", "vanilla"]
        self.kl_weight = kl_weight
        self.pixel_weight = pixelloss_weight
        self.perceptual_weight = perceptual_weight
        self.perceptual_loss = LPIPS(lpips_weights).eval()
        self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init)          # the learned output log-variance
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers,
                                                 use_actnorm=use_actnorm).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_loss = {"hinge": hinge_d_loss, "vanilla": vanilla_d_loss}[disc_loss]
        self.disc_factor = disc_factor
        self.discriminator_weight = disc_weight
        self.disc_conditional = disc_conditional

    def calculate_adaptive_weight(self, nll_loss, g_loss, last_layer=None):
        """discriminator_weight * clamp(|d nll / d layer| / (|d g / d layer| + 1e-4), 0, 1e4), detached; `layer` is
        `last_layer`, or the module's own `last_layer[0]` where none is given."""
        layer = last_layer if last_layer is not None else self.last_layer[0]
        nll_grads = torch.autograd.grad(nll_loss, layer, retain_graph=True)[0]
        g_grads = torch.autograd.grad(g_loss, layer, retain_graph=True)[0]
        ratio = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
        return torch.clamp(ratio, 0.0, 1e4).detach() * self.discriminator_weight

    def _takes_kernels(self, inputs, reconstructions, weights):
        return (weights is None and _gpu.native(inputs, reconstructions) and inputs.shape == reconstructions.shape
                and inputs.numel() > 0 and not inputs.requires_grad)

    def _perceptual(self, inputs, reconstructions):
        return self.perceptual_loss(inputs.contiguous(), reconstructions.contiguous())

    def _nll_native(self, inputs, reconstructions):
        """(nll, the same, mean reconstruction error) from the kernels: 0-dim device tensors, the first two fp64 (they
        cost nothing there, and every gradient element is then rounded once)."""
        rec = engine.pixel_loss(reconstructions, inputs, 'l1', loss_weight=1.0 / inputs.numel(), reduction='sum').double()
        if self.perceptual_weight > 0:
            rec = rec + self.perceptual_weight * torch.mean(self._perceptual(inputs, reconstructions).double())
        logvar = self.logvar.double()
        nll = (rec / torch.exp(logvar) + logvar) / inputs.shape[0]
        return nll, nll, rec.detach().float()

    def _nll_torch(self, inputs, reconstructions, weights):
        """(nll, nll under `weights`, mean reconstruction error) in the fork's operations: the full-size error map, the
        perceptual term broadcast onto it, mean over every element divided by the batch size."""
        rec = torch.abs(inputs.contiguous() - reconstructions.contiguous())
        if self.perceptual_weight > 0:
            rec = rec + self.perceptual_weight * self._perceptual(inputs, reconstructions)
        per_element = rec / torch.exp(self.logvar) + self.logvar
        nll = torch.mean(per_element) / per_element.shape[0]
        if weights is None:
            weighted = nll
        else:
            scaled = weights * per_element
            weighted = torch.mean(scaled) / scaled.shape[0]
        return nll, weighted, rec.detach().mean()

    def _logits(self, images, cond):
        images = images.contiguous()
        return self.discriminator(images if cond is None else torch.cat((images, cond), dim=1))

    def _generator_pass(self, inputs, reconstructions, posteriors, factor, last_layer, cond, weights, native):
        if native:
            nll, weighted_nll, rec_mean = self._nll_native(inputs, reconstructions)
        else:
            nll, weighted_nll, rec_mean = self._nll_torch(inputs, reconstructions, weights)
        with_kl = self.kl_weight > 0
        if with_kl:
            kl = posteriors.kl()
            kl = torch.mean(kl) / kl.shape[0]
        assert self.disc_conditional == (cond is not None)
        logits_fake = self._logits(reconstructions, cond)
        g_loss = _GENERATOR_TERM(logits_fake, True) if native else -torch.mean(logits_fake)
        if self.disc_factor > 0.0:
            try:
                d_weight = self.calculate_adaptive_weight(nll, g_loss, last_layer=last_layer)
            except RuntimeError:          # e.g. a layer outside the graph: the fork falls back to weight 1
                d_weight = torch.tensor(1.0) * self.discriminator_weight
        else:
            d_weight = torch.tensor(0.0)
        adversarial = d_weight * factor * g_loss
        loss = weighted_nll + self.kl_weight * kl + adversarial if with_kl else weighted_nll + adversarial
        if native:
            loss, nll = loss.float(), nll.float()
        shown = {"total_loss": loss.clone().detach().mean(), "logvar": self.logvar.detach(),
                 "kl_loss": kl.detach().mean() if with_kl else None, "nll_loss": nll.detach().mean(),
                 "rec_loss": rec_mean, "d_weight": d_weight.detach(), "disc_factor": torch.tensor(factor),
                 "g_loss": g_loss.detach().mean()}
        values = [(key, shown[key]) for key in _GENERATOR_LOG if shown[key] is not None]
        return loss, values, (() if with_kl else _PREFIXED_WITHOUT_KL)

    def _discriminator_pass(self, inputs, reconstructions, factor, cond, native):
        logits_real = self._logits(inputs.detach(), cond)
        logits_fake = self._logits(reconstructions.detach(), cond)
        criterion = _DISC_CRITERIA.get(self.disc_loss) if native else None
        if criterion is not None:
            terms = 0.5 * (criterion(logits_real, True, is_disc=True) + criterion(logits_fake, False, is_disc=True))
        else:
            terms = self.disc_loss(logits_real, logits_fake)
        d_loss = factor * terms
        shown = (d_loss.clone().detach().mean(), logits_real.detach().mean(), logits_fake.detach().mean())
        return d_loss, list(zip(_DISCRIMINATOR_LOG, shown)), _DISCRIMINATOR_LOG

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx,
                global_step, last_layer=None, cond=None, split="train",
                weights=None, return_dic=False):
        native = self._takes_kernels(inputs, reconstructions, weights)
        factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        if optimizer_idx == 0:
            loss, values, prefixed = self._generator_pass(inputs, reconstructions, posteriors, factor, last_layer, cond,
                                                          weights, native)
        elif optimizer_idx == 1:
            loss, values, prefixed = self._discriminator_pass(inputs, reconstructions, factor, cond, native)
        else:
            return None
        log, dic = _report(split, values, prefixed)
        return (loss, log, dic) if return_dic else (loss, log)
