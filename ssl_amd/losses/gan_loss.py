"""The adversarial criteria behind the reference's names, plain and relativistic, on the kernels of
ssl_amd/csrc/ssg_gan.hip (include/ssg_hip.h section (Q)).

GANLoss / MultiScaleGANLoss mirror GAN-Based-SR/basicsr/losses/gan_loss.py:11-140 (constructor arguments, forward(input,
target_is_real, is_disc), loss_weight for generators only) and serve KAIR's train_BSGRAN/models/loss.py:135-172 as well:
its gan_type names are accepted beside basicsr's, and its forward(input, target_is_real) is the same call with the
default is_disc and the default loss_weight of 1.  Nine *ssl_model.py files and KAIR's model_ssl.py call the criterion
four times per iteration, in the relativistic-average form `cri_gan(real - torch.mean(fake), ...)`;
GANLoss.relativistic_term and GANLoss.relativistic_generator are those lines as one fused call each (the reference has
no name for them).

On fp32 GPU tensors a call is one streaming pass that forms sum l(d) and sum l'(d) in fp64 (ssg_gan_sums; d = x - mean
of the other tensor in the relativistic form, the mean from the same kernel) and, in backward, one pass that writes the
gradient (ssg_gan_grad), instead of the label tensor, the element-wise criterion, the means, the subtraction and their
autograd replay.  Everything else -- CPU tensors, fp64, half / bf16, and, after `set_native_criteria(False)`, a second
derivative through the criterion (the native node is once-differentiable) -- takes the torch expressions below, which
are the reference's operations and give its bits.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _gpu, _lib

__all__ = ["GANLoss", "MultiScaleGANLoss"]

BCE, LS, LINEAR, SOFTPLUS, HINGE = (_lib.CONSTANTS["SSG_GAN_" + k] for k in ("BCE", "LS", "LINEAR", "SOFTPLUS", "HINGE"))

# gan_type (basicsr's names, then KAIR's) -> the criterion family
_FAMILIES = {"vanilla": "bce", "lsgan": "ls", "wgan": "wgan", "wgan_softplus": "softplus", "hinge": "hinge",
             "gan": "bce", "ragan": "bce", "softplusgan": "softplus"}


def _native(*tensors):
    """Whether the tensors can go through ssg_gan_sums / ssg_gan_grad: the package's rule (_gpu.native: the switch, fp32
    tensors on ONE GPU) and none of them empty."""
    if not _gpu.native(*tensors):
        return False
    for t in tensors:       # (a plain loop: a call is host-bound, and a generator costs as much as the rule itself)
        if t.numel() == 0:
            return False
    return True


_CONSTANTS, _WORKSPACES = {}, {}


def _const(device, *values):
    """A cached fp64 device tensor of a few host values (the coefficients a call multiplies on the device: building one
    per call would be a host-to-device copy each)."""
    key = (device, values)
    t = _CONSTANTS.get(key)
    if t is None:
        if len(_CONSTANTS) >= 256:
            _CONSTANTS.clear()
        t = _CONSTANTS[key] = torch.tensor(values, dtype=torch.float64, device=device)
    return t


def _sums_workspace(device, stream):
    """One workspace of the sums per device and stream: calls on one stream run in order, calls on different streams
    never share one."""
    work = _WORKSPACES.get((device, stream))
    if work is None:
        work = _WORKSPACES[(device, stream)] = torch.empty(_lib.lib().ssg_gan_workspace_bytes(), dtype=torch.uint8,
                                                           device=device)
    return work


def _sums(x, spec, shift=None):
    """(sum l(d), sum l'(d)) of the contiguous fp32 GPU tensor x as two device doubles; shift: one device float."""
    out = torch.empty(2, dtype=torch.float64, device=x.device)
    with _gpu.on(x.device):     # (not _gpu.launch: the stream's handle picks the workspace as well)
        stream = _gpu.stream(x.device)
        _lib.check(_lib.lib().ssg_gan_sums(x.data_ptr(), x.numel(), *spec, _gpu.ptr(shift),
                                           _sums_workspace(x.device, stream).data_ptr(), out.data_ptr(), stream))
    return out


def _grad(x, spec, shift, coef):
    """(float)(coef[0] l'(d) + coef[1]) in the shape of the contiguous x; coef: two device doubles."""
    grad = torch.empty_like(x)
    _gpu.launch(x.device, _lib.lib().ssg_gan_grad, x.data_ptr(), x.numel(), *spec, _gpu.ptr(shift), coef.data_ptr(),
                grad.data_ptr())
    return grad


def _mean_shift(x):
    """The mean of x as the kernels' shift: the fp64 sum over n, rounded to fp32 once (one device float)."""
    shift = torch.empty(1, dtype=torch.float32, device=x.device)
    return torch.div(_sums(x, (LINEAR, 1.0, 0.0))[:1], x.numel(), out=shift)


def _scaled(total, scale):
    """fp32 of (device double) total * scale, one rounding."""
    return torch.mul(total, scale, out=torch.empty((), dtype=torch.float32, device=total.device))


# The coefficient pairs of the gradient passes are formed on the device from the upstream gradient g (a 0-dim fp32
# tensor) and cached fp64 constants: a product of a constant pair with g is one small kernel and no copy.
class _PlainCriterion(torch.autograd.Function):
    """weight * mean l(x): one ssg_gan_sums forward, one ssg_gan_grad backward."""

    @staticmethod
    def forward(ctx, x, spec, weight):
        a = x.contiguous()
        ctx.save_for_backward(a)
        ctx.spec, ctx.scale = spec, weight / a.numel()
        return _scaled(_sums(a, spec)[0], ctx.scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, = ctx.saved_tensors
        return _grad(a, ctx.spec, None, _const(a.device, ctx.scale, 0.0) * g), None, None


class _RelativisticTerm(torch.autograd.Function):
    """weight * mean l(pred - mean(other)), the gradient to pred directly and to other through the mean:
    d/d other_j = -weight sum_i l'(d_i) / (n_pred n_other), a constant written by the LINEAR kind (l' = 1)."""

    @staticmethod
    def forward(ctx, pred, other, spec, weight):
        p, o = pred.contiguous(), other.contiguous()
        shift = _mean_shift(o)
        sums = _sums(p, spec, shift)
        ctx.save_for_backward(p, o, shift, sums)
        ctx.spec, ctx.scale = spec, weight / p.numel()
        return _scaled(sums[0], ctx.scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, o, shift, sums = ctx.saved_tensors
        grad_p = grad_o = None
        if ctx.needs_input_grad[0]:
            grad_p = _grad(p, ctx.spec, shift, _const(p.device, ctx.scale, 0.0) * g)
        if ctx.needs_input_grad[1]:
            through = _const(p.device, -ctx.scale / o.numel(), 0.0) * sums[1] * g
            grad_o = _grad(o, (LINEAR, 1.0, 0.0), None, through)
        return grad_p, grad_o, None, None


class _RelativisticPair(torch.autograd.Function):
    """weight / 2 * (mean l_A(real - mean(fake)) + mean l_B(fake - mean(real))): each mean once, one gradient pass per
    tensor that wants one, the direct term (coef[0]) and the term through the mean (coef[1]) in the same pass."""

    @staticmethod
    def forward(ctx, real, fake, spec_a, spec_b, weight):
        r, f = real.contiguous(), fake.contiguous()
        m_r, m_f = _mean_shift(r), _mean_shift(f)
        sa, sb = _sums(r, spec_a, m_f), _sums(f, spec_b, m_r)
        ctx.save_for_backward(r, f, m_r, m_f, sa, sb)
        ctx.specs, ctx.scales = (spec_a, spec_b), (0.5 * weight / r.numel(), 0.5 * weight / f.numel())
        out = torch.empty((), dtype=torch.float32, device=r.device)
        return torch.add(sa[0] * ctx.scales[0], sb[0], alpha=ctx.scales[1], out=out)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        r, f, m_r, m_f, sa, sb = ctx.saved_tensors
        (ka, kb), dev = ctx.scales, r.device
        grad_r = grad_f = None
        if ctx.needs_input_grad[0]:
            coef = torch.addcmul(_const(dev, ka, 0.0), _const(dev, 0.0, -kb / r.numel()), sb[1]) * g
            grad_r = _grad(r, ctx.specs[0], m_f, coef)
        if ctx.needs_input_grad[1]:
            coef = torch.addcmul(_const(dev, kb, 0.0), _const(dev, 0.0, -ka / f.numel()), sa[1]) * g
            grad_f = _grad(f, ctx.specs[1], m_r, coef)
        return grad_r, grad_f, None, None, None


class GANLoss(nn.Module):
    """GANLoss(gan_type, real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0).

    gan_type: 'vanilla' | 'lsgan' | 'wgan' | 'wgan_softplus' | 'hinge' (basicsr) or 'gan' | 'ragan' | 'lsgan' | 'wgan' |
    'softplusgan' (KAIR), in any letter case; anything else raises NotImplementedError.  loss_weight multiplies the
    generator's terms only (is_disc=False); a discriminator's term always has weight 1.

    forward(input, target_is_real, is_disc=False): the mean over every element of
      vanilla / gan / ragan        binary cross entropy of the logits against the real or fake label value
      lsgan                        the squared distance to that label value
      wgan                         -input for a real target, input for a fake one
      wgan_softplus / softplusgan  softplus(-input) for a real target, softplus(input) for a fake one
      hinge                        relu(1 - input) / relu(1 + input) for a discriminator, -input for a generator
    """

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0):
        super().__init__()
        family = _FAMILIES.get(gan_type.lower()) if isinstance(gan_type, str) else None
        if family is None:
            raise NotImplementedError(f"GAN type {gan_type} is not implemented.")
        self.gan_type, self.family = gan_type, family
        self.real_label_val, self.fake_label_val, self.loss_weight = real_label_val, fake_label_val, loss_weight

    def _spec(self, target_is_real, is_disc):
        """(kind, sign, label) of ssg_gan_sums / ssg_gan_grad for one call."""
        label = float(self.real_label_val if target_is_real else self.fake_label_val)
        toward = -1.0 if target_is_real else 1.0
        if self.family == "bce":
            return BCE, 1.0, label
        if self.family == "ls":
            return LS, 1.0, label
        if self.family == "wgan":
            return LINEAR, toward, 0.0
        if self.family == "softplus":
            return SOFTPLUS, toward, 0.0
        return (HINGE, toward, 0.0) if is_disc else (LINEAR, -1.0, 0.0)

    def _torch(self, x, target_is_real, is_disc):
        """The criterion in the reference's torch operations (any device and dtype, twice differentiable)."""
        if self.family in ("bce", "ls"):
            label = x.new_ones(x.size()) * (self.real_label_val if target_is_real else self.fake_label_val)
            loss = F.binary_cross_entropy_with_logits(x, label) if self.family == "bce" else F.mse_loss(x, label)
        elif self.family == "wgan":
            loss = -x.mean() if target_is_real else x.mean()
        elif self.family == "softplus":
            loss = F.softplus(-x).mean() if target_is_real else F.softplus(x).mean()
        elif is_disc:
            loss = F.relu(1 + (-x if target_is_real else x)).mean()
        else:
            loss = -x.mean()
        return loss if is_disc else loss * self.loss_weight

    def _weight(self, is_disc):
        return 1.0 if is_disc else float(self.loss_weight)

    def forward(self, input, target_is_real, is_disc=False):
        if _native(input):
            return _PlainCriterion.apply(input, self._spec(target_is_real, is_disc), self._weight(is_disc))
        return self._torch(input, target_is_real, is_disc)

    def relativistic_term(self, pred, other, target_is_real, is_disc=False):
        """self(pred - torch.mean(other), target_is_real, is_disc) without the subtraction's tensor: the gradient goes to
        `pred` directly and to `other` through its mean, to whichever of the two requires one (pass `other.detach()`
        where the reference detaches).  The mean is the scalar mean over every element; the two sizes may differ."""
        if _native(pred, other):
            return _RelativisticTerm.apply(pred, other, self._spec(target_is_real, is_disc), self._weight(is_disc))
        return self._torch(pred - torch.mean(other), target_is_real, is_disc)

    def relativistic_generator(self, real_pred, fake_pred):
        """(relativistic_term(real_pred, fake_pred, False) + relativistic_term(fake_pred, real_pred, True)) / 2, the
        generator's adversarial term of the relativistic-average models, with each mean formed once."""
        if _native(real_pred, fake_pred):
            return _RelativisticPair.apply(real_pred, fake_pred, self._spec(False, False), self._spec(True, False),
                                           self._weight(False))
        return (self._torch(real_pred - torch.mean(fake_pred), False, False)
                + self._torch(fake_pred - torch.mean(real_pred), True, False)) / 2


class MultiScaleGANLoss(GANLoss):
    """GANLoss over the outputs of a multi-scale discriminator: `input` is a list of tensors, or a list of lists of
    which the last element counts (the features in front of it serve feature matching); the mean over the scales.  A
    tensor is passed to GANLoss.forward unchanged."""

    def forward(self, input, target_is_real, is_disc=False):
        if not isinstance(input, list):
            return super().forward(input, target_is_real, is_disc)
        loss = 0
        for pred in input:
            loss = loss + super().forward(pred[-1] if isinstance(pred, list) else pred, target_is_real, is_disc)
        return loss / len(input)
