"""The Gaussian posterior of the Diffusion fork's autoencoder and the KL divergence between two Gaussians, under the
names the fork's models use (`ldm.modules.distributions.distributions`): `DiagonalGaussianDistribution` with `sample`,
`kl`, `nll`, `mode`, its attributes `mean`, `logvar`, `std`, `var`, `deterministic`, `parameters`, and `normal_kl`.
Torch only, any device and dtype.  The operations and their order are the fork's, so the results are its bits
(tests/golden/f37_contperceptual.npz); the text is this package's own.

What the fork's callers rely on and is kept: the log-variance is clamped to [-30, 20]; a deterministic distribution has
zero spread and answers `kl` and `nll` with a one-element CPU tensor of 0; `sample` draws its noise on the CPU, from
torch's global generator, and moves it to the parameters' device."""
import math

import torch

__all__ = ["AbstractDistribution", "DiracDistribution", "DiagonalGaussianDistribution", "normal_kl"]

LOGVAR_RANGE = (-30.0, 20.0)
_IMAGE_DIMS = [1, 2, 3]


class AbstractDistribution:
    """What a first-stage model's encoder may return: something to `sample` from and a `mode`."""

    def sample(self):
        raise NotImplementedError()

    def mode(self):
        raise NotImplementedError()


class DiracDistribution(AbstractDistribution):
    """All mass on one value."""

    def __init__(self, value):
        self.value = value

    def sample(self):
        return self.value

    def mode(self):
        return self.value


def _nothing():
    return torch.Tensor([0.])


class DiagonalGaussianDistribution(object):
    """An independent Gaussian per element from `parameters` (N, 2 C, H, W): the first C channels are the mean, the
    last C the log-variance."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.deterministic = deterministic
        mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.mean = mean
        self.logvar = torch.clamp(logvar, *LOGVAR_RANGE)
        if deterministic:
            self.var = self.std = torch.zeros_like(mean).to(device=parameters.device)
        else:
            self.std = torch.exp(0.5 * self.logvar)
            self.var = torch.exp(self.logvar)

    def sample(self):
        noise = torch.randn(self.mean.shape).to(device=self.parameters.device)
        return self.mean + self.std * noise

    def mode(self):
        return self.mean

    def kl(self, other=None):
        """KL(self || other) per sample; against the standard normal where `other` is None."""
        if self.deterministic:
            return _nothing()
        if other is None:
            terms = torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar
        else:
            terms = (torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar
                     + other.logvar)
        return 0.5 * torch.sum(terms, dim=_IMAGE_DIMS)

    def nll(self, sample, dims=_IMAGE_DIMS):
        """The negative log-likelihood of `sample`, summed over `dims`."""
        if self.deterministic:
            return _nothing()
        terms = math.log(2.0 * math.pi) + self.logvar + torch.pow(sample - self.mean, 2) / self.var
        return 0.5 * torch.sum(terms, dim=dims)


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL(N(mean1, exp(logvar1)) || N(mean2, exp(logvar2))) element by element, shapes broadcasting.  At least one of
    the four is a tensor; a log-variance given as a number becomes a tensor of that one's dtype and device (torch.exp
    takes no numbers)."""
    like = next((v for v in (mean1, logvar1, mean2, logvar2) if isinstance(v, torch.Tensor)), None)
    assert like is not None, "at least one argument must be a Tensor"
    if not isinstance(logvar1, torch.Tensor):
        logvar1 = torch.tensor(logvar1).to(like)
    if not isinstance(logvar2, torch.Tensor):
        logvar2 = torch.tensor(logvar2).to(like)
    return 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2)
                  + ((mean1 - mean2) ** 2) * torch.exp(-logvar2))
