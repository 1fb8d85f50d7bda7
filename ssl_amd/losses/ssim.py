"""KAIR's SSIM criterion behind the reference's names (GAN-Based-SR/train_BSGRAN/models/loss_ssim.py:15-82, the
pytorch-ssim module that models/model_ssl.py selects with G_lossfn_type "ssim"), on the kernels of
ssl_amd/csrc/ssg_ssim.hip: the five windowed moments, the map, its mean and the gradient with respect to either image
come out of one fused call instead of five grouped convolutions and their autograd replay.

Like the reference these return SSIM itself (1 for equal images): the caller's sign and weight stay the caller's
(model_ssl.py:284 multiplies by G_lossfn_weight; the reference's own demo minimises -ssim)."""
import torch
from torch import nn

from .. import engine

__all__ = ["gaussian", "create_window", "ssim", "SSIMLoss"]


def gaussian(window_size, sigma):
    """The window_size normalised fp32 taps of a Gaussian of width sigma centred on tap window_size // 2: the
    exponentials are taken in fp64 and rounded once, the normalisation is fp32 (for sigma 1.5 and odd sizes up to 11
    these are the taps of ssg_ssim_taps bit for bit, tests/test_cpu_ssim.py)."""
    offset = torch.arange(window_size, dtype=torch.float64) - window_size // 2
    taps = torch.exp(offset.square() / (-2.0 * sigma * sigma)).to(torch.float32)
    return taps / taps.sum()


def create_window(window_size, channel):
    """(channel, 1, window_size, window_size) fp32: the outer product of the sigma-1.5 taps with themselves, once per
    channel.  The kernels form the same taps themselves; this table serves callers that read `SSIMLoss.window`."""
    taps = gaussian(window_size, 1.5)
    return torch.outer(taps, taps).repeat(channel, 1, 1, 1)


def ssim(img1, img2, window_size=11, size_average=True):
    """The mean SSIM of two (B,C,H,W) images (a scalar; (B,) per-image means with size_average=False), differentiable
    once with respect to either image or both.  window_size odd and <= 11 (ValueError otherwise); computed in fp32."""
    return engine.ssim_loss(img1, img2, window_size, size_average)


class SSIMLoss(nn.Module):
    """The reference's SSIMLoss(window_size=11, size_average=True) with its attributes: `window_size`, `size_average`,
    `channel` and `window` (the last two follow the input's channel count, device and dtype as in the reference)."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size, self.size_average = engine.check_ssim_window(window_size), size_average
        self._tabulate(1)

    def _tabulate(self, channel, like=None):
        """Sets `channel` and `window`, the latter on the device and in the dtype of `like`."""
        table = create_window(self.window_size, channel)
        self.channel, self.window = channel, table if like is None else table.to(device=like.device, dtype=like.dtype)

    def forward(self, img1, img2):
        out = engine.ssim_loss(img1, img2, self.window_size, self.size_average)
        if (img1.shape[1], img1.dtype, img1.device) != (self.channel, self.window.dtype, self.window.device):
            self._tabulate(img1.shape[1], img1)
        return out
