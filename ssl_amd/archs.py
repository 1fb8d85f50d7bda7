"""The reference's two U-Net discriminators with spectral normalisation, restated in plain torch and fused by default
(ssl_amd/spectral.py): basicsr's `UNetDiscriminatorSN(num_in_ch, num_feat=64, skip_connection=True)`
(options/train/RealESRGANSSL/train_RealESRGANSSL_x4.yml) and KAIR's `Discriminator_UNet(input_nc=3, ndf=64)`
(train_BSGRAN/options/BSRGAN/*.json, net_type discriminator_unet).

Both are the same network: a 3 x 3 stem `conv0`, three 4 x 4 stride-2 convolutions `conv1..conv3` that double the
width, three 3 x 3 convolutions `conv4..conv6` that halve it again, each behind a bilinear x 2 upsampling and with the
encoder's map of the same size added to its output, two more 3 x 3 convolutions `conv7`, `conv8` and a 3 x 3 head `conv9`
to one channel; leaky ReLU (0.2) behind every convolution but the head.  `conv1..conv8` have no bias and are wrapped in
torch.nn.utils.spectral_norm.  The attribute names are the reference's, so its checkpoints load:
`convN.weight_orig`, `convN.weight_u`, `convN.weight_v`, `conv0.weight`, `conv0.bias`, `conv9.weight`, `conv9.bias`.

The convolutions and the upsampling are torch's; what is native here is the weight reparametrisation in front of them.
`fused=False` leaves torch's per-layer hooks in place; `module.spectral.unfuse()` does the same later.
"""
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm

from .spectral import fuse_spectral_norm

__all__ = ["UNetDiscriminatorSN", "Discriminator_UNet"]

# (attribute, width in, width out, kernel, stride) in units of the base width, for conv1 .. conv8
_NORMED = (("conv1", 1, 2, 4, 2), ("conv2", 2, 4, 4, 2), ("conv3", 4, 8, 4, 2), ("conv4", 8, 4, 3, 1),
           ("conv5", 4, 2, 3, 1), ("conv6", 2, 1, 3, 1), ("conv7", 1, 1, 3, 1), ("conv8", 1, 1, 3, 1))


class UNetDiscriminatorSN(nn.Module):
    def __init__(self, num_in_ch, num_feat=64, skip_connection=True, fused=True):
        super().__init__()
        self.skip_connection = skip_connection
        self.conv0 = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        for name, cin, cout, k, stride in _NORMED:
            setattr(self, name, spectral_norm(nn.Conv2d(num_feat * cin, num_feat * cout, k, stride, 1, bias=False)))
        self.conv9 = nn.Conv2d(num_feat, 1, 3, 1, 1)
        # (kept out of the module tree: the handle refers to this module)
        object.__setattr__(self, "spectral", fuse_spectral_norm(self) if fused else None)

    def forward(self, x):
        act = lambda t: F.leaky_relu(t, negative_slope=0.2, inplace=True)                            # noqa: E731
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)       # noqa: E731
        skips = [act(self.conv0(x))]
        for conv in (self.conv1, self.conv2, self.conv3):
            skips.append(act(conv(skips[-1])))
        y = skips.pop()
        for conv in (self.conv4, self.conv5, self.conv6):
            y = act(conv(up(y)))
            skip = skips.pop()
            if self.skip_connection:
                y = y + skip
        return self.conv9(act(self.conv8(act(self.conv7(y)))))


class Discriminator_UNet(UNetDiscriminatorSN):
    """KAIR's constructor on the same network (its skip connections are always on)."""

    def __init__(self, input_nc=3, ndf=64, fused=True):
        super().__init__(input_nc, ndf, True, fused)
