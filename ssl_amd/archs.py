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

SwinIR (basicsr/archs/swinir_arch.py; options/train/SwinIRGANSSL/train_SwinIRGANSSL_bicubic_x4.yml) is restated below
under the reference's attribute names and buffers, so its checkpoints load with strict=True in both directions.  What is
native there is the attention between a block's qkv and proj Linears (ssl_amd/winattn.py); see the text above
`WindowAttention`.
"""
import math

import torch
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint
from torch import nn
from torch.nn.utils import spectral_norm

from . import winattn
from .spectral import fuse_spectral_norm

__all__ = ["UNetDiscriminatorSN", "Discriminator_UNet", "WindowAttention", "SwinTransformerBlock", "BasicLayer", "RSTB",
           "PatchEmbed", "PatchUnEmbed", "Upsample", "UpsampleOneStep", "SwinIR"]

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


# ---- SwinIR ----
# One generator of the reference is not made of convolutions.  Per block, the reference runs torch.roll,
# window_partition, the qkv Linear on windows, a permute, q * scale, a batched matmul that materialises the
# (windows, heads, 64, 64) scores, a gather of the relative-position bias, two adds, a softmax, a second matmul, a
# transpose copy, the proj Linear, window_reverse and a roll back.  With `fused=True` a block whose tensors are in the
# native domain (ssl_amd/winattn.py: fp32 on one GPU, window 8, head_dim <= 32, sides multiples of 8, no live attention
# dropout) runs norm1, attn.qkv on (B, H W, C), winattn.window_attention and attn.proj instead: the Linears act per
# token and so commute with the roll and the partition.  Every other call runs the reference's lines in the reference's
# order (and gives its bits).  The buffers `relative_position_index` and `attn_mask` are registered with the reference's
# values so that state dicts are interchangeable; the native path does not read them.  DropPath sits outside the
# attention and stays torch's.  LayerNorm, the Linears and GELU stay torch's.
def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _drop_path(x, drop_prob=0.0, training=False):
    """Stochastic depth per sample: x / keep times a Bernoulli(keep) draw per sample, formed as the reference forms it."""
    if drop_prob == 0.0 or not training:
        return x
    keep = 1 - drop_prob
    draw = keep + torch.rand((x.shape[0],) + (1,) * (x.ndim - 1), dtype=x.dtype, device=x.device)
    draw.floor_()
    return x.div(keep) * draw


class DropPath(nn.Module):
    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        return _drop_path(x, self.drop_prob, self.training)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


def window_partition(x, window_size):
    """(b, h, w, c) -> (b nW, ws, ws, c)"""
    c = x.shape[-1]
    return winattn._windows(x, window_size).view(-1, window_size, window_size, c)


def window_reverse(windows, window_size, h, w):
    """(b nW, ws, ws, c) -> (b, h, w, c)"""
    b = int(windows.shape[0] / (h * w / window_size / window_size))
    x = windows.view(b, h // window_size, w // window_size, window_size, window_size, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(b, h, w, -1)


class WindowAttention(nn.Module):
    """Multi-head self-attention inside a window, with the relative-position bias; `forward` is the reference's (the
    torch route).  The fused route goes through SwinTransformerBlock, which needs the token grid."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        rows = (2 * window_size[0] - 1) * (2 * window_size[1] - 1)
        self.relative_position_bias_table = nn.Parameter(torch.zeros(rows, num_heads))
        iy = torch.arange(window_size[0]).repeat_interleave(window_size[1])
        ix = torch.arange(window_size[1]).repeat(window_size[0])
        index = ((iy[:, None] - iy[None, :] + window_size[0] - 1) * (2 * window_size[1] - 1)
                 + (ix[:, None] - ix[None, :] + window_size[1] - 1))
        self.register_buffer("relative_position_index", index)
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x, mask=None):
        """x (b nW, n, c); mask (nW, n, n) of 0 / -100 or None"""
        b_, n, c = x.shape
        qkv = self.qkv(x).reshape(b_, n, 3, self.num_heads, c // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        q = q * self.scale
        attn = q @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(n, n, -1)
        attn = attn + bias.permute(2, 0, 1).contiguous().unsqueeze(0)
        if mask is not None:
            nw = mask.shape[0]
            attn = attn.view(b_ // nw, nw, self.num_heads, n, n) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, self.num_heads, n, n)
        attn = self.attn_drop(self.softmax(attn))
        x = (attn @ v).transpose(1, 2).reshape(b_, n, c)
        return self.proj_drop(self.proj(x))

    def extra_repr(self):
        return f"dim={self.dim}, window_size={self.window_size}, num_heads={self.num_heads}"


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, input_resolution, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True,
                 qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm,
                 fused=True):
        super().__init__()
        self.dim, self.input_resolution, self.num_heads = dim, input_resolution, num_heads
        self.window_size, self.shift_size, self.mlp_ratio = window_size, shift_size, mlp_ratio
        self.fused = fused
        if min(self.input_resolution) <= self.window_size:       # a grid of one window is not partitioned
            self.shift_size = 0
            self.window_size = min(self.input_resolution)
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=_pair(self.window_size), num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.register_buffer("attn_mask", self.calculate_mask(self.input_resolution) if self.shift_size > 0 else None)

    def calculate_mask(self, x_size):
        return winattn.shift_mask(x_size[0], x_size[1], self.window_size, self.shift_size)

    def takes_kernels(self, x, x_size):
        """Whether this call's attention goes to ssl_amd.winattn's kernels ("Which calls take the kernels")."""
        from . import _gpu
        h, w = x_size
        return (self.fused and self.window_size == winattn.WINDOW and h % winattn.WINDOW == 0
                and w % winattn.WINDOW == 0 and self.dim % self.num_heads == 0
                and self.dim // self.num_heads <= winattn.MAX_HEAD_DIM
                and not (self.training and self.attn.attn_drop.p > 0)
                and _gpu.native(x, self.attn.relative_position_bias_table, self.attn.qkv.weight, self.attn.proj.weight))

    def _attention(self, x, x_size):
        """norm1's output (b, h w, c) -> the attention's (b, h w, c)"""
        h, w = x_size
        b, _, c = x.shape
        if self.takes_kernels(x, x_size):
            qkv = self.attn.qkv(x).view(b, h, w, 3 * c)
            x = winattn.window_attention(qkv, self.attn.relative_position_bias_table, self.num_heads, self.window_size,
                                         self.shift_size, self.attn.scale)
            return self.attn.proj_drop(self.attn.proj(x.view(b, h * w, c)))
        x = x.view(b, h, w, c)
        if self.shift_size > 0:
            x = torch.roll(x, shifts=(-self.shift_size, -self.shift_size), dims=(1, 2))
        windows = window_partition(x, self.window_size).view(-1, self.window_size * self.window_size, c)
        if self.input_resolution == x_size:
            windows = self.attn(windows, mask=self.attn_mask)
        else:       # (testing on an image of another size: the mask is made for it; all zeros in an unshifted block)
            windows = self.attn(windows, mask=self.calculate_mask(x_size).to(x.device))
        x = window_reverse(windows.view(-1, self.window_size, self.window_size, c), self.window_size, h, w)
        if self.shift_size > 0:
            x = torch.roll(x, shifts=(self.shift_size, self.shift_size), dims=(1, 2))
        return x.view(b, h * w, c)

    def forward(self, x, x_size):
        x = x + self.drop_path(self._attention(self.norm1(x), x_size))
        return x + self.drop_path(self.mlp(self.norm2(x)))

    def extra_repr(self):
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, "
                f"window_size={self.window_size}, shift_size={self.shift_size}, mlp_ratio={self.mlp_ratio}")


class BasicLayer(nn.Module):
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False,
                 fused=True):
        super().__init__()
        self.dim, self.input_resolution, self.depth, self.use_checkpoint = dim, input_resolution, depth, use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, window_size=window_size,
                                 shift_size=0 if i % 2 == 0 else window_size // 2, mlp_ratio=mlp_ratio,
                                 qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                 norm_layer=norm_layer, fused=fused) for i in range(depth)])
        self.downsample = None if downsample is None else downsample(input_resolution, dim=dim, norm_layer=norm_layer)

    def forward(self, x, x_size):
        for blk in self.blocks:
            # (the reference's checkpoint call leaves x_size out and cannot run; it is passed here)
            x = checkpoint.checkpoint(blk, x, x_size, use_reentrant=False) if self.use_checkpoint else blk(x, x_size)
        return x if self.downsample is None else self.downsample(x)

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, depth={self.depth}"


class PatchEmbed(nn.Module):
    """(b, c, h, w) -> (b, h w, c), normalised where a norm_layer is given"""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.img_size, self.patch_size = _pair(img_size), _pair(patch_size)
        self.patches_resolution = [self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1]]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.norm = None if norm_layer is None else norm_layer(embed_dim)

    def forward(self, x):
        x = x.flatten(2).transpose(1, 2)
        return x if self.norm is None else self.norm(x)


class PatchUnEmbed(nn.Module):
    """(b, h w, c) -> (b, c, h, w)"""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.img_size, self.patch_size = _pair(img_size), _pair(patch_size)
        self.patches_resolution = [self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1]]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans, self.embed_dim = in_chans, embed_dim

    def forward(self, x, x_size):
        return x.transpose(1, 2).view(x.shape[0], self.embed_dim, x_size[0], x_size[1])


def _residual_conv(dim, resi_connection):
    if resi_connection == "1conv":
        return nn.Conv2d(dim, dim, 3, 1, 1)
    if resi_connection == "3conv":            # fewer parameters
        return nn.Sequential(nn.Conv2d(dim, dim // 4, 3, 1, 1), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                             nn.Conv2d(dim // 4, dim // 4, 1, 1, 0), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                             nn.Conv2d(dim // 4, dim, 3, 1, 1))
    return None


class RSTB(nn.Module):
    """A BasicLayer, a convolution on the image form of its output, and the residual."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False,
                 img_size=224, patch_size=4, resi_connection="1conv", fused=True):
        super().__init__()
        self.dim, self.input_resolution = dim, input_resolution
        self.residual_group = BasicLayer(dim=dim, input_resolution=input_resolution, depth=depth, num_heads=num_heads,
                                         window_size=window_size, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                         qk_scale=qk_scale, drop=drop, attn_drop=attn_drop, drop_path=drop_path,
                                         norm_layer=norm_layer, downsample=downsample, use_checkpoint=use_checkpoint,
                                         fused=fused)
        conv = _residual_conv(dim, resi_connection)
        if conv is not None:
            self.conv = conv
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=0, embed_dim=dim)
        self.patch_unembed = PatchUnEmbed(img_size=img_size, patch_size=patch_size, in_chans=0, embed_dim=dim)

    def forward(self, x, x_size):
        return self.patch_embed(self.conv(self.patch_unembed(self.residual_group(x, x_size), x_size))) + x


class Upsample(nn.Sequential):
    """Convolution + PixelShuffle(2) per factor of two, or one pair for scale 3."""

    def __init__(self, scale, num_feat):
        if scale & (scale - 1) == 0:
            steps = [2] * int(math.log(scale, 2))
        elif scale == 3:
            steps = [3]
        else:
            raise ValueError(f"scale {scale} is not supported. Supported scales: 2^n and 3.")
        m = []
        for r in steps:
            m += [nn.Conv2d(num_feat, r * r * num_feat, 3, 1, 1), nn.PixelShuffle(r)]
        super().__init__(*m)


class UpsampleOneStep(nn.Sequential):
    """One convolution and one PixelShuffle, whatever the scale (lightweight SR)."""

    def __init__(self, scale, num_feat, num_out_ch, input_resolution=None):
        self.num_feat, self.input_resolution = num_feat, input_resolution
        super().__init__(nn.Conv2d(num_feat, (scale ** 2) * num_out_ch, 3, 1, 1), nn.PixelShuffle(scale))


class SwinIR(nn.Module):
    """The reference's SwinIR(img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths, num_heads, window_size=7, ...)
    with `fused=True` added; upsampler is 'pixelshuffle', 'pixelshuffledirect', 'nearest+conv' or anything else (no
    upsampling: denoising, JPEG artifacts)."""

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6),
                 window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False, upscale=2,
                 img_range=1.0, upsampler="", resi_connection="1conv", fused=True, **kwargs):
        super().__init__()
        num_out_ch, num_feat = in_chans, 64
        self.window_size, self.img_range, self.upscale, self.upsampler = window_size, img_range, upscale, upsampler
        self.mean = (torch.Tensor((0.4488, 0.4371, 0.4040)).view(1, 3, 1, 1) if in_chans == 3
                     else torch.zeros(1, 1, 1, 1))
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)

        self.num_layers, self.embed_dim, self.ape, self.patch_norm = len(depths), embed_dim, ape, patch_norm
        self.num_features, self.mlp_ratio = embed_dim, mlp_ratio
        norm = norm_layer if patch_norm else None
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=embed_dim, embed_dim=embed_dim,
                                      norm_layer=norm)
        self.patches_resolution = res = self.patch_embed.patches_resolution
        self.patch_unembed = PatchUnEmbed(img_size=img_size, patch_size=patch_size, in_chans=embed_dim,
                                          embed_dim=embed_dim, norm_layer=norm)
        if ape:
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches, embed_dim))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=0.02)
        self.pos_drop = nn.Dropout(p=drop_rate)
        rates = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]     # stochastic depth grows with depth
        self.layers = nn.ModuleList()
        for i, depth in enumerate(depths):
            first = sum(depths[:i])
            self.layers.append(RSTB(dim=embed_dim, input_resolution=(res[0], res[1]), depth=depth,
                                    num_heads=num_heads[i], window_size=window_size, mlp_ratio=mlp_ratio,
                                    qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                                    drop_path=rates[first:first + depth], norm_layer=norm_layer, downsample=None,
                                    use_checkpoint=use_checkpoint, img_size=img_size, patch_size=patch_size,
                                    resi_connection=resi_connection, fused=fused))
        self.norm = norm_layer(self.num_features)
        conv = _residual_conv(embed_dim, resi_connection)
        if conv is not None:
            self.conv_after_body = conv

        if upsampler == "pixelshuffle":                       # classical SR
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.upsample = Upsample(upscale, num_feat)
            self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        elif upsampler == "pixelshuffledirect":               # lightweight SR
            self.upsample = UpsampleOneStep(upscale, embed_dim, num_out_ch, (res[0], res[1]))
        elif upsampler == "nearest+conv":                     # real-world SR
            assert upscale == 4, "only support x4 now."
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
            self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        else:
            self.conv_last = nn.Conv2d(embed_dim, num_out_ch, 3, 1, 1)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"absolute_pos_embed"}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {"relative_position_bias_table"}

    def check_image_size(self, x):
        """Mirror the image past its bottom and right edges up to the next multiple of the window (a whole window more
        where it already is one, as the reference does)."""
        _, _, h, w = x.size()
        ws = self.window_size
        x = torch.cat([x, torch.flip(x, [2])], 2)[:, :, :(h // ws + 1) * ws, :]
        return torch.cat([x, torch.flip(x, [3])], 3)[:, :, :, :(w // ws + 1) * ws]

    def forward_features(self, x):
        x_size = (x.shape[2], x.shape[3])
        x = self.patch_embed(x)
        if self.ape:
            x = x + self.absolute_pos_embed
        x = self.pos_drop(x)
        for layer in self.layers:
            x = layer(x, x_size)
        return self.patch_unembed(self.norm(x), x_size)

    def forward(self, x):
        _, _, h, w = x.size()
        x = self.check_image_size(x)
        self.mean = self.mean.type_as(x)
        x = (x - self.mean) * self.img_range
        if self.upsampler in ("pixelshuffle", "pixelshuffledirect", "nearest+conv"):
            x = self.conv_first(x)
            x = self.conv_after_body(self.forward_features(x)) + x
            if self.upsampler == "pixelshuffle":
                x = self.conv_last(self.upsample(self.conv_before_upsample(x)))
            elif self.upsampler == "pixelshuffledirect":
                x = self.upsample(x)
            else:
                x = self.conv_before_upsample(x)
                x = self.lrelu(self.conv_up1(F.interpolate(x, scale_factor=2, mode="nearest")))
                x = self.lrelu(self.conv_up2(F.interpolate(x, scale_factor=2, mode="nearest")))
                x = self.conv_last(self.lrelu(self.conv_hr(x)))
        else:
            first = self.conv_first(x)
            x = x + self.conv_last(self.conv_after_body(self.forward_features(first)) + first)
        x = x / self.img_range + self.mean
        return x[:, :, 0:h * self.upscale, 0:w * self.upscale]
