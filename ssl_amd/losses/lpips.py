"""LPIPS as a DIFFERENTIABLE term: the perceptual part of the Diffusion fork's autoencoder stage
(Diffusion-Based-SR/ldm/modules/losses/contperceptual.py, which takes `LPIPS` from taming-transformers'
taming/modules/losses/lpips.py: VGG16, five taps, v0.1's linear layers).

ssl_amd.metrics.LPIPS is a validation metric: an input that requires grad sends it to the torch lines.  Here the
criterion behind the network is an autograd node on the kernels of ssl_amd/csrc/ssg_featmetric.hip (include/ssg_hip.h
section (V)): forward `ssg_lpips_layers` (every pair read once, nothing of feature size written), backward ONE
`ssg_lpips_layers_backward` launch that writes the gradient of every map that wants one.  The node keeps the maps the
trunk's own backward keeps anyway and nothing else, where the torch lines keep 8 - 20 full-size temporaries per layer.
The backward is deterministic: `calculate_adaptive_weight`'s autograd.grad(..., retain_graph=True) and the backward()
behind it get the same bits.

Dispatch: fp32 maps on one GPU with the switch on (_gpu.native) take the kernels whether or not they require grad; CPU
tensors, fp64, half / bf16, `set_native_criteria(False)` and a `lin` that requires grad take `lpips_torch_lines` and give
its bits.  The kernels' gradient is the adjoint of the unclamped distance, formed in fp64; where a pixel's own vector is
all zero it is NaN on that side, as the torch lines' is.

taming-transformers is no dependency of this package and is not available to its tests: that `LPIPS` below IS taming's
module (ScalingLayer, torchvision's VGG16 `features` tapped behind relu1_2, relu2_2, relu3_3, relu4_3, relu5_3,
`normalize_tensor` with eps 1e-10, the squared difference, a bias-free 1x1 convolution per tap, the spatial mean, their
sum; dropout inactive under .eval()) is supposed equal, not verified.  Its state_dict keys are this package's (`lins.k`,
the trunk's layer names), not taming's (`lin{k}.model.1.weight`, `net.slice*`): a checkpoint that carries taming's keys
does not fill it; the weights come through `weights=` in either key layout (load_lpips_weights).
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _gpu
from .. import metrics_feat as _mf

__all__ = ["LPIPS", "lpips_criterion"]


class _LpipsCriterion(torch.autograd.Function):
    """out[:, K] of ssg_lpips_layers as fp32 (N,1,1,1); backward: one ssg_lpips_layers_backward launch."""

    @staticmethod
    def forward(ctx, K, *tensors):
        f0, f1, w = (_mf._maps(tensors[i * K:(i + 1) * K]) for i in range(3))
        out = _mf.lpips_layers(f0, f1, w)
        ctx.K = K
        ctx.save_for_backward(*f0, *f1, *w)
        return out[:, K].to(torch.float32).reshape(-1, 1, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        K, saved = ctx.K, ctx.saved_tensors
        f0, f1, w = saved[:K], saved[K:2 * K], saved[2 * K:]
        need0, need1 = any(ctx.needs_input_grad[1:1 + K]), any(ctx.needs_input_grad[1 + K:1 + 2 * K])
        none = (None,) * K
        if not (need0 or need1):
            return (None,) + 3 * none
        g0, g1 = _mf.lpips_layers_backward(f0, f1, w, g.to(torch.float32), need0, need1)
        return (None,) + (tuple(g0) if need0 else none) + (tuple(g1) if need1 else none) + none


def lpips_criterion(feats0, feats1, lins):
    """LPIPS behind its network, differentiable with respect to both sets of maps: (N,1,1,1), the sum over the K
    layers of the spatial mean of the 1x1 convolution `lins[k]` of the squared difference of the channel-normalised
    maps.  See the module's text for which calls take the kernels; the others are `lpips_torch_lines` itself."""
    feats0, feats1, lins = list(feats0), list(feats1), list(lins)
    if _gpu.native(*feats0, *feats1, *lins) and not any(w.requires_grad for w in lins):
        return _LpipsCriterion.apply(len(feats0), *feats0, *feats1, *lins)
    return _mf.lpips_torch_lines(feats0, feats1, lins)


class LPIPS(nn.Module):
    """LPIPS(weights=None): forward(input, target) -> (N,1,1,1) for RGB batches in [-1, 1], differentiable with respect
    to both.  weights: see ssl_amd.metrics_feat.load_lpips_weights (net 'vgg'); nothing is downloaded.  The parameters
    are frozen and the module stays in eval mode; the trunk's backward is torch's."""

    def __init__(self, weights=None):
        super().__init__()
        trunk, lins, self.weights_key = _mf.load_lpips_weights('vgg', weights)
        self.scaling_layer = _mf.ScalingLayer()
        self.net = _mf._vgg16_trunk(trunk)[1]
        self.chns = _mf.VGG_CHANNELS
        self.lins = nn.ParameterList()
        for k, (w, c) in enumerate(zip(lins, self.chns)):
            if w.numel() != c:
                raise ValueError(f"ssl_amd: lin{k}.model.1.weight has {w.numel()} elements, the layer {c} channels")
            self.lins.append(nn.Parameter(w.detach().clone().to(torch.float32).reshape(1, c, 1, 1)))
        _mf._freeze(self)

    def train(self, mode=True):
        return super().train(False)

    def features(self, x):
        return _mf._tapped(self.net, _mf.VGG_TAPS, self.scaling_layer(x))

    def forward(self, input, target):
        return lpips_criterion(self.features(input), self.features(target), list(self.lins))
