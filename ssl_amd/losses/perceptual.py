"""The VGG perceptual (and style) loss behind the reference's names: GAN-Based-SR/basicsr/archs/vgg_arch.py
(VGGFeatureExtractor) and basicsr/losses/basic_loss.py:160-266 (PerceptualLoss), the `type: PerceptualLoss` of every
options/train/*SSL/*.yml.  KAIR's pair (train_BSGRAN/models/loss.py:54-130) is in ssl_amd/losses/kair.py, on the trunk
built here.

The network stays on torch: plain torch.nn layers, named from VGG's block structure, filled from a torchvision-format
state_dict (`features.N.weight`).  torchvision is not needed and nothing is ever downloaded.  What follows the network --
the criterion over the K tapped feature pairs, five tensors whose sizes span 32 : 1 -- is ONE call of
engine.multi_pixel_loss (ssl_amd/csrc/ssg_mcrit.hip, include/ssg_hip.h section (U)): one launch over the chunks of all
pairs and a fold, and one launch for all K gradients, where the reference runs sub, abs, mean, mul, add per layer and
their backward.  The style term forms its Gram matrices with torch.bmm and takes the same single call over the K Gram
pairs.

Dispatch: fp32 GPU feature pairs of equal shape and equal dense strides (contiguous or channels_last) whose target
wants no gradient take the kernels; everything else -- CPU tensors, fp64, half precision, mismatched strides, an empty
tensor, `set_native_criteria(False)` -- takes the reference's torch expression, `criterion(x_k, gt_k) * w_k` summed in
layer order, and gives its bits.

criterion 'l2': the reference constructs `torch.nn.L2loss()`, which does not exist (AttributeError).  Here 'l2' is the
mean squared error, torch.nn.MSELoss.
"""
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from .. import _gpu, engine

__all__ = ["VGGFeatureExtractor", "PerceptualLoss", "vgg_layer_names", "multi_criterion", "VGG_PRETRAIN_PATH",
           "VGG_WEIGHTS_ENV"]

VGG_PRETRAIN_PATH = 'experiments/pretrained_models/vgg19-dcbb9e9d.pth'   # (the reference's, relative to the run's cwd)
VGG_WEIGHTS_ENV = 'SSL_AMD_VGG_WEIGHTS'

# convolutions per block; the widths of the five blocks
_BLOCKS = {'vgg11': (1, 1, 2, 2, 2), 'vgg13': (2, 2, 2, 2, 2), 'vgg16': (2, 2, 3, 3, 3), 'vgg19': (2, 2, 4, 4, 4)}
_WIDTHS = (64, 128, 256, 512, 512)
_CRITERIA = {'l1': 'l1', 'l2': 'mse', 'fro': 'fro'}


def _split_type(vgg_type):
    base = vgg_type[:-3] if vgg_type.endswith('_bn') else vgg_type
    if base not in _BLOCKS:
        raise ValueError(f"Unsupported vgg_type: {vgg_type}. Supported ones are: "
                         f"{sorted(_BLOCKS) + [k + '_bn' for k in sorted(_BLOCKS)]}")
    return base, vgg_type.endswith('_bn')


def vgg_layer_names(vgg_type):
    """The names of torchvision's `features` of a VGG, in order: position i of the list is `features.i`."""
    base, bn = _split_type(vgg_type)
    names = []
    for block, convs in enumerate(_BLOCKS[base], 1):
        for j in range(1, convs + 1):
            names.append(f'conv{block}_{j}')
            if bn:
                names.append(f'bn{block}_{j}')
            names.append(f'relu{block}_{j}')
        names.append(f'pool{block}')
    return names


def _width_of(name):
    return _WIDTHS[int(name.lstrip('convbn').split('_')[0]) - 1]


def load_vgg_state_dict(vgg_weights=None):
    """The torchvision-format state_dict: `vgg_weights` (a dict, or a path for torch.load), else the file the
    SSL_AMD_VGG_WEIGHTS variable names, else the reference's experiments/pretrained_models/vgg19-dcbb9e9d.pth.
    Nothing is downloaded."""
    if isinstance(vgg_weights, dict):
        return vgg_weights
    tried = []
    for source, path in (("vgg_weights=", vgg_weights), (VGG_WEIGHTS_ENV, os.environ.get(VGG_WEIGHTS_ENV)),
                         ("the reference's path", VGG_PRETRAIN_PATH)):
        if not path:
            continue
        if os.path.exists(path):
            return torch.load(path, map_location='cpu', weights_only=True)
        tried.append(f"{source} {path!r}")
        if source == "vgg_weights=":
            break                               # a path that was asked for and is missing is an error, not a hint
    raise FileNotFoundError(
        "ssl_amd: no VGG weights found" + (f" (tried {', '.join(tried)})" if tried else "") + ".  Give them one of three "
        "ways: the vgg_weights= argument (a torchvision-format state_dict with `features.N.weight` keys, or the path of "
        f"one), the {VGG_WEIGHTS_ENV} environment variable (a path), or the file {VGG_PRETRAIN_PATH} under the working "
        "directory.  Nothing is downloaded.")


def _fill(module, state, index, keys):
    for key in keys:
        name = f'features.{index}.{key}'
        if name not in state:
            raise KeyError(f"ssl_amd: the VGG state_dict has no {name!r}")
        dst, src = getattr(module, key), state[name]
        if tuple(dst.shape) != tuple(src.shape):
            raise ValueError(f"ssl_amd: {name} has shape {tuple(src.shape)}, the network's layer {tuple(dst.shape)}: the "
                             "weights belong to another vgg_type")
        with torch.no_grad():
            dst.copy_(src)


def build_vgg_trunk(names, taps, last, state, remove_pooling=False, pooling_stride=2):
    """`features[:last + 1]` of the VGG whose layer names are `names` as an nn.Sequential keyed by those names and
    filled from `state`.  The ReLU behind a tapped layer is out of place, so a tapped feature is never overwritten and
    needs no clone; every other ReLU works in place as torchvision's do."""
    layers, width = OrderedDict(), 3
    for i, name in enumerate(names[:last + 1]):
        if name.startswith('conv'):
            layers[name] = nn.Conv2d(width, _width_of(name), kernel_size=3, padding=1)
            _fill(layers[name], state, i, ('weight', 'bias'))
            width = _width_of(name)
        elif name.startswith('bn'):
            layers[name] = nn.BatchNorm2d(width)
            _fill(layers[name], state, i, ('weight', 'bias', 'running_mean', 'running_var'))
        elif name.startswith('relu'):
            layers[name] = nn.ReLU(inplace=names[i - 1] not in taps)
        elif not remove_pooling:
            layers[name] = nn.MaxPool2d(kernel_size=2, stride=pooling_stride)
    return nn.Sequential(layers)


class VGGFeatureExtractor(nn.Module):
    """VGGFeatureExtractor(layer_name_list, vgg_type='vgg19', use_input_norm=True, range_norm=False,
    requires_grad=False, remove_pooling=False, pooling_stride=2, vgg_weights=None): forward(x) -> {name: feature} for
    the names of layer_name_list, in network order (vgg_arch.py:55-161).  Only the layers up to the last tapped one
    exist.  vgg_weights: see load_vgg_state_dict."""

    def __init__(self, layer_name_list, vgg_type='vgg19', use_input_norm=True, range_norm=False, requires_grad=False,
                 remove_pooling=False, pooling_stride=2, vgg_weights=None):
        super().__init__()
        self.layer_name_list = layer_name_list
        self.use_input_norm = use_input_norm
        self.range_norm = range_norm
        self.names = vgg_layer_names(vgg_type)
        for v in layer_name_list:
            if v not in self.names:
                raise ValueError(f"{v!r} is not a layer of {vgg_type}: {self.names}")
        last = max(self.names.index(v) for v in layer_name_list)
        self.vgg_net = build_vgg_trunk(self.names, set(layer_name_list), last, load_vgg_state_dict(vgg_weights),
                                       remove_pooling, pooling_stride)
        self.vgg_net.train(bool(requires_grad))
        for param in self.parameters():
            param.requires_grad = bool(requires_grad)
        if self.use_input_norm:
            # for images in [0, 1]
            self.register_buffer('mean', torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
            self.register_buffer('std', torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    def train(self, mode=True):
        # (the frozen network stays in eval mode, as the reference leaves it: its constructor's eval() is the last word
        # only until the owning model calls train())
        super().train(mode)
        if not any(p.requires_grad for p in self.vgg_net.parameters()):
            self.vgg_net.eval()
        return self

    def forward(self, x):
        if self.range_norm:
            x = (x + 1) / 2
        if self.use_input_norm:
            x = (x - self.mean) / self.std
        output = {}
        for key, layer in self.vgg_net._modules.items():
            x = layer(x)
            if key in self.layer_name_list:
                output[key] = x
        return output


def _reference_term(kind, x, g):
    if kind == 'l1':
        return F.l1_loss(x, g)
    if kind == 'mse':
        return F.mse_loss(x, g)
    return torch.norm(x - g, p='fro')


def multi_criterion(preds, targets, weights, kind='l1', scale=1.0):
    """scale * sum_k criterion(preds[k], targets[k]) * weights[k], kind 'l1' | 'mse' (both means) | 'fro': one
    engine.multi_pixel_loss call with the weights scale * weights[k] where every pair can take the kernels, the
    reference's loop of torch operations and its closing product (and their bits) otherwise."""
    preds, targets = list(preds), list(targets)
    if preds and _gpu.native_criteria() and all(
            engine.multi_pair_is_native(p, t) and not t.requires_grad and p.device == preds[0].device
            for p, t in zip(preds, targets)):
        return engine.multi_pixel_loss(preds, targets, [float(w) * float(scale) for w in weights], kind)
    loss = 0
    for p, t, w in zip(preds, targets, weights):
        loss += _reference_term(kind, p, t) * w
    return loss * scale


def gram_mat(x):
    """The (n, c, c) Gram matrix of a (n, c, h, w) feature, divided by c h w (basic_loss.py:253-266)."""
    n, c, h, w = x.size()
    features = x.reshape(n, c, w * h)
    return features.bmm(features.transpose(1, 2)) / (c * h * w)


class PerceptualLoss(nn.Module):
    """PerceptualLoss(layer_weights, vgg_type='vgg19', use_input_norm=True, range_norm=False, perceptual_weight=1.0,
    style_weight=0., criterion='l1', vgg_weights=None): forward(x, gt) -> (percep, style), either None where its
    weight is not positive (basic_loss.py:160-266).  criterion 'l1' | 'l2' (MSE; the reference raises AttributeError
    here) | 'fro'."""

    def __init__(self, layer_weights, vgg_type='vgg19', use_input_norm=True, range_norm=False, perceptual_weight=1.0,
                 style_weight=0., criterion='l1', vgg_weights=None):
        super().__init__()
        if criterion not in _CRITERIA:
            raise NotImplementedError(f'{criterion} criterion has not been supported.')
        self.perceptual_weight = perceptual_weight
        self.style_weight = style_weight
        self.layer_weights = layer_weights
        self.vgg = VGGFeatureExtractor(layer_name_list=list(layer_weights.keys()), vgg_type=vgg_type,
                                       use_input_norm=use_input_norm, range_norm=range_norm, vgg_weights=vgg_weights)
        self.criterion_type = criterion

    def _term(self, xs, gs, keys, weight):
        return multi_criterion(xs, gs, [self.layer_weights[k] for k in keys], _CRITERIA[self.criterion_type], weight)

    def forward(self, x, gt):
        x_features = self.vgg(x)
        gt_features = self.vgg(gt.detach())
        keys = list(x_features.keys())
        percep_loss = style_loss = None
        if self.perceptual_weight > 0:
            percep_loss = self._term([x_features[k] for k in keys], [gt_features[k] for k in keys], keys,
                                     self.perceptual_weight)
        if self.style_weight > 0:
            style_loss = self._term([gram_mat(x_features[k]) for k in keys], [gram_mat(gt_features[k]) for k in keys],
                                    keys, self.style_weight)
        return percep_loss, style_loss

    _gram_mat = staticmethod(gram_mat)
