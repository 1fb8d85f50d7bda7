"""LPIPS and DISTS, the two feature-space validation metrics of the reference's `val.metrics` blocks
(GAN-Based-SR/basicsr/metrics/lpips.py, dists.py), re-exported from ssl_amd.metrics.

The networks stay on torch and are built here from plain torch.nn layers: AlexNet's or VGG16's `features` for LPIPS
v0.1, VGG16 with `L2pooling` for DISTS.  Neither torchvision nor the `lpips` / `DISTS_pytorch` packages are needed and
nothing is ever downloaded; the weights come from a state_dict, a file, an environment variable or the files of an
installed package (`load_lpips_weights`, `load_dists_weights`).

What follows each network -- a criterion over five or six feature pairs of very different sizes -- is ONE call of
ssl_amd/csrc/ssg_featmetric.hip (include/ssg_hip.h section (V)): every pair is read once, nothing of feature size is
written, where the packages run 8 - 20 torch operations per layer with full-size temporaries.

Dispatch: fp32 GPU feature maps none of which requires a gradient take the kernels (no gradient flows through them);
CPU tensors, fp64, half / bf16, an input that requires grad and `set_native_criteria(False)` take the packages' torch
lines (`lpips_torch_lines`, `dists_torch_lines`) and give their bits.  LPIPS as a differentiable loss term is
ssl_amd/losses/lpips.py, on `lpips_layers` and its adjoint `lpips_layers_backward` below.

Differences from the reference's two functions, both where its own line cannot run: `crop_border=0` means no crop
(its `[0:-0]` slice is an empty tensor), and `calculate_lpips(test_y_channel=True)` is refused (it would feed one
channel to a three-channel convolution)."""
import importlib.util
import os
import re
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._gpu import address_array, launch as _launch, native, ptr as _ptr, readable, workspace as _workspace
from .losses.perceptual import build_vgg_trunk, vgg_layer_names

__all__ = ["LPIPS", "DISTS", "L2pooling", "ScalingLayer", "calculate_lpips", "calculate_dists", "lpips_dists",
           "lpips_layers", "lpips_layers_backward", "dists_score", "lpips_torch_lines", "dists_torch_lines", "load_lpips_weights",
           "load_dists_weights", "LPIPS_WEIGHTS_ENV", "DISTS_WEIGHTS_ENV"]

LPIPS_WEIGHTS_ENV = "SSL_AMD_LPIPS_WEIGHTS"
DISTS_WEIGHTS_ENV = "SSL_AMD_DISTS_WEIGHTS"
MAX_LAYERS = 16

ALEX_NAMES = ('conv1', 'relu1', 'pool1', 'conv2', 'relu2', 'pool2', 'conv3', 'relu3', 'conv4', 'relu4', 'conv5', 'relu5')
ALEX_TAPS = ('relu1', 'relu2', 'relu3', 'relu4', 'relu5')
ALEX_CHANNELS = (64, 192, 384, 256, 256)
# (in, out, kernel, stride, padding) of torchvision's AlexNet `features`
_ALEX_CONVS = {'conv1': (3, 64, 11, 4, 2), 'conv2': (64, 192, 5, 1, 2), 'conv3': (192, 384, 3, 1, 1),
               'conv4': (384, 256, 3, 1, 1), 'conv5': (256, 256, 3, 1, 1)}
VGG_TAPS = ('relu1_2', 'relu2_2', 'relu3_3', 'relu4_3', 'relu5_3')
VGG_CHANNELS = (64, 128, 256, 512, 512)
DISTS_CHANNELS = (3,) + VGG_CHANNELS
# the hub cache's file names of torchvision's own checkpoints (looked for, never fetched)
_TRUNK_FILES = {'alex': 'alexnet-', 'vgg': 'vgg16-'}


# ------------------------------------------------------------------------------------------------- the criteria ---
def _normalize_tensor(in_feat, eps=1e-10):
    norm_factor = torch.sqrt(torch.sum(in_feat ** 2, dim=1, keepdim=True))
    return in_feat / (norm_factor + eps)


def lpips_torch_lines(feats0, feats1, lins):
    """The package's lines behind its network: (N,1,1,1), the sum over the layers of the spatial mean of the 1x1
    convolution `lins[k]` ((1,C,1,1)) of the squared difference of the channel-normalised maps."""
    val = 0
    for f0, f1, w in zip(feats0, feats1, lins):
        diff = (_normalize_tensor(f0) - _normalize_tensor(f1)) ** 2
        val = val + F.conv2d(diff, w).mean([2, 3], keepdim=True)
    return val


def dists_torch_lines(feats0, feats1, alpha, beta):
    """The package's lines behind its network: (N,), from alpha and beta of shape (1, sum C, 1, 1)."""
    chns = [f.shape[1] for f in feats0]
    dist1 = 0
    dist2 = 0
    c1 = 1e-6
    c2 = 1e-6
    w_sum = alpha.sum() + beta.sum()
    alphas = torch.split(alpha / w_sum, chns, dim=1)
    betas = torch.split(beta / w_sum, chns, dim=1)
    for k in range(len(chns)):
        x_mean = feats0[k].mean([2, 3], keepdim=True)
        y_mean = feats1[k].mean([2, 3], keepdim=True)
        S1 = (2 * x_mean * y_mean + c1) / (x_mean ** 2 + y_mean ** 2 + c1)
        dist1 = dist1 + (alphas[k] * S1).sum(1, keepdim=True)
        x_var = ((feats0[k] - x_mean) ** 2).mean([2, 3], keepdim=True)
        y_var = ((feats1[k] - y_mean) ** 2).mean([2, 3], keepdim=True)
        xy_cov = (feats0[k] * feats1[k]).mean([2, 3], keepdim=True) - x_mean * y_mean
        S2 = (2 * xy_cov + c2) / (x_var + y_var + c2)
        dist2 = dist2 + (betas[k] * S2).sum(1, keepdim=True)
    return 1 - (dist1 + dist2).reshape(-1)


def features_are_native(*tensors):
    """Whether a module's call takes the kernels: the package's rule (_gpu.native: the switch, fp32 tensors on one GPU)
    and none requiring grad (no gradient flows through the kernels)."""
    return native(*tensors) and not any(t.requires_grad for t in tensors)


def _refuse_unreadable(name, *tensors):
    if not readable(*tensors):
        seen = sorted({f"{t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__ for t in tensors})
        raise ValueError(f"ssl_amd: {name} takes fp32 tensors on one GPU (the kernels read their memory as floats), got "
                         f"{', '.join(seen)}; the packages' torch lines ({name.split('_')[0]}_torch_lines) take anything")


def _shapes(name, a, b):
    K = len(a)
    if K < 1 or K > MAX_LAYERS or len(b) != K:
        raise ValueError(f"ssl_amd: {name} takes 1 .. {MAX_LAYERS} feature pairs, got {K} and {len(b)}")
    N = a[0].shape[0]
    for x, y in zip(a, b):
        if x.dim() != 4 or x.shape != y.shape or x.shape[0] != N or x.numel() == 0:
            raise ValueError(f"ssl_amd: {name} takes pairs of non-empty (N,C,H,W) maps of one shape and one N, got "
                             f"{tuple(x.shape)} and {tuple(y.shape)}")
    dims = [np.ascontiguousarray([t.shape[i] for t in a], dtype=np.int32) for i in (1, 2, 3)]
    return K, N, dims


def _maps(ts):
    return [t.detach().contiguous() for t in ts]


def lpips_layers(feats0, feats1, lins):
    """ssg_lpips_layers on K feature pairs (fp32 GPU (N,C_k,H_k,W_k)) and their 1x1 convolutions (C_k floats each, any
    shape): a device (N, K + 1) float64 tensor, [n, k] the layer's spatial mean, [n, K] their sum in layer order.  Two
    launches on the current stream, no host synchronisation."""
    feats0, feats1, lins = list(feats0), list(feats1), list(lins)
    _refuse_unreadable("lpips_layers", *feats0, *feats1, *lins)
    K, N, (C, H, W) = _shapes("lpips_layers", feats0, feats1)
    f0, f1 = _maps(feats0), _maps(feats1)
    w = [t.detach().contiguous().reshape(-1) for t in lins]
    if len(w) != K or any(t.numel() != c for t, c in zip(w, C)):
        raise ValueError("ssl_amd: lpips_layers takes one weight of C_k elements per layer")
    dev = f0[0].device
    L = _lib.lib()
    out = torch.empty((N, K + 1), dtype=torch.float64, device=dev)
    ws, nb = _workspace(L.ssg_lpips_workspace_bytes(K, N, C.ctypes.data, H.ctypes.data, W.ctypes.data), dev)
    a0, a1, aw = (address_array([t.data_ptr() for t in ts]) for ts in (f0, f1, w))
    _launch(dev, L.ssg_lpips_layers, K, N, a0.ctypes.data, a1.ctypes.data, aw.ctypes.data, C.ctypes.data, H.ctypes.data,
            W.ctypes.data, _ptr(ws), nb, _ptr(out))
    return out


def lpips_layers_backward(feats0, feats1, lins, coef, need0=True, need1=True):
    """ssg_lpips_layers_backward: the gradients of sum_n coef[n] * lpips_layers(...)[n, K] with respect to the maps of
    the sides that are needed, as (grads0, grads1), each a list of K fp32 tensors shaped as its maps or None.  coef: N
    fp32 values on the maps' GPU, any shape.  ONE launch on the current stream, no workspace, no host synchronisation.
    It is the adjoint of the unclamped per-pixel distance; a pixel whose own vector is all zero gets NaN on that side
    (what torch's autograd gives there)."""
    feats0, feats1, lins = list(feats0), list(feats1), list(lins)
    _refuse_unreadable("lpips_layers_backward", *feats0, *feats1, *lins, coef)
    K, N, (C, H, W) = _shapes("lpips_layers_backward", feats0, feats1)
    if not (need0 or need1):
        raise ValueError("ssl_amd: lpips_layers_backward writes the gradient of at least one side")
    f0, f1 = _maps(feats0), _maps(feats1)
    w = [t.detach().contiguous().reshape(-1) for t in lins]
    if len(w) != K or any(t.numel() != c for t, c in zip(w, C)):
        raise ValueError("ssl_amd: lpips_layers_backward takes one weight of C_k elements per layer")
    coef = coef.detach().contiguous().reshape(-1)
    if coef.numel() != N:
        raise ValueError(f"ssl_amd: lpips_layers_backward takes one coefficient per image, got {coef.numel()} for {N}")
    dev = f0[0].device
    g0 = [torch.empty_like(t) for t in f0] if need0 else None
    g1 = [torch.empty_like(t) for t in f1] if need1 else None
    a0, a1, aw = (address_array([t.data_ptr() for t in ts]) for ts in (f0, f1, w))
    b0, b1 = (None if ts is None else address_array([t.data_ptr() for t in ts]) for ts in (g0, g1))
    _launch(dev, _lib.lib().ssg_lpips_layers_backward, K, N, a0.ctypes.data, a1.ctypes.data, aw.ctypes.data, C.ctypes.data,
            H.ctypes.data, W.ctypes.data, _ptr(coef), None if b0 is None else b0.ctypes.data,
            None if b1 is None else b1.ctypes.data)
    return g0, g1


def dists_score(feats0, feats1, alpha, beta):
    """ssg_dists_score on K feature pairs and alpha, beta (sum C_k floats each, any shape): a device (N, 3) float64
    tensor {score, the structure share, the texture share}.  Two launches on the current stream, no host
    synchronisation."""
    feats0, feats1 = list(feats0), list(feats1)
    _refuse_unreadable("dists_score", *feats0, *feats1, alpha, beta)
    K, N, (C, H, W) = _shapes("dists_score", feats0, feats1)
    x, y = _maps(feats0), _maps(feats1)
    a, b = alpha.detach().contiguous().reshape(-1), beta.detach().contiguous().reshape(-1)
    if a.numel() != int(C.sum()) or b.numel() != int(C.sum()):
        raise ValueError(f"ssl_amd: dists_score takes alpha and beta of {int(C.sum())} elements, got {a.numel()} and "
                         f"{b.numel()}")
    dev = x[0].device
    L = _lib.lib()
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    ws, nb = _workspace(L.ssg_dists_workspace_bytes(K, N, C.ctypes.data, H.ctypes.data, W.ctypes.data), dev)
    ax, ay = (address_array([t.data_ptr() for t in ts]) for ts in (x, y))
    _launch(dev, L.ssg_dists_score, K, N, ax.ctypes.data, ay.ctypes.data, C.ctypes.data, H.ctypes.data, W.ctypes.data,
            _ptr(a), _ptr(b), _ptr(ws), nb, _ptr(out))
    return out


# ------------------------------------------------------------------------------------------------- the weights ---
def _load_file(path):
    return torch.load(path, map_location='cpu', weights_only=True)


def _hub_trunk(net):
    """torchvision's own checkpoint where an earlier download left it (torch.hub's cache); None if it is not there."""
    try:
        folder = os.path.join(torch.hub.get_dir(), 'checkpoints')
        for name in sorted(os.listdir(folder)):
            if name.startswith(_TRUNK_FILES[net]) and name.endswith('.pth'):
                return os.path.join(folder, name)
    except OSError:
        pass
    return None


def _package_file(package, *relative):
    try:
        spec = importlib.util.find_spec(package)            # located, never imported
    except (ImportError, ValueError):
        spec = None
    for root in (spec.submodule_search_locations or []) if spec is not None else []:
        cand = os.path.join(root, *relative)
        if os.path.exists(cand):
            return cand
    return None


def _merge(parts):
    state = {}
    for part in parts:
        state.update(part if isinstance(part, dict) else _load_file(os.fspath(part)))
    return state


def _gather(weights, env, package_file, net, what, hint):
    """One flat dict from whatever names the weights: a dict, a path, a sequence of those (the trunk and the package's
    small file), the environment variable (one path, or two joined by os.pathsep), an installed package's file beside a
    cached torchvision checkpoint.  Returns (dict, cache key)."""
    if isinstance(weights, dict):
        return weights, ('dict', id(weights))
    if isinstance(weights, (str, os.PathLike)):
        return _merge([weights]), ('file', os.path.abspath(os.fspath(weights)))
    if isinstance(weights, (tuple, list)):
        key = tuple(id(p) if isinstance(p, dict) else os.path.abspath(os.fspath(p)) for p in weights)
        return _merge(weights), ('parts',) + key
    if weights is not None:
        raise TypeError(f"ssl_amd: weights is a state_dict, a path or a sequence of those, got {type(weights)}")
    value = os.environ.get(env)
    if value:
        paths = [p for p in value.split(os.pathsep) if p]
        return _merge(paths), ('env',) + tuple(os.path.abspath(p) for p in paths)
    small, trunk = package_file(), _hub_trunk(net)
    if small and trunk:
        return _merge([trunk, small]), ('package', trunk, small)
    raise FileNotFoundError(
        f"ssl_amd: no {what} weights found.  Give them one of these ways: the weights= argument (a state_dict in the "
        f"package's own key layout ({hint}), or a torchvision trunk dict (`features.N.weight`) together with the "
        f"package's small file, as dicts or paths, alone or as a pair); the {env} environment variable (one path, or "
        f"the trunk's and the small file's joined by {os.pathsep!r}); or an installed package's weight file beside "
        f"torchvision's checkpoint in torch.hub's cache.  Nothing is downloaded.")


def _trunk_keys(state, pattern):
    """`features.N.weight` keys from whichever layout the dict has: torchvision's own, or the package's (`pattern`
    finds the layer index and the parameter name)."""
    out = {k: v for k, v in state.items() if k.startswith('features.')}
    for key, value in state.items():
        m = re.fullmatch(pattern, key)
        if m:
            out[f'features.{m.group(1)}.{m.group(2)}'] = value
    return out


def load_lpips_weights(net='alex', weights=None):
    """(trunk dict with `features.N.weight` keys, the five (1,C,1,1) lin weights, cache key) for LPIPS v0.1."""
    state, key = _gather(weights, LPIPS_WEIGHTS_ENV, lambda: _package_file('lpips', 'weights', 'v0.1', f'{net}.pth'), net,
                         f"LPIPS ({net})", "`net.slice{k}.{i}.weight`, `lin{k}.model.1.weight`")
    trunk = _trunk_keys(state, r'net\.slice\d+\.(\d+)\.(weight|bias)')
    lins = []
    for k in range(5):
        name = f'lin{k}.model.1.weight'
        if name not in state:
            raise KeyError(f"ssl_amd: the LPIPS weights have no {name!r}")
        lins.append(state[name])
    return trunk, lins, key


def load_dists_weights(weights=None):
    """(trunk dict with `features.N.weight` keys, alpha, beta, cache key) for DISTS."""
    state, key = _gather(weights, DISTS_WEIGHTS_ENV, lambda: _package_file('DISTS_pytorch', 'weights.pt'), 'vgg', "DISTS",
                         "`stage{k}.{i}.weight`, `alpha`, `beta`")
    for name in ('alpha', 'beta'):
        if name not in state:
            raise KeyError(f"ssl_amd: the DISTS weights have no {name!r}")
    return _trunk_keys(state, r'stage\d+\.(\d+)\.(weight|bias)'), state['alpha'], state['beta'], key


# ------------------------------------------------------------------------------------------------ the networks ---
class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('scale', torch.Tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, inp):
        return (inp - self.shift) / self.scale


def build_alex_trunk(state):
    """torchvision AlexNet's `features[:12]` as an nn.Sequential keyed by ALEX_NAMES (position i is `features.i`)."""
    layers = OrderedDict()
    for i, name in enumerate(ALEX_NAMES):
        if name.startswith('conv'):
            cin, cout, k, s, p = _ALEX_CONVS[name]
            layers[name] = nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p)
            for key in ('weight', 'bias'):
                src = state.get(f'features.{i}.{key}')
                if src is None:
                    raise KeyError(f"ssl_amd: the AlexNet state_dict has no 'features.{i}.{key}'")
                if tuple(src.shape) != tuple(getattr(layers[name], key).shape):
                    raise ValueError(f"ssl_amd: features.{i}.{key} has shape {tuple(src.shape)}, AlexNet's layer "
                                     f"{tuple(getattr(layers[name], key).shape)}")
                with torch.no_grad():
                    getattr(layers[name], key).copy_(src)
        elif name.startswith('relu'):
            layers[name] = nn.ReLU(inplace=True)
        else:
            layers[name] = nn.MaxPool2d(kernel_size=3, stride=2)
    return nn.Sequential(layers)


def _vgg16_trunk(state, remove_pooling=False):
    names = vgg_layer_names('vgg16')
    return names, build_vgg_trunk(names, set(VGG_TAPS), names.index(VGG_TAPS[-1]), state, remove_pooling=remove_pooling)


def _tapped(trunk, taps, x):
    out = []
    for key, layer in trunk._modules.items():
        x = layer(x)
        if key in taps:
            out.append(x)
    return out


def _freeze(module):
    module.eval()
    for p in module.parameters():
        p.requires_grad = False


class LPIPS(nn.Module):
    """LPIPS(net='alex' | 'vgg', weights=None): the package's v0.1 with its linear layers; forward(in0, in1,
    normalize=False) -> (N,1,1,1) for RGB inputs in [-1, 1] (normalize=True: in [0, 1]).  weights: see
    load_lpips_weights.  The parameters are frozen and the module stays in eval mode."""

    def __init__(self, net='alex', weights=None):
        super().__init__()
        if net not in ('alex', 'vgg'):
            raise ValueError(f"ssl_amd: LPIPS net is 'alex' or 'vgg', got {net!r}")
        trunk, lins, self.weights_key = load_lpips_weights(net, weights)
        self.pnet_type = net
        self.scaling_layer = ScalingLayer()
        if net == 'alex':
            self.net, self.taps, self.chns = build_alex_trunk(trunk), ALEX_TAPS, ALEX_CHANNELS
        else:
            self.net, self.taps, self.chns = _vgg16_trunk(trunk)[1], VGG_TAPS, VGG_CHANNELS
        self.lins = nn.ParameterList()
        for k, (w, c) in enumerate(zip(lins, self.chns)):
            if w.numel() != c:
                raise ValueError(f"ssl_amd: lin{k}.model.1.weight has {w.numel()} elements, the layer {c} channels")
            self.lins.append(nn.Parameter(w.detach().clone().to(torch.float32).reshape(1, c, 1, 1)))
        _freeze(self)

    def train(self, mode=True):
        return super().train(False)

    def features(self, x):
        return _tapped(self.net, self.taps, self.scaling_layer(x))

    def forward(self, in0, in1, normalize=False):
        if normalize:
            in0 = 2 * in0 - 1
            in1 = 2 * in1 - 1
        f0, f1 = self.features(in0), self.features(in1)
        lins = list(self.lins)
        if features_are_native(*f0, *f1, *lins):
            out = lpips_layers(f0, f1, lins)
            return out[:, -1].to(in0.dtype).reshape(-1, 1, 1, 1)
        return lpips_torch_lines(f0, f1, lins)


class L2pooling(nn.Module):
    """sqrt(depthwise 3x3 Hann filter of x^2, stride 2, padding 1, + 1e-12): DISTS's replacement of VGG's max-pools."""

    def __init__(self, filter_size=5, stride=2, channels=None, pad_off=0):
        super().__init__()
        self.padding = (filter_size - 2) // 2
        self.stride = stride
        self.channels = channels
        a = np.hanning(filter_size)[1:-1]
        g = torch.Tensor(a[:, None] * a[None, :])
        g = g / torch.sum(g)
        self.register_buffer('filter', g[None, None, :, :].repeat((self.channels, 1, 1, 1)))

    def forward(self, input):
        input = input ** 2
        out = F.conv2d(input, self.filter, stride=self.stride, padding=self.padding, groups=input.shape[1])
        # (a sum of products of non-negative numbers: the clamp changes nothing where the convolution adds them up
        # directly.  On large maps the GPU library's convolution returns values down to -1e-6, and the package's line,
        # (out + 1e-12).sqrt(), is NaN there -- measured at 64 x 2040 x 1356 and already at 64 x 512 x 1356.)
        return (out.clamp_min(0) + 1e-12).sqrt()


class DISTS(nn.Module):
    """DISTS(weights=None): forward(x, y) -> (N,) for RGB inputs in [0, 1] (x the reference image, as the package names
    them).  weights: see load_dists_weights.  The parameters are frozen and the module stays in eval mode."""

    def __init__(self, weights=None):
        super().__init__()
        trunk, alpha, beta, self.weights_key = load_dists_weights(weights)
        names, plain = _vgg16_trunk(trunk, remove_pooling=True)
        layers, width = OrderedDict(), 64
        for name in names[:names.index(VGG_TAPS[-1]) + 1]:
            if name.startswith('pool'):
                layers[name] = L2pooling(channels=width)
            else:
                layers[name] = plain._modules[name]
                if name.startswith('conv'):
                    width = layers[name].out_channels
        self.net = nn.Sequential(layers)
        self.chns = DISTS_CHANNELS
        self.register_buffer('mean', torch.tensor([0.485, 0.456, 0.406]).view(1, -1, 1, 1))
        self.register_buffer('std', torch.tensor([0.229, 0.224, 0.225]).view(1, -1, 1, 1))
        total = sum(self.chns)
        if alpha.numel() != total or beta.numel() != total:
            raise ValueError(f"ssl_amd: DISTS's alpha and beta have {total} elements, got {alpha.numel()} and "
                             f"{beta.numel()}")
        self.alpha = nn.Parameter(alpha.detach().clone().to(torch.float32).reshape(1, total, 1, 1))
        self.beta = nn.Parameter(beta.detach().clone().to(torch.float32).reshape(1, total, 1, 1))
        _freeze(self)

    def train(self, mode=True):
        return super().train(False)

    def features(self, x):
        return [x] + _tapped(self.net, VGG_TAPS, (x - self.mean) / self.std)

    def forward(self, x, y):
        f0, f1 = self.features(x), self.features(y)
        if features_are_native(*f0, *f1, self.alpha, self.beta):
            return dists_score(f0, f1, self.alpha, self.beta)[:, 0].to(x.dtype)
        return dists_torch_lines(f0, f1, self.alpha, self.beta)


# ------------------------------------------------------------------------------ the reference's two functions ---
_models = {}                            # (metric, net, device, weights source) -> module


def _device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _model(metric, net, weights, dev):
    """The network of a metric on a device, built once per weights source (the reference rebuilds it per image)."""
    if weights is None:                  # (which files the default names is decided when the network is built)
        key = ('default', os.environ.get(LPIPS_WEIGHTS_ENV if metric == 'lpips' else DISTS_WEIGHTS_ENV))
    elif isinstance(weights, (tuple, list)):
        key = tuple(id(p) if isinstance(p, dict) else os.path.abspath(os.fspath(p)) for p in weights)
    else:
        key = id(weights) if isinstance(weights, dict) else os.path.abspath(os.fspath(weights))
    full = (metric, net, str(dev), key)
    if full not in _models:
        with torch.no_grad():
            module = LPIPS(net=net, weights=weights) if metric == 'lpips' else DISTS(weights=weights)
        _models[full] = (module.to(dev), weights)          # (a dict is kept alive: its id is the key)
    return _models[full][0]


def _as_array(img):
    return img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)


def _crop(img, crop_border):
    if crop_border != 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border, ...]
    return img


def calculate_lpips(img, img2, crop_border, input_order='HWC', test_y_channel=False, **kwargs):
    """basicsr.metrics.calculate_lpips of the reference: BGR images with range [0, 255] (arrays or tensors), `net='alex'`.
    Returns a Python float.  crop_border=0 means no crop; test_y_channel=True is refused.  `lpips_weights=` names the
    weights (see load_lpips_weights), `lpips_net=` another trunk."""
    img, img2 = _as_array(img), _as_array(img2)
    assert img.shape == img2.shape, (f'Image shapes are differnet: {img.shape}, {img2.shape}.')
    if input_order not in ['HWC', 'CHW']:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are ' '"HWC" and "CHW"')
    if test_y_channel:
        raise ValueError("ssl_amd: calculate_lpips(test_y_channel=True) would feed one channel to LPIPS's three-channel "
                         "network (the reference's own line raises inside the first convolution)")
    if img.ndim != 3 or img.shape[0 if input_order == 'CHW' else 2] != 3:
        raise ValueError(f"ssl_amd: calculate_lpips takes three-channel images, got {img.shape} as {input_order}")
    dev = _device()
    tensors = []
    for a in (img2, img):                       # (ground truth first, as the reference's img2tensor call lists them)
        if input_order == 'CHW':
            a = a.transpose(1, 2, 0)
        a = _crop(a.astype(np.float64), crop_border) / 255.
        t = torch.from_numpy(np.ascontiguousarray(a[:, :, ::-1].transpose(2, 0, 1))).float()
        tensors.append(t.sub_(0.5).div_(0.5).to(dev))
    img_gt, img_restored = tensors
    model = _model('lpips', kwargs.get('lpips_net', 'alex'), kwargs.get('lpips_weights'), dev)
    with torch.no_grad():
        lpips_val = model(img_restored.unsqueeze(0), img_gt.unsqueeze(0))
    return float(lpips_val.detach().cpu().numpy().mean())


def calculate_dists(img, img2, crop_border, color_order='BGR', **kwargs):
    """basicsr.metrics.calculate_dists of the reference: (H,W,3) uint8 images (any other type is taken as already
    scaled to [0, 1], as ToTensor takes it), ground truth first in the model's call.  Returns a Python float.
    crop_border=0 means no crop.  `dists_weights=` names the weights (see load_dists_weights)."""
    dev = _device()
    tensors = []
    for a in (img, img2):
        a = _as_array(a)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"ssl_amd: calculate_dists takes (H,W,3) images, got {a.shape}")
        if color_order == 'BGR':
            a = a[:, :, ::-1]
        t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
        t = t.to(torch.float32).div(255) if t.dtype == torch.uint8 else t.to(torch.float32)
        t = t.unsqueeze(0)
        if crop_border != 0:
            t = t[:, :, crop_border:-crop_border, crop_border:-crop_border]
        tensors.append(t.contiguous().to(dev))
    a, b = tensors
    model = _model('dists', 'vgg', kwargs.get('dists_weights'), dev)
    with torch.no_grad():
        return float(model(b, a).reshape(-1)[0])


# --------------------------------------------------------------------------------------------- the batched call ---
def _model_tensors(name, sr, gt, crop_border):
    assert sr.shape == gt.shape, (f'Image shapes are different: {sr.shape}, {gt.shape}.')
    if not (torch.is_tensor(sr) and sr.is_floating_point() and torch.is_tensor(gt) and gt.is_floating_point()):
        raise TypeError(f"ssl_amd: {name} takes floating-point tensors (use calculate_lpips / calculate_dists for images)")
    if sr.dim() == 3:
        sr, gt = sr[None], gt[None]
    if sr.dim() != 4 or sr.shape[1] != 3:
        raise ValueError(f"ssl_amd: {name} takes (N,3,H,W) or (3,H,W) tensors, got {tuple(sr.shape)}")
    dev = sr.device if sr.is_cuda else _device()
    out = []
    for t in (sr, gt):
        t = t.detach().to(device=dev, dtype=torch.float32)
        t = (t.clamp(0, 1) * 255.0).round() / 255.0          # tensor2img's quantisation, back in [0, 1]
        if crop_border != 0:
            t = t[:, :, crop_border:-crop_border, crop_border:-crop_border]
        out.append(t.contiguous())
    return out[0], out[1], dev


def lpips(sr, gt, crop_border=0, lpips_weights=None, lpips_net='alex'):
    """LPIPS of float (N,3,H,W) (or (3,H,W)) RGB tensors in nominal [0, 1]: a device (N,) float64 tensor."""
    a, b, dev = _model_tensors("lpips", sr, gt, crop_border)
    model = _model('lpips', lpips_net, lpips_weights, dev)
    with torch.no_grad():
        return model((a - 0.5) / 0.5, (b - 0.5) / 0.5).reshape(-1).to(torch.float64)


def dists(sr, gt, crop_border=0, dists_weights=None):
    """DISTS of float (N,3,H,W) (or (3,H,W)) RGB tensors in nominal [0, 1]: a device (N,) float64 tensor."""
    a, b, dev = _model_tensors("dists", sr, gt, crop_border)
    model = _model('dists', 'vgg', dists_weights, dev)
    with torch.no_grad():
        return model(b, a).reshape(-1).to(torch.float64)


def lpips_dists(sr, gt, crop_border=0, lpips_weights=None, dists_weights=None, lpips_net='alex'):
    """LPIPS and DISTS of float (N,3,H,W) (or (3,H,W)) RGB tensors in nominal [0, 1], as `visuals['result']` and
    `visuals['gt']` hold them: what the reference gets from tensor2img (clamp, * 255, round, uint8) followed by
    calculate_lpips / calculate_dists, for every image of the batch.  Returns a device (N,2) float64 tensor {LPIPS,
    DISTS}; runs on the current stream without synchronising with the host (once the networks are on the device)."""
    return torch.stack([lpips(sr, gt, crop_border, lpips_weights, lpips_net), dists(sr, gt, crop_border, dists_weights)], 1)


FEATURE_METRICS = {"calculate_lpips": lpips, "calculate_dists": dists}
WEIGHT_OPTIONS = ("lpips_weights", "dists_weights")
_OWN_OPTIONS = {"calculate_lpips": ("lpips_weights", "lpips_net"), "calculate_dists": ("dists_weights",)}


def batched(metric_type, sr, gt, opt):
    """(N,) device float64 values of one of the two metrics on a model's tensors, from a YAML entry's options."""
    if metric_type == "calculate_lpips" and opt.get('test_y_channel', False):
        raise ValueError("ssl_amd: calculate_lpips(test_y_channel=True) would feed one channel to LPIPS's three-channel "
                         "network")
    own = {k: opt[k] for k in _OWN_OPTIONS[metric_type] if k in opt}
    return FEATURE_METRICS[metric_type](sr, gt, int(opt.get('crop_border', 0)), **own)
