"""KAIR's VGG perceptual loss behind its own names and signatures (GAN-Based-SR/train_BSGRAN/models/loss.py:54-130, the
`F_lossfn` of model_ssl.py:162-179 with F_feature_layer [2,7,16,25,34] and F_weights [0.1,0.1,1,1,1]), on the trunk and
the one-launch criterion of ssl_amd/losses/perceptual.py.

feature_layer counts torchvision's `vgg19.features`: 2, 7, 16, 25, 34 are conv1_2, conv2_2, conv3_4, conv4_4, conv5_4,
so this class and the basicsr class give equal features from one state_dict.  PerceptualLoss keeps the attributes `.vgg`
and `.lossfn` that the model moves to its device (model_ssl.py:174-175); `.vgg` may be wrapped (DataParallel) and is
only ever called.  `.lossfn` is torch's nn.L1Loss or nn.MSELoss; it is what the fallback applies, and its type decides
the kernel's criterion, so a replaced `.lossfn` of another type is simply applied as given.
"""
import torch
from torch import nn

from . import perceptual

__all__ = ["VGGFeatureExtractor", "PerceptualLoss"]


class VGGFeatureExtractor(nn.Module):
    """VGGFeatureExtractor(feature_layer=[2,7,16,25,34], use_input_norm=True, use_range_norm=False, vgg_weights=None):
    forward(x) -> the list of the features at those indices of vgg19.features (a list argument), or the one feature
    (an int)."""

    def __init__(self, feature_layer=[2, 7, 16, 25, 34], use_input_norm=True, use_range_norm=False, vgg_weights=None):
        super().__init__()
        self.use_input_norm = use_input_norm
        self.use_range_norm = use_range_norm
        if self.use_input_norm:
            self.register_buffer('mean', torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
            self.register_buffer('std', torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self.list_outputs = isinstance(feature_layer, (list, tuple))
        names = perceptual.vgg_layer_names('vgg19')
        layers = [int(v) for v in feature_layer] if self.list_outputs else [int(feature_layer)]
        if not layers or any(not 0 <= v < len(names) for v in layers) or sorted(set(layers)) != layers:
            raise ValueError(f"feature_layer must be increasing indices of vgg19.features (0 .. {len(names) - 1}), got "
                             f"{feature_layer!r}")
        self.taps = [names[v] for v in layers]
        self.features = perceptual.build_vgg_trunk(names, set(self.taps), layers[-1],
                                                   perceptual.load_vgg_state_dict(vgg_weights))
        self.features.eval()
        for v in self.features.parameters():     # no need to BP to variable
            v.requires_grad = False

    def forward(self, x):
        if self.use_range_norm:
            x = (x + 1.0) / 2.0
        if self.use_input_norm:
            x = (x - self.mean) / self.std
        output = []
        for key, layer in self.features._modules.items():
            x = layer(x)
            if key in self.taps:
                output.append(x)
        return output if self.list_outputs else output[0]


class PerceptualLoss(nn.Module):
    """PerceptualLoss(feature_layer=[2,7,16,25,34], weights=[0.1,0.1,1.0,1.0,1.0], lossfn_type='l1',
    use_input_norm=True, use_range_norm=False, vgg_weights=None): forward(x, gt) -> sum_i weights[i] *
    lossfn(vgg(x)[i], vgg(gt)[i]) (a list feature_layer) or lossfn(vgg(x), vgg(gt)) (an int)."""

    def __init__(self, feature_layer=[2, 7, 16, 25, 34], weights=[0.1, 0.1, 1.0, 1.0, 1.0], lossfn_type='l1',
                 use_input_norm=True, use_range_norm=False, vgg_weights=None):
        super().__init__()
        self.vgg = VGGFeatureExtractor(feature_layer=feature_layer, use_input_norm=use_input_norm,
                                       use_range_norm=use_range_norm, vgg_weights=vgg_weights)
        self.lossfn_type = lossfn_type
        self.weights = weights
        self.lossfn = nn.L1Loss() if self.lossfn_type == 'l1' else nn.MSELoss()

    def _kind(self):
        """the kernel's criterion for `.lossfn`, None for a module that is neither of torch's two mean criteria"""
        fn = self.lossfn
        if type(fn) is nn.L1Loss and fn.reduction == 'mean':
            return 'l1'
        if type(fn) is nn.MSELoss and fn.reduction == 'mean':
            return 'mse'
        return None

    def forward(self, x, gt):
        x_vgg, gt_vgg = self.vgg(x), self.vgg(gt.detach())
        kind = self._kind()
        if isinstance(x_vgg, list):
            if kind is not None:
                return perceptual.multi_criterion(x_vgg, gt_vgg, self.weights[:len(x_vgg)], kind)
            loss = 0.0
            for i in range(len(x_vgg)):
                loss += self.weights[i] * self.lossfn(x_vgg[i], gt_vgg[i])
            return loss
        if kind is not None:
            return perceptual.multi_criterion([x_vgg], [gt_vgg.detach()], [1.0], kind)
        return 0.0 + self.lossfn(x_vgg, gt_vgg.detach())
