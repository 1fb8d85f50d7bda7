"""SPSR's gradient map and its gradient-space pixel losses behind the reference's names, on the kernels of
ssl_amd/csrc/ssg_spsr.hip (include/ssg_hip.h section (R)).

Get_gradient / Get_gradient_nopadding mirror GAN-Based-SR/basicsr/models/spsrssl_model.py:18-84 (the two are the same
arithmetic there: both pad by 1), as parameter-free modules that stay on no device of their own and take any number of
channels.  MSELoss / CharbonnierLoss mirror basicsr/losses/basic_loss.py:69-128.  GradientLoss is the model's two lines
`cri_pix_gradSR(G(output), G(gt))` (:363) and `cri_pix_gradBranch(branch, G(gt))` (:368) as one fused call each; the
reference has no name for them.

Dispatch ("Which calls take the kernels"): fp32 tensors of one shape on one GPU, a target that wants no
gradient, no element-wise weight and a 'mean' or 'sum' reduction take the kernels; everything else -- CPU tensors, other
dtypes, `weight=`, 'none', a target that requires grad, `set_native_criteria(False)` -- takes the torch expressions
below, which are the reference's operations and give its bits.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import _gpu, engine
from . import basic_loss
from .basic_loss import _check_reduction, weight_reduce_loss as _torch_criterion

__all__ = ["Get_gradient", "Get_gradient_nopadding", "GradientLoss", "MSELoss", "CharbonnierLoss"]


def _torch_map(x):
    """The map in torch operations, plane by plane as the reference forms it: two 3 x 3 correlations with one -1 and one
    +1 each under a zero padding of 1, then sqrt(v^2 + h^2 + 1e-6).  Any device and dtype, twice differentiable."""
    kv = x.new_tensor([[0, -1, 0], [0, 0, 0], [0, 1, 0]]).reshape(1, 1, 3, 3)
    kh = x.new_tensor([[0, 0, 0], [-1, 0, 1], [0, 0, 0]]).reshape(1, 1, 3, 3)
    planes = []
    for c in range(x.shape[1]):
        p = x[:, c].unsqueeze(1)
        v, h = F.conv2d(p, kv, padding=1), F.conv2d(p, kh, padding=1)
        planes.append(torch.sqrt(torch.pow(v, 2) + torch.pow(h, 2) + 1e-6))
    return torch.cat(planes, dim=1)


class Get_gradient(nn.Module):
    """forward(x): the gradient map of a (B,C,H,W) batch (spsrssl_model.py:18-50), any C."""

    def forward(self, x):
        native = _gpu.native(x) and x.dim() == 4 and x.numel() > 0
        return engine.gradient_map(x) if native else _torch_map(x)


class Get_gradient_nopadding(Get_gradient):
    """The reference's second name for the same arithmetic (spsrssl_model.py:52-84: it pads by 1 as well)."""


class _PixelCriterion(nn.Module):
    kind = None

    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        _check_reduction(reduction)
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.eps = 1e-12

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is None and self.reduction in ('mean', 'sum') and basic_loss._native_pair(pred, target):
            return engine.pixel_loss(pred, target, self.kind, self.eps, self.loss_weight, self.reduction)
        return _torch_criterion(self.kind, pred, target, weight, self.eps, self.loss_weight, self.reduction)


class MSELoss(_PixelCriterion):
    """loss_weight * MSE(pred, target) with 'none' | 'mean' | 'sum' reduction and an optional element-wise weight
    (basic_loss.py:69-94)."""
    kind = 'mse'


class CharbonnierLoss(_PixelCriterion):
    """loss_weight * sqrt((pred - target)^2 + eps) under the same reductions (basic_loss.py:97-128)."""
    kind = 'charbonnier'

    def __init__(self, loss_weight=1.0, reduction='mean', eps=1e-12):
        super().__init__(loss_weight, reduction)
        self.eps = eps


class GradientLoss(nn.Module):
    """GradientLoss(criterion='mse' | 'l1' | 'charbonnier', loss_weight=1.0, reduction='mean', eps=1e-12).

    forward(sr, gt, return_map=False): loss_weight * criterion(G(sr), G(gt)) with G the gradient map, in one pass over
    sr and gt that stores neither map; return_map=True returns (loss, G(sr)) -- the gradient discriminator's input --
    and one backward launch carries the gradient of both.
    branch(branch, gt): loss_weight * criterion(branch, G(gt)), the gradient going to `branch` only."""

    def __init__(self, criterion='mse', loss_weight=1.0, reduction='mean', eps=1e-12):
        super().__init__()
        if criterion not in engine.PIXEL_KINDS:
            raise ValueError(f'Unsupported criterion: {criterion}. Supported ones are: {sorted(engine.PIXEL_KINDS)}')
        _check_reduction(reduction)
        self.criterion, self.loss_weight, self.reduction, self.eps = criterion, loss_weight, reduction, eps

    def _fused(self, a, b):
        return self.reduction in ('mean', 'sum') and a.dim() == 4 and basic_loss._native_pair(a, b)

    def forward(self, sr, gt, return_map=False):
        if self._fused(sr, gt):
            return engine.gradient_loss(sr, gt, self.criterion, self.eps, self.loss_weight, self.reduction, return_map)
        m = _torch_map(sr)
        loss = _torch_criterion(self.criterion, m, _torch_map(gt), None, self.eps, self.loss_weight, self.reduction)
        return (loss, m) if return_map else loss

    def branch(self, branch, gt):
        if self._fused(branch, gt):
            return engine.gradient_branch_loss(branch, gt, self.criterion, self.eps, self.loss_weight, self.reduction)
        return _torch_criterion(self.criterion, branch, _torch_map(gt), None, self.eps, self.loss_weight, self.reduction)
