"""BebyGAN's best-buddy loss and flat mask behind the reference's names (bebyganssl_model.py:93-104, 471-565),
on the kernels of ssl_amd/csrc/ssg_bbl.hip."""
import torch.nn.functional as F
from torch import nn

from .. import engine


class BBL():
    """The reference's BBL: forward(x, gt) -> (p1, sel_p2), both (B,N,d).  p1 is differentiable with respect to x,
    sel_p2 carries no gradient, so the caller's `L1Loss(p1, sel_p2)` trains as before.  Among candidates whose fp32
    scores are equal the lowest index of cat[p2, p2_2, p2_4] is selected.

    Native domain: dist_norm 'l2', pad 0, stride >= ksize, C * ksize^2 <= 31 (every reference config constructs
    BBL()); anything else raises NotImplementedError."""

    def __init__(self, alpha=1.0, beta=1.0, ksize=3, pad=0, stride=3, dist_norm='l2'):
        if dist_norm != 'l2':
            raise NotImplementedError(f"ssl_amd: BBL runs the 'l2' distance only (one matrix product per search), "
                                      f"got dist_norm={dist_norm!r}")
        if pad != 0:
            raise NotImplementedError(f"ssl_amd: BBL runs pad=0 only, got pad={pad}")
        if stride < ksize:
            raise NotImplementedError(f"ssl_amd: BBL needs stride >= ksize (patches that do not overlap), got "
                                      f"ksize={ksize}, stride={stride}")
        self.alpha = alpha
        self.beta = beta
        self.ksize = ksize
        self.pad = pad
        self.stride = stride
        self.dist_norm = dist_norm

    def forward(self, x, gt):
        return engine.bbl_patches(x, gt, self.alpha, self.beta, self.ksize, self.stride)

    __call__ = forward


def get_flat_mask(img, kernel_size=11, std_thresh=0.025, scale=1):
    """1.0 where the standard deviation of the kernel_size^2 luminance window is below std_thresh; no gradient."""
    if scale > 1:
        img = F.interpolate(img, scale_factor=scale, mode='bicubic', align_corners=False)
    return engine.flat_mask(img.detach(), kernel_size, std_thresh)


class BestBuddyLoss(nn.Module):
    """L1Loss(loss_weight, reduction)(*BBL(alpha, beta).forward(x, gt)) in one fused call: the search, the loss and
    the gradient with respect to x come out of the same pass.  reduction 'mean' or 'sum'; a gt that requires grad
    raises."""

    def __init__(self, loss_weight=1.0, reduction='mean', alpha=1.0, beta=1.0, ksize=3, stride=3):
        super(BestBuddyLoss, self).__init__()
        if reduction not in ('mean', 'sum'):
            raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: ['mean', 'sum']")
        if stride < ksize:
            raise NotImplementedError(f"ssl_amd: BestBuddyLoss needs stride >= ksize, got ksize={ksize}, "
                                      f"stride={stride}")
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.alpha = alpha
        self.beta = beta
        self.ksize = ksize
        self.stride = stride

    def forward(self, x, gt):
        return engine.bbl_loss(x, gt, self.alpha, self.beta, self.ksize, self.stride, self.loss_weight,
                               self.reduction)
