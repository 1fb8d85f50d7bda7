"""BebyGAN's best-buddy loss and flat mask behind the reference's names (bebyganssl_model.py:93-104, 471-565),
on the kernels of ssl_amd/csrc/ssg_bbl.hip, and its imresize and back-projection loss (:375-469, :727-731) on those
of ssl_amd/csrc/ssg_bp.hip."""
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


def imresize(x, scale=None, sides=None, kernel='cubic', sigma=2, rotation_degree=0, padding_type='reflect',
             antialiasing=True):
    """The reference's imresize (bebyganssl_model.py:375-469) on the path its configs reach: an integer downsampling
    factor 1 / scale in {2, 3, 4} with the discrete antialiased bicubic kernel (Keys a = -0.5, 4 / scale taps,
    edge-repeating "reflect" padding), output sides H // s, W // s.  2-D, 3-D and 4-D floating tensors; computed in fp32
    and cast back; differentiable with respect to x.  `sigma` and `rotation_degree` are accepted and unused, as in the
    reference.  The table-driven path (`sides=`, non-integer scales, upsampling, the 'gaussian' or a tensor kernel,
    antialiasing=False, integer dtypes) raises NotImplementedError: no reference config reaches it."""
    if scale is None and sides is None:
        raise ValueError('One of scale or sides must be specified!')
    if scale is not None and sides is not None:
        raise ValueError('Please specify scale or sides to avoid conflict!')
    if x.dim() not in (2, 3, 4):
        raise ValueError('{}-dim Tensor is not supported!'.format(x.dim()))
    if sides is not None:
        raise NotImplementedError("ssl_amd: imresize runs the integer-factor path only; `sides=` selects the "
                                  "table-driven resize_1d path")
    if not isinstance(kernel, str) or kernel != 'cubic':
        raise NotImplementedError(f"ssl_amd: imresize runs kernel='cubic' only, got kernel="
                                  f"{kernel if isinstance(kernel, str) else type(kernel).__name__!r}")
    if not antialiasing:
        raise NotImplementedError("ssl_amd: imresize runs antialiasing=True only")
    if padding_type != 'reflect':
        raise NotImplementedError(f"ssl_amd: imresize runs padding_type='reflect' only, got {padding_type!r}")
    if not x.dtype.is_floating_point:
        raise NotImplementedError(f"ssl_amd: imresize runs floating dtypes only, got dtype {x.dtype}")
    scale = float(scale)
    if not (0 < scale < 1) or not (1 / scale).is_integer():
        raise NotImplementedError(f"ssl_amd: imresize runs scale = 1/2, 1/3 and 1/4 only (an integer downsampling "
                                  f"factor), got scale={scale}")
    if int(1 / scale) > 4:
        raise NotImplementedError(f"ssl_amd: imresize runs downsampling factors up to 4, got scale={scale} "
                                  f"(factor {int(1 / scale)})")
    return engine.bp_downsample(x, int(1 / scale))


class BackProjectionLoss(nn.Module):
    """L1Loss(loss_weight, reduction)(imresize(output, scale=1 / scale), lq) in one fused call (the caller's
    bebyganssl_model.py:727-731, pixel_bp_opt): the downsampling, the loss and the gradient with respect to the output
    come out of the same pass.  reduction 'mean' or 'sum'; lq is (B, C, H // scale, W // scale) and carries no
    gradient (an lq that requires grad raises)."""

    def __init__(self, loss_weight=1.0, reduction='mean', scale=4):
        super(BackProjectionLoss, self).__init__()
        if reduction not in ('mean', 'sum'):
            raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: ['mean', 'sum']")
        if scale != int(scale) or int(scale) not in (2, 3, 4):
            raise NotImplementedError(f"ssl_amd: BackProjectionLoss runs the integer factors 2, 3 and 4 only, got "
                                      f"scale={scale}")
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.scale = int(scale)

    def forward(self, output, lq):
        if output.dim() != 4:
            raise ValueError(f"ssl_amd: BackProjectionLoss takes a (B,C,H,W) output, got {tuple(output.shape)}")
        return engine.bp_loss(output, lq, self.scale, self.loss_weight, self.reduction)
