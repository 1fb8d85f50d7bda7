from .basic_loss import ArtifactLoss, KLDistanceLoss, L1Loss, SSGLoss, set_native_criteria  # noqa: F401
from .loss_util import get_artifact_map, get_local_weights, get_refined_artifact_map, similarity_map  # noqa: F401
from .lazy import LazySSG, lazy_enabled, set_lazy  # noqa: F401
from .bebygan import BBL, BackProjectionLoss, BestBuddyLoss, get_flat_mask, imresize  # noqa: F401
from .ssim import SSIMLoss, create_window, gaussian, ssim  # noqa: F401
from .gan_loss import GANLoss, MultiScaleGANLoss  # noqa: F401
from .spsr import CharbonnierLoss, Get_gradient, Get_gradient_nopadding, GradientLoss, MSELoss  # noqa: F401
from .perceptual import PerceptualLoss, VGGFeatureExtractor  # noqa: F401
from . import kair  # noqa: F401
from .lpips import lpips_criterion  # noqa: F401
from .contperceptual import LPIPSWithDiscriminator  # noqa: F401
