"""What test_cpu_native_rule.py and test_gpu_native_rule.py share: the public calls whose path (kernels or torch) the
rule decides, each as a function of one pair of tensors, and the counter that observes which path a call took.

The path is observed, not asked: every launch and every host-side C call passes through ssl_amd._lib.check, the torch
expressions make no C call, so a call took the kernels exactly when the counter moved."""
import contextlib

import torch

T = 50                      # the diffusion schedule's steps
TILES, TILE = [(0, 0), (4, 4)], 4


@contextlib.contextmanager
def c_calls():
    """The statuses that passed through ssl_amd._lib.check inside the block."""
    from ssl_amd import _lib
    seen, real = [], _lib.check

    def counting(status):
        seen.append(status)
        return real(status)

    _lib.check = counting
    try:
        yield seen
    finally:
        _lib.check = real


_SCHEDULES = {}


def _schedule(x):
    from ssl_amd.diffusion import Schedule
    key = str(x.device)
    if key not in _SCHEDULES:
        _SCHEDULES[key] = Schedule(timesteps=T, device=x.device)
    return _SCHEDULES[key]


def _t(x):
    return torch.tensor([0, T - 1], device=x.device)


def calls():
    """name -> f(a, b).  `b` is the tensor the asymmetric variations change (the target, the second device, the other
    layout), so the calls of one tensor take `b`."""
    from ssl_amd import diffusion, losses
    from ssl_amd.losses import perceptual
    gan = losses.GANLoss('vanilla')
    return {
        "L1Loss": lambda a, b: losses.L1Loss()(a, b),
        "KLDistanceLoss": lambda a, b: losses.KLDistanceLoss()(a, b),
        "MSELoss": lambda a, b: losses.MSELoss()(a, b),
        "CharbonnierLoss": lambda a, b: losses.CharbonnierLoss()(a, b),
        "GradientLoss.forward": lambda a, b: losses.GradientLoss()(a, b),
        "GradientLoss.branch": lambda a, b: losses.GradientLoss().branch(a, b),
        "Get_gradient": lambda a, b: losses.Get_gradient()(b),
        "GANLoss.forward": lambda a, b: gan(b, True),
        "GANLoss.relativistic_term": lambda a, b: gan.relativistic_term(a, b, True),
        "GANLoss.relativistic_generator": lambda a, b: gan.relativistic_generator(a, b),
        "multi_criterion": lambda a, b: perceptual.multi_criterion([a], [b], [1.0], 'l1'),
        "q_sample": lambda a, b: _schedule(a).q_sample(a, _t(a), b),
        "p_sample": lambda a, b: _schedule(a).p_sample(a, b, _t(a), b),
        "p_losses_criterion": lambda a, b: diffusion.p_losses_criterion(a, b, b, _t(a), _schedule(a),
                                                                        torch.zeros(T, device=a.device)),
        "canvas_gather": lambda a, b: diffusion.canvas_gather(b, TILES, TILE),
    }


PAIR = {"L1Loss", "KLDistanceLoss", "MSELoss", "CharbonnierLoss"}
GRADIENT = {"GradientLoss.forward", "GradientLoss.branch"}
GAN = {"GANLoss.forward", "GANLoss.relativistic_term", "GANLoss.relativistic_generator"}
DIFFUSION = {"q_sample", "p_sample", "p_losses_criterion", "canvas_gather"}
MODULES = PAIR | GRADIENT | GAN | {"Get_gradient", "multi_criterion"}      # everything but the diffusion calls
ALL = MODULES | DIFFUSION


def pair(device, shape=(2, 3, 8, 8), seed=0):
    """Two positive fp32 tensors (KLDistanceLoss takes logarithms)."""
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.rand(shape, generator=g) + 0.1).to(device) for _ in range(2))


def took_kernels(call, a, b, may_raise=()):
    """Whether call(a, b) made a C call.  An exception of a type in may_raise ends the call without failing the test
    (torch refuses some of the inputs that the rule sends its way)."""
    with c_calls() as seen:
        try:
            call(a, b)
        except may_raise:
            pass
    return bool(seen)
