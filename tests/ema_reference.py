"""The three EMA / copy updates of the reference as torch expressions on CPU tensors, written out from
GAN-Based-SR/basicsr/models/base_model.py:75-82 (model_ema), GAN-Based-SR/train_BSGRAN/models/model_base.py:192-197
(update_E) and Diffusion-Based-SR/ldm/modules/ema.py (LitEma), with LitEma's warm-up scalars step by step, and the small
seeded model of tests/golden/f34_ema.npz.  The oracle of ssl_amd.ema and of ssg_multi_apply: their results are compared
with these bit for bit."""
import torch
from torch import nn

EMA, LIT, COPY = 0, 1, 2        # include/ssg_hip.h: SSG_MT_*

FIXTURE_STEPS, FIXTURE_DECAY = 12, 0.5      # the warm-up (1 + n) / (10 + n) crosses 0.5 at n = 8
FIXED_STEPS, FIXED_DECAY = 3, 0.9999        # use_num_upates=False: no warm-up


def ema_update(e, p, decay):
    """model_ema / update_E on one pair, in place: e <- e * decay + (1 - decay) * p as torch rounds it."""
    return e.mul_(decay).add_(p, alpha=1 - decay)


def lit_scalars(decay, num_updates):
    """LitEma.forward's scalars.  decay: the 0-d fp32 buffer; num_updates: the 0-d int32 buffer, INCREMENTED IN PLACE when
    it counts (>= 0).  Returns (decay of this step, one_minus_decay), two 0-d fp32 tensors."""
    d = decay
    if num_updates >= 0:
        num_updates += 1
        d = min(decay, (1 + num_updates) / (10 + num_updates))
    return d, 1.0 - d


def lit_update(shadow, p, one_minus_decay):
    """LitEma.forward on one pair, in place."""
    return shadow.sub_(one_minus_decay * (shadow - p))


def copy_update(e, p):
    return e.copy_(p)


def apply(kind, e, p, decay=None, w=None):
    """One pair through the update `kind` (in place on e): decay a Python float for EMA, w a 0-d fp32 tensor for LIT."""
    if kind == EMA:
        return ema_update(e, p, decay)
    if kind == LIT:
        return lit_update(e, p, w)
    return copy_update(e, p)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, want):
    """Equal int32 patterns, except that where both are NaN any NaN matches."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != torch.float32:
        return bool(torch.equal(got, want))
    both_nan = torch.isnan(got) & torch.isnan(want)
    return bool(((bits(got) == bits(want)) | both_nan.contiguous()).all())


# ---- the fixture's model: two convolutions, one frozen parameter ----
def fixture_model(init=None):
    """The model of the fixture; init: {parameter name: values} as recorded in it (the tests take the recorded ones, so
    that they do not depend on the generator's stream; make_golden_ema.py draws them)."""
    gen = torch.Generator().manual_seed(34)
    net = nn.Sequential(nn.Conv2d(3, 4, 3), nn.Conv2d(4, 2, 1))
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.2 if init is None else torch.as_tensor(init[name]))
    net[0].bias.requires_grad_(False)
    return net


def fixture_perturbations(steps):
    """{parameter name: (steps, *shape)}: what is added to each parameter (the frozen one too) before update t."""
    gen = torch.Generator().manual_seed(340)
    return {name: torch.randn((steps,) + tuple(p.shape), generator=gen) * 0.05
            for name, p in fixture_model().named_parameters()}


def perturb(net, pert, t):
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.add_(pert[name][t])
