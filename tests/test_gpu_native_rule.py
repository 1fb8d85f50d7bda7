"""Which path, the kernels or the reference's torch expressions, every public call takes for every kind of input: the
rule of ssl_amd/_gpu.py (the switch, fp32 tensors on one GPU) and each family's extras, as a table ("Which
calls take the kernels").  Only the decision is under test: every kernel is held to its reference elsewhere."""
import pytest
import torch

import native_rule_cases as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _channels_last(x):
    return x.contiguous(memory_format=torch.channels_last)


def _with_gaps(x):
    wide = torch.rand(x.shape[:-1] + (2 * x.shape[-1],), device=x.device) + 0.1
    return wide[..., ::2]


# variation -> (what it makes of the fp32 GPU pair, the calls it is asked of, those of them that take the kernels,
#               the exceptions with which torch may refuse the input)
NONE = set()
VARIATIONS = {
    "fp32": (lambda a, b: (a, b), N.ALL, N.ALL, ()),
    "fp64": (lambda a, b: (a.double(), b.double()), N.ALL, NONE, ()),
    "fp16": (lambda a, b: (a.half(), b.half()), N.ALL, NONE, ()),
    "bf16": (lambda a, b: (a.bfloat16(), b.bfloat16()), N.ALL, NONE, ()),
    "cpu": (lambda a, b: (a.cpu(), b.cpu()), N.ALL, NONE, ()),
    "gpu_and_cpu": (lambda a, b: (a, b.cpu()), N.ALL, NONE, (RuntimeError,)),
    "target_requires_grad": (lambda a, b: (a, b.clone().requires_grad_(True)), N.ALL, N.GAN | {"Get_gradient"}, ()),
    "empty": (lambda a, b: (a[:0], b[:0]), N.MODULES, NONE, ()),
    "three_dimensions": (lambda a, b: (a[:, 0].contiguous(), b[:, 0].contiguous()), N.PAIR | N.GRADIENT | {"Get_gradient"},
                         N.PAIR, (RuntimeError,)),
    "two_shapes": (lambda a, b: (a, b[:1]), N.PAIR | N.GRADIENT | {"multi_criterion", "GANLoss.relativistic_term"},
                   {"GANLoss.relativistic_term"}, ()),
    "channels_last": (lambda a, b: (_channels_last(a), _channels_last(b)), N.ALL, N.ALL, ()),
    "one_channels_last": (lambda a, b: (a, _channels_last(b)), N.ALL, N.ALL - {"multi_criterion"}, ()),
    "view_with_gaps": (lambda a, b: (a, _with_gaps(b)), N.ALL, N.ALL - {"multi_criterion"}, ()),
}


@pytest.mark.parametrize("variation", list(VARIATIONS))
def test_the_path_of_every_call(dev, variation):
    make, asked, native, may_raise = VARIATIONS[variation]
    a, b = make(*N.pair(dev))
    calls = N.calls()
    took = {name for name in sorted(asked) if N.took_kernels(calls[name], a, b, may_raise)}
    assert took == native, (sorted(took - native), sorted(native - took))


def test_diffusion_takes_the_kernels_under_no_grad_whatever_requires_grad(dev):
    a, b = N.pair(dev)
    b.requires_grad_(True)
    calls = N.calls()
    with torch.no_grad():
        took = {name for name in sorted(N.ALL) if N.took_kernels(calls[name], a, b)}
    assert took == N.GAN | N.DIFFUSION | {"Get_gradient"}


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_a_pair_on_two_gpus_takes_torch(dev):
    a, b = N.pair(dev)
    b = b.to("cuda:1")
    calls = N.calls()
    took = {name for name in sorted(N.ALL) if N.took_kernels(calls[name], a, b, (RuntimeError,))}
    # (the calls of one tensor are handed b alone: one GPU, the kernels, on cuda:1)
    assert took == {"Get_gradient", "GANLoss.forward", "canvas_gather"}


def test_a_weight_and_reduction_none_take_torch(dev):
    from ssl_amd import losses
    a, b = N.pair(dev)
    for cls in (losses.L1Loss, losses.MSELoss, losses.CharbonnierLoss):
        assert N.took_kernels(lambda x, y: cls()(x, y), a, b)
        assert not N.took_kernels(lambda x, y: cls()(x, y, weight=torch.ones_like(x)), a, b)
        assert not N.took_kernels(lambda x, y: cls(reduction='none')(x, y), a, b)
    none = losses.GradientLoss(reduction='none')
    assert not N.took_kernels(none, a, b) and not N.took_kernels(none.branch, a, b)


def test_the_switch_governs_the_modules_not_the_functional_api(dev):
    from ssl_amd import engine
    from ssl_amd.losses import set_native_criteria
    a, b = N.pair(dev)
    calls = N.calls()
    prev = set_native_criteria(False)
    try:
        took = {name for name in sorted(N.ALL) if N.took_kernels(calls[name], a, b)}
        assert took == set()
        assert engine.multi_pair_is_native(a, b)
        assert N.took_kernels(lambda x, y: engine.multi_pixel_loss([x], [y], [1.0], 'l1'), a, b)
    finally:
        set_native_criteria(prev)
    assert N.took_kernels(calls["L1Loss"], a, b)
