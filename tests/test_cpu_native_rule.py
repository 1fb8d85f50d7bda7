"""The rule that decides which calls take the kernels (ssl_amd/_gpu.py: the switch, `readable`, `native`) on what a
machine without a GPU can form: CPU tensors never reach the C ABI and give the torch expressions' bits, the switch has
one home, and ssl_amd.ema / ssl_amd.diffusion stand on _gpu alone."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import native_rule_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _bce(x, label):
    return F.binary_cross_entropy_with_logits(x, x.new_ones(x.size()) * label)


# the torch expressions of the reference for the calls of N.calls(), as test_cpu_spsr.py, test_cpu_gan.py and
# test_cpu_perceptual.py state them
EXPRESSIONS = {
    "L1Loss": lambda a, b: F.l1_loss(a, b, reduction='none').mean(),
    "KLDistanceLoss": lambda a, b: 0.1 * F.kl_div(torch.clamp(a, min=1e-10).log(), torch.clamp(b, min=1e-10),
                                                  reduction='mean'),
    "MSELoss": lambda a, b: F.mse_loss(a, b, reduction='none').mean(),
    "CharbonnierLoss": lambda a, b: torch.sqrt((a - b) ** 2 + 1e-12).mean(),
    "GANLoss.forward": lambda a, b: _bce(b, 1.0),
    "GANLoss.relativistic_term": lambda a, b: _bce(a - torch.mean(b), 1.0),
    "GANLoss.relativistic_generator": lambda a, b: (_bce(a - torch.mean(b), 0.0) + _bce(b - torch.mean(a), 1.0)) / 2,
    "multi_criterion": lambda a, b: (0 + F.l1_loss(a, b) * 1.0) * 1.0,
}


@pytest.mark.parametrize("switch", [True, False])
def test_cpu_tensors_never_reach_the_c_abi(switch):
    from ssl_amd.losses import set_native_criteria
    a, b = N.pair(CPU)
    prev = set_native_criteria(switch)
    try:
        for name, call in N.calls().items():
            with N.c_calls() as seen:
                got = call(a, b)
            assert not seen, name
            if name in EXPRESSIONS:
                assert torch.equal(_bits(got), _bits(EXPRESSIONS[name](a, b))), name
    finally:
        set_native_criteria(prev)


def test_readable_and_native_on_what_a_cpu_machine_can_form():
    from ssl_amd import _gpu
    from ssl_amd.losses import set_native_criteria
    x = torch.rand(2, 3)
    assert _gpu.readable() is False
    assert not _gpu.readable(None) and not _gpu.readable([1.0]) and not _gpu.readable(x, 1.0)
    assert not _gpu.readable(x) and not _gpu.readable(x, x) and not _gpu.readable(x.double())
    for switch in (True, False):
        prev = set_native_criteria(switch)
        try:
            assert not _gpu.native() and not _gpu.native(x) and not _gpu.native(object())
        finally:
            set_native_criteria(prev)


def test_native_follows_the_switch(monkeypatch):
    """(with `readable` taken as given: no GPU tensor can be formed here)"""
    from ssl_amd import _gpu
    from ssl_amd.losses import set_native_criteria
    monkeypatch.setattr(_gpu, "readable", lambda *tensors: True)
    x = torch.rand(2, 3)
    prev = set_native_criteria(True)
    try:
        assert _gpu.native(x)
        set_native_criteria(False)
        assert not _gpu.native(x)
    finally:
        set_native_criteria(prev)


def test_set_native_criteria_returns_the_previous_setting_and_gpu_holds_it():
    from ssl_amd import _gpu, losses
    first = losses.set_native_criteria(False)
    try:
        assert _gpu.native_criteria() is False
        assert losses.set_native_criteria(True) is False and _gpu.native_criteria() is True
        assert losses.set_native_criteria(0) is True and _gpu.native_criteria() is False
    finally:
        losses.set_native_criteria(first)
    assert _gpu.native_criteria() is first
    assert losses.set_native_criteria is losses.basic_loss.set_native_criteria


def test_the_flag_has_one_home():
    old = "_NATIVE_CRITERIA"
    package = os.path.join(ROOT, "ssl_amd")
    found = []
    for folder, _, files in os.walk(package):
        for name in files:
            path = os.path.join(folder, name)
            if name.endswith(".py") and os.path.relpath(path, package) != "_gpu.py":
                with open(path) as f:
                    if re.search(old, f.read()):
                        found.append(os.path.relpath(path, ROOT))
    assert not found


@pytest.mark.parametrize("module", ["ssl_amd.ema", "ssl_amd.diffusion"])
def test_ema_and_diffusion_load_neither_engine_nor_losses(module):
    code = (f"import sys; import {module}; "
            "print([m for m in ('ssl_amd.engine', 'ssl_amd.losses') if m in sys.modules])")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "[]"


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("channels", [None, 1, 3])
def test_l1_fallback_is_the_references_weight_reduce_loss(reduction, channels):
    """basicsr's weighted_loss / weight_reduce_loss (loss_util.py:33-62) written out: with a weight under 'mean', the
    sum over the weighted region, a one-channel weight counting once per channel of the loss."""
    from ssl_amd.losses import L1Loss
    a, b = N.pair(CPU, seed=3)
    weight = None if channels is None else torch.rand(2, channels, 8, 8, generator=torch.Generator().manual_seed(4))
    loss = F.l1_loss(a, b, reduction='none')
    if weight is not None:
        loss = loss * weight
    want = loss
    if reduction == 'sum':
        want = loss.sum()
    elif reduction == 'mean' and weight is None:
        want = loss.mean()
    elif reduction == 'mean':
        want = loss.sum() / (weight.sum() if weight.size(1) > 1 else weight.sum() * loss.size(1))
    got = L1Loss(loss_weight=0.7, reduction=reduction)(a, b, weight)
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(0.7 * want))
