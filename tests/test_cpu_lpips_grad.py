"""The differentiable LPIPS term and the autoencoder stage's criterion without a GPU: the gradient's restatement against
fp64 autograd of the package's lines, torch's fp32 lines within the wider bound, the NaN pattern at all-zero vectors,
every refusal of ssg_lpips_layers_backward (decided before any launch, so no GPU is needed), the dispatch of
lpips_criterion and LPIPS on CPU tensors, and LPIPSWithDiscriminator / DiagonalGaussianDistribution / normal_kl on the
CPU against the fixture recorded from the reference (tests/golden/f37_contperceptual.npz), bit for bit."""
import os

import numpy as np
import pytest
import torch

import contperceptual_cases as CC
import featmetric_cases as FC
import lpips_grad_cases as C
import lpips_grad_reference as R
from ssl_amd import distributions as D, metrics_feat as MF
from ssl_amd.losses import contperceptual as CP, lpips as LP

UNIT, CAP = 256, 4            # (a small cap keeps the CPU cases small; the GPU tests use the library's)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f37_contperceptual.npz")


@pytest.fixture(scope="module")
def sets():
    """(name, maps, restatement, fp64 autograd, fp32 autograd) of every case, computed once"""
    out = []
    for name, N, layers, content in C.cases(UNIT, CAP):
        f0, f1, w, coef = C.maps(N, layers, content)
        grads = []
        for dtype in (torch.float64, torch.float32):
            a = [t.clone().to(dtype).requires_grad_(True) for t in f0]
            b = [t.clone().to(dtype).requires_grad_(True) for t in f1]
            val = MF.lpips_torch_lines(a, b, [t.to(dtype).reshape(1, -1, 1, 1) for t in w])
            (val.reshape(-1) * coef.to(dtype)).sum().backward()
            grads.append(([t.grad for t in a], [t.grad for t in b]))
        out.append((name, (f0, f1, w, coef), R.lpips_grad(f0, f1, w, coef), grads[0], grads[1]))
    return out


def test_restatement_against_fp64_autograd_of_the_package_lines(sets):
    for name, _, ref, (g0, g1), _ in sets:
        for k, r in enumerate(ref):
            s0 = R.share(g0[k], r.g0, r.fp64_bound0, skip=r.nan0)
            s1 = R.share(g1[k], r.g1, r.fp64_bound1, skip=r.nan1)
            print(f"{name} layer {k}: fp64 autograd uses {s0:.3g} / {s1:.3g} of the fp64 bound")
            assert s0 <= 1.0 and s1 <= 1.0, (name, k)
            if "identical" in name:
                assert (r.g0 == 0).all() and (r.g1 == 0).all()


def test_torch_fp32_lines_within_the_wider_bound(sets):
    for name, _, ref, _, (g0, g1) in sets:
        for k, r in enumerate(ref):
            s0 = R.share(g0[k], r.g0, r.torch_bound0, skip=r.nan0)
            s1 = R.share(g1[k], r.g1, r.torch_bound1, skip=r.nan1)
            print(f"{name} layer {k}: torch's fp32 lines (CPU) use {s0:.3g} / {s1:.3g} of the wider bound")
            assert s0 <= 1.0 and s1 <= 1.0, (name, k)


def test_nan_pattern_at_zero_vectors_is_torchs(sets):
    seen = 0
    for name, (f0, f1, _, _), ref, g64, g32 in sets:
        for k, r in enumerate(ref):
            want0 = np.broadcast_to(r.nan0, r.g0.shape)
            want1 = np.broadcast_to(r.nan1, r.g1.shape)
            assert (want0 == (f0[k].numpy() == 0).all(axis=1, keepdims=True)).all()
            assert (R.nan_pattern(r.g0) == want0).all() and (R.nan_pattern(r.g1) == want1).all(), (name, k)
            for g0, g1 in (g64, g32):
                assert (R.nan_pattern(g0[k]) == want0).all() and (R.nan_pattern(g1[k]) == want1).all(), (name, k)
            seen += int(want0.any()) + int(want1.any())
            # one side's zero vector leaves the other side finite there
            only0 = np.broadcast_to(r.nan0 & ~r.nan1, r.g1.shape)
            assert np.isfinite(r.g1[only0]).all()
    assert seen >= 4


def test_every_refusal_without_a_gpu():
    from ssl_amd import _lib
    from ssl_amd._gpu import address_array
    L, E = _lib.lib(), _lib.CONSTANTS
    ints = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    # made-up device addresses: a refusal is decided before any launch and reads none of them
    a0, a1, aw, b0, b1 = (address_array([base, base + 4096]) for base in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20))
    Cs, H, W = ints([3, 6]), ints([4, 1]), ints([5, 1])
    coef = 6 << 20

    def call(K=2, n=2, p0=a0, p1=a1, pw=aw, c=Cs, h=H, wd=W, cf=coef, g0=b0, g1=b1):
        arr = lambda v: None if v is None else v.ctypes.data
        return L.ssg_lpips_layers_backward(K, n, arr(p0), arr(p1), arr(pw), arr(c), arr(h), arr(wd), cf, arr(g0), arr(g1),
                                           None)

    many = ints([1] * 17)
    zero = address_array([1 << 20, 0])
    odd = address_array([(1 << 20) + 2, 2 << 20])
    bad, align, large = E["SSG_E_BADARG"], E["SSG_E_ALIGN"], E["SSG_E_TOOLARGE"]
    assert call(K=0) == bad and call(K=17, c=many, h=many, wd=many) == bad and call(n=0) == bad
    assert call(c=ints([3, 0])) == bad and call(h=ints([0, 1])) == bad and call(wd=ints([5, -1])) == bad
    assert call(p0=None) == bad and call(p1=None) == bad and call(pw=None) == bad and call(c=None) == bad
    assert call(cf=None) == bad                                   # a null coef
    assert call(g0=None, g1=None) == bad                          # both gradient arrays null
    for name in ("p0", "p1", "pw", "g0", "g1"):                   # a null entry inside a given array
        assert call(**{name: zero}) == bad, name
    assert call(g0=zero, g1=None) == bad and call(g0=None, g1=zero) == bad
    for name in ("p0", "p1", "pw", "g0", "g1"):                   # a float address that is not 4-byte aligned
        assert call(**{name: odd}) == align, name
    assert call(cf=coef + 2) == align
    assert call(h=ints([1 << 20, 1]), wd=ints([1 << 20, 1])) == large
    assert call(n=1 << 30, h=ints([1 << 10, 1]), wd=ints([1 << 10, 1])) == large      # the unit count


def test_wrapper_refuses_what_the_kernel_cannot_read_whatever_the_flag():
    from ssl_amd.losses import set_native_criteria
    f, w, coef = torch.rand(1, 4, 3, 3), torch.rand(4), torch.rand(1)
    for flag in (True, False):
        prev = set_native_criteria(flag)
        try:
            for t in (f, f.half(), f.double(), f.bfloat16()):
                with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                    MF.lpips_layers_backward([t], [t], [w], coef, True, True)
        finally:
            set_native_criteria(prev)


def test_criterion_on_cpu_tensors_is_the_torch_lines():
    f0, f1, w, _ = C.maps(2, C.LAYERS_A[:3], "relu")
    lins = [t.reshape(1, -1, 1, 1) for t in w]
    a = [t.clone().requires_grad_(True) for t in f0]
    b = [t.clone().requires_grad_(True) for t in f0]
    got, want = LP.lpips_criterion(a, f1, lins), MF.lpips_torch_lines(b, f1, lins)
    assert got.shape == (2, 1, 1, 1) and torch.equal(got, want)
    got.sum().backward(), want.sum().backward()
    for x, y in zip(a, b):
        assert torch.equal(x.grad.isnan(), y.grad.isnan()) and torch.equal(x.grad.nan_to_num(), y.grad.nan_to_num())


@pytest.fixture(scope="module")
def vgg_state():
    return FC.lpips_state('vgg')[0]


def test_lpips_module_on_the_cpu(vgg_state):
    net = LP.LPIPS(vgg_state)
    metric = MF.LPIPS('vgg', vgg_state)
    assert not net.training and not net.train().training and not any(p.requires_grad for p in net.parameters())
    x, y = C.images((2, 3, 32, 32))
    x = x.requires_grad_(True)
    out = net(x, y)
    assert out.shape == (2, 1, 1, 1) and out.requires_grad
    with torch.no_grad():
        assert torch.equal(out.detach(), metric(x, y))           # the metric's module on the same weights
    out.sum().backward()
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    assert [tuple(f.shape) for f in net.features(y)] == [(2, c, 32 >> s, 32 >> s) for s, c in enumerate(MF.VGG_CHANNELS)]
    with pytest.raises(KeyError):
        LP.LPIPS(FC.lpips_state('vgg')[1])                       # a trunk without the lin layers


def test_taming_restatements():
    d = CP.NLayerDiscriminator()
    convs = [m for m in d.main if isinstance(m, torch.nn.Conv2d)]
    assert [(c.in_channels, c.out_channels, c.stride[0], c.bias is not None) for c in convs] == [
        (3, 64, 2, True), (64, 128, 2, False), (128, 256, 2, False), (256, 512, 1, False), (512, 1, 1, True)]
    assert all(c.kernel_size == (4, 4) and c.padding == (1, 1) for c in convs)
    assert sum(isinstance(m, torch.nn.BatchNorm2d) for m in d.main) == 3
    assert sum(isinstance(m, torch.nn.LeakyReLU) and m.negative_slope == 0.2 for m in d.main) == 4
    assert d(torch.zeros(1, 3, 64, 64)).shape == (1, 1, 6, 6)
    wide = [m.out_channels for m in CP.NLayerDiscriminator(input_nc=4, ndf=8, n_layers=5).main if isinstance(m, torch.nn.Conv2d)]
    assert wide == [8, 16, 32, 64, 64, 64, 1]
    with pytest.raises(NotImplementedError):
        CP.NLayerDiscriminator(use_actnorm=True)
    torch.manual_seed(0)
    d.apply(CP.weights_init)
    bn = [m for m in d.main if isinstance(m, torch.nn.BatchNorm2d)][0]
    assert float(bn.bias.detach().abs().max()) == 0 and abs(float(bn.weight.detach().mean()) - 1) < 0.02
    assert abs(float(convs[2].weight.detach().std()) - 0.02) < 1e-3
    real, fake = torch.tensor([[2.0, 0.5, -1.0]]), torch.tensor([[-2.0, 0.5, 1.0]])
    assert float(CP.hinge_d_loss(real, fake)) == pytest.approx(0.5 * ((0 + 0.5 + 2) / 3 + (0 + 1.5 + 2) / 3))
    want = 0.5 * (torch.log1p(torch.exp(-real)).mean() + torch.log1p(torch.exp(fake)).mean())
    assert float(CP.vanilla_d_loss(real, fake)) == pytest.approx(float(want))
    assert CP.adopt_weight(0.7, 9, threshold=10) == 0.0 and CP.adopt_weight(0.7, 10, threshold=10) == 0.7
    lr, lf = torch.rand(2, 1, 3, 3) * 3 - 1, torch.rand(2, 1, 3, 3) * 3 - 2
    assert float(CP.hinge_d_loss_with_exemplar_weights(lr, lf, torch.ones(2))) == pytest.approx(float(CP.hinge_d_loss(lr, lf)))


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


def _same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(
        (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def test_inputs_are_the_fixtures(golden):
    t = CC.make_inputs()
    assert all(_same_bits(v, golden["in_" + k]) for k, v in t.items())


@pytest.mark.parametrize("name", list(CC.CASES))
def test_module_on_the_cpu_reproduces_the_reference(golden, vgg_state, name):
    t = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    loss = CC.plug(CC.build(CP.LPIPSWithDiscriminator, name, lpips_weights=vgg_state), t)
    got = CC.run_case(loss, D.DiagonalGaussianDistribution, t, name)
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "_")}
    assert set(got) == set(want) and len(want) >= 4, (sorted(got), sorted(want))
    for key in want:
        assert _same_bits(got[key], want[key]), (key, got[key], want[key])
    idx, _, kl, step, factor, in_graph = CC.CASES[name]
    if idx == 0:
        assert ("log_kl_loss" in want) == (kl > 0)
        assert float(want["log_disc_factor"]) == (factor if step >= CC.DISC_START else 0.0)
        if factor > 0 and not in_graph:
            assert float(want["log_d_weight"]) == 0.5             # torch.tensor(1.0) * discriminator_weight
        if factor == 0:
            assert float(want["log_d_weight"]) == 0.0
    else:
        assert set(want) == {"loss", "log_disc_loss", "log_logits_real", "log_logits_fake", "grad_disc_w0"}


def test_return_dic_and_weights_take_the_reference_lines(golden, vgg_state):
    t = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    name = "gen_hinge_kl_late"
    loss = CC.plug(CC.build(CP.LPIPSWithDiscriminator, name, lpips_weights=vgg_state), t)
    rec, last, _ = CC.reconstructions(t, True)
    post = D.DiagonalGaussianDistribution(t["posterior"])
    value, log, dic = loss(t["inputs"], rec, post, 0, 150, last_layer=last, return_dic=True)
    assert _same_bits(value.detach(), golden[name + "_loss"]) and set(dic) == {k.split("/")[1] for k in log}
    w = torch.full((CC.N, 1, 1, 1), 2.0)
    twice, _ = loss(t["inputs"], rec, post, 0, 150, last_layer=last, weights=w)
    assert twice.requires_grad and float(twice.detach()) != float(value.detach())
    d_loss, log, dic = loss(t["inputs"], rec, post, 1, 150, return_dic=True)
    assert set(dic) == set(log) == {"train/disc_loss", "train/logits_real", "train/logits_fake"}


def test_key_sets_star_import_and_the_criterion_chosen_at_the_call(golden, vgg_state):
    t = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    name = "gen_vanilla_nokl_early"                      # without a KL term the third result prefixes two keys only
    loss = CC.plug(CC.build(CP.LPIPSWithDiscriminator, name, lpips_weights=vgg_state), t)
    rec, last, _ = CC.reconstructions(t, True)
    post = D.DiagonalGaussianDistribution(t["posterior"])
    value, log, dic = loss(t["inputs"], rec, post, 0, 50, last_layer=last, return_dic=True)
    assert _same_bits(value.detach(), golden[name + "_loss"])
    assert list(log) == ["train/" + k for k in ("total_loss", "logvar", "nll_loss", "rec_loss", "d_weight", "disc_factor",
                                                "g_loss")]
    assert set(dic) == {"train/total_loss", "train/logvar", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss"}
    assert all(_same_bits(dic[k if k in dic else k.split("/")[1]], v) for k, v in log.items())
    assert loss(t["inputs"], rec, post, 2, 50) is None
    # `disc_loss` is read when the module is called: a module built with "vanilla" and handed the hinge function
    loss.disc_loss = CP.hinge_d_loss
    got, _ = loss(t["inputs"], rec, post, 1, 150)
    assert _same_bits(got.detach(), golden["disc_hinge_kl_late_loss"])
    # what `from ssl_amd.losses.contperceptual import *` gives a file that took these names from taming
    names = {}
    exec("from ssl_amd.losses.contperceptual import *", names)
    for wanted in ("LPIPS", "NLayerDiscriminator", "weights_init", "hinge_d_loss", "vanilla_d_loss", "adopt_weight",
                   "LPIPSWithDiscriminator"):
        assert wanted in names, wanted
    assert names["LPIPS"] is LP.LPIPS


def test_distributions_reproduce_the_reference(golden):
    p = D.DiagonalGaussianDistribution(golden["in_posterior"])
    q = D.DiagonalGaussianDistribution(golden["in_posterior"].flip(0) * 0.7)
    torch.manual_seed(5)
    got = {"dist_sample": p.sample(), "dist_kl": p.kl(), "dist_kl_other": p.kl(q), "dist_nll": p.nll(q.mean),
           "dist_mode": p.mode(), "dist_std": p.std, "dist_var": p.var,
           "normal_kl": D.normal_kl(p.mean, p.logvar, q.mean, 0.3)}
    d = D.DiagonalGaussianDistribution(golden["in_posterior"], deterministic=True)
    got["dist_det_kl"], got["dist_det_sample"] = d.kl(), d.sample()
    for key, value in got.items():
        assert _same_bits(value, golden[key]), key
    assert float(p.logvar.max()) <= 20 and float(p.logvar.min()) >= -30
    assert isinstance(D.DiracDistribution(3).sample(), int) and D.DiracDistribution(3).mode() == 3
