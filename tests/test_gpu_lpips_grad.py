"""ssg_lpips_layers_backward (ssl_amd/csrc/ssg_featmetric.hip, include/ssg_hip.h section (V)) on synthetic feature sets
against the fp64 restatement of tests/lpips_grad_reference.py within its per-element bound; the values it must hold
exactly (+-0 on identical inputs, NaN at all-zero vectors and nowhere else, a NaN input inside its image), its
reproducibility, either side alone, every 4-byte offset with guarded outputs; the autograd node (two backward passes over
one graph); and end to end: the native LPIPS on a random-weight VGG16 and LPIPSWithDiscriminator on the fixture's cases,
each measured against the same lines in fp64 beside torch's fp32 lines on the same GPU."""
import copy
import os

import numpy as np
import pytest
import torch

import contperceptual_cases as CC
import featmetric_cases as FC
import lpips_grad_cases as C
import lpips_grad_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f37_contperceptual.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _L():
    from ssl_amd import _lib
    return _lib.lib()


def _geometry():
    L = _L()
    return L.ssg_featmetric_unit(), L.ssg_featmetric_grid_cap()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _to(ts, dev):
    return [t.to(dev) for t in ts]


NAMES = [c[0] for c in C.cases(256, 1024)]
_sets = {}


def grad_set(name, dev):
    """(cpu inputs, device inputs, restatement) of one case, computed once and left unchanged"""
    if name not in _sets:
        _, N, layers, content = next(c for c in C.cases(*_geometry()) if c[0] == name)
        f0, f1, w, coef = C.maps(N, layers, content)
        _sets[name] = ((f0, f1, w, coef), (_to(f0, dev), _to(f1, dev), _to(w, dev), coef.to(dev)),
                       R.lpips_grad(f0, f1, w, coef))
    return _sets[name]


# ---------------------------------------------------------------------------------- against the restatement ---
@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_the_restatement(dev, name):
    from ssl_amd import metrics_feat as MF
    _, (f0, f1, w, coef), ref = grad_set(name, dev)
    g0, g1 = MF.lpips_layers_backward(f0, f1, w, coef, True, True)
    worst = 0.0
    for k, r in enumerate(ref):
        a, b = g0[k].cpu(), g1[k].cpu()
        assert a.shape == f0[k].shape and a.dtype == torch.float32
        # NaN on a side's C elements of the pixels whose own vector is all zero, and nowhere else
        assert (R.nan_pattern(a) == np.broadcast_to(r.nan0, r.g0.shape)).all(), (name, k)
        assert (R.nan_pattern(b) == np.broadcast_to(r.nan1, r.g1.shape)).all(), (name, k)
        s0, s1 = R.share(a, r.g0, r.bound0, skip=r.nan0), R.share(b, r.g1, r.bound1, skip=r.nan1)
        worst = max(worst, s0, s1)
        assert s0 <= 1.0 and s1 <= 1.0, (name, k, s0, s1)
        if "identical" in name:
            assert not r.nan0.any() and bool(((_bits(a) & 0x7FFFFFFF) == 0).all() and ((_bits(b) & 0x7FFFFFFF) == 0).all())
        if "near" in name and f0[k].shape[1] >= 64:       # (one channel normalises to 1 whatever its value: no gradient)
            # the case an fp32 evaluation fails: u times the summed terms is far outside the bound
            with np.errstate(divide="ignore"):
                assert float(np.median(r.bound0 / np.abs(r.g0))) < 1e-5 and float(np.abs(r.g0).max()) > 0
    print(f"lpips grad {name}: the kernel uses {worst:.3g} of the bound")
    if "second_trip" in name:
        unit, cap = _geometry()
        assert -(-(f0[0].shape[2] * f0[0].shape[3]) // unit) == cap + 1
    if "relu" in name and len(ref) > 1:
        assert any(r.nan0.any() for r in ref) and any(r.nan1.any() for r in ref)


def test_either_side_alone(dev):
    from ssl_amd import metrics_feat as MF
    _, (f0, f1, w, coef), _ = grad_set("k5_n3_relu", dev)
    g0, g1 = MF.lpips_layers_backward(f0, f1, w, coef, True, True)
    a0, a1 = MF.lpips_layers_backward(f0, f1, w, coef, True, False)
    b0, b1 = MF.lpips_layers_backward(f0, f1, w, coef, False, True)
    assert a1 is None and b0 is None
    for k in range(len(f0)):
        assert torch.equal(_bits(a0[k]), _bits(g0[k])) and torch.equal(_bits(b1[k]), _bits(g1[k])), k
    with pytest.raises(ValueError):
        MF.lpips_layers_backward(f0, f1, w, coef, False, False)


def test_bits_repeat_batch_and_layer_set(dev):
    from ssl_amd import metrics_feat as MF
    _, (f0, f1, w, coef), _ = grad_set("k5_n3_relu", dev)
    K = len(f0)
    full = MF.lpips_layers_backward(f0, f1, w, coef)
    again = MF.lpips_layers_backward(f0, f1, w, coef)
    for side in (0, 1):
        for k in range(K):
            assert torch.equal(_bits(full[side][k]), _bits(again[side][k])), (side, k)                    # a repeat
    for n in range(3):                                                                                  # image n alone
        alone = MF.lpips_layers_backward([t[n:n + 1].clone() for t in f0], [t[n:n + 1].clone() for t in f1], w,
                                         coef[n:n + 1].clone())
        for side in (0, 1):
            for k in range(K):
                assert torch.equal(_bits(alone[side][k][0]), _bits(full[side][k][n])), (n, side, k)
    for k in range(K):                                                                                  # layer k alone
        alone = MF.lpips_layers_backward([f0[k]], [f1[k]], [w[k]], coef)
        assert torch.equal(_bits(alone[0][0]), _bits(full[0][k])) and torch.equal(_bits(alone[1][0]), _bits(full[1][k])), k


def test_nan_input_stays_inside_its_image(dev):
    from ssl_amd import metrics_feat as MF
    _, (f0, f1, w, coef), _ = grad_set("k5_n3_relu", dev)
    clean = MF.lpips_layers_backward(f0, f1, w, coef)
    bad = [t.clone() for t in f0]
    bad[2][1, 7, 3, 2] = float("nan")
    got = MF.lpips_layers_backward(bad, f1, w, coef)
    for side in (0, 1):
        for k in range(len(f0)):
            same = _bits(got[side][k]) == _bits(clean[side][k])
            if k == 2:
                assert bool(torch.isnan(got[side][k][1, :, 3, 2]).all())
                same[1, :, 3, 2] = True
            assert bool(same.all()), (side, k)


SENTINEL = -7.0


def _guarded(t, off, fill=None):
    """a copy of t (or `fill` in its shape) at a 4-byte offset `off` floats into a buffer of sentinels: (buffer, view)"""
    buf = torch.full((t.numel() + 8,), SENTINEL, dtype=torch.float32, device=t.device)
    view = buf[off:off + t.numel()].view(t.shape)
    if fill is None:
        view.copy_(t)
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 == (4 * off) % 16 and view.is_contiguous()
    return buf, view


def _raw(f0, f1, w, coef, g0, g1):
    from ssl_amd.engine import address_array
    L = _L()
    K, N = len(f0), f0[0].shape[0]
    Cs, H, W = (np.ascontiguousarray([t.shape[i] for t in f0], dtype=np.int32) for i in (1, 2, 3))
    arr = lambda ts: None if ts is None else address_array([t.data_ptr() for t in ts])
    a = [arr(ts) for ts in (f0, f1, w, g0, g1)]
    p = [None if x is None else x.ctypes.data for x in a]
    return L.ssg_lpips_layers_backward(K, N, p[0], p[1], p[2], Cs.ctypes.data, H.ctypes.data, W.ctypes.data,
                                       coef.data_ptr() if coef is not None else None, p[3], p[4],
                                       torch.cuda.current_stream().cuda_stream)


def test_every_offset_guarded_outputs_and_refusals(dev):
    from ssl_amd import _lib, metrics_feat as MF
    E = _lib.CONSTANTS
    _, (f0, f1, w, coef), _ = grad_set("k5_n3_relu", dev)
    want = MF.lpips_layers_backward(f0, f1, w, coef)
    K = len(f0)
    for off in range(4):
        s0 = [_guarded(t, (off + k) % 4) for k, t in enumerate(f0)]
        s1 = [_guarded(t, (off + k + 1) % 4) for k, t in enumerate(f1)]
        sw = [_guarded(t, (off + k + 2) % 4) for k, t in enumerate(w)]
        sc = _guarded(coef, off)
        o0 = [_guarded(t, (off + k + 3) % 4, fill=SENTINEL) for k, t in enumerate(f0)]
        o1 = [_guarded(t, (off + 2 * k) % 4, fill=SENTINEL) for k, t in enumerate(f1)]
        views = lambda ps: [v for _, v in ps]
        # every refusal leaves the outputs untouched
        assert _raw(views(s0), views(s1), views(sw), None, views(o0), views(o1)) == E["SSG_E_BADARG"]
        assert _raw(views(s0), views(s1), views(sw), sc[1], None, None) == E["SSG_E_BADARG"]
        torch.cuda.synchronize()
        assert all(bool((b == SENTINEL).all()) for b, _ in o0 + o1)
        assert _raw(views(s0), views(s1), views(sw), sc[1], views(o0), views(o1)) == 0
        torch.cuda.synchronize()
        for k in range(K):
            for (buf, view), ref, o in ((o0[k], want[0][k], (off + k + 3) % 4), (o1[k], want[1][k], (off + 2 * k) % 4)):
                assert torch.equal(_bits(view), _bits(ref)), (off, k)
                assert bool((buf[:o] == SENTINEL).all()) and bool((buf[o + view.numel():] == SENTINEL).all()), (off, k)
        # the inputs are read only
        for (buf, view), t in zip(s0 + s1 + sw, list(f0) + list(f1) + list(w)):
            assert torch.equal(_bits(view), _bits(t))


# -------------------------------------------------------------------------------------------- the autograd node ---
def test_criterion_two_backward_passes_over_one_graph(dev):
    from ssl_amd import metrics_feat as MF
    from ssl_amd.losses import lpips as LP, set_native_criteria
    _, (f0, f1, w, coef), ref = grad_set("k5_n3_relu", dev)
    lins = [t.reshape(1, -1, 1, 1) for t in w]
    calls, saved = [], MF.lpips_layers_backward

    def spy(*args):
        calls.append(args[-2:])
        return saved(*args)

    MF.lpips_layers_backward = spy
    try:
        a = [t.clone().requires_grad_(True) for t in f0]
        out = LP.lpips_criterion(a, f1, lins)
        assert out.shape == (3, 1, 1, 1) and out.dtype == torch.float32
        assert torch.equal(_bits(out.detach().reshape(-1)), _bits(MF.lpips_layers(f0, f1, w)[:, -1].float()))
        total = (out.reshape(-1) * coef).sum()
        first = torch.autograd.grad(total, a, retain_graph=True)          # calculate_adaptive_weight's use
        total.backward()
        assert calls == [(True, False), (True, False)]                    # one launch each, side 0 alone
        direct = saved(f0, f1, w, coef, True, False)[0]
        for k in range(len(a)):
            assert torch.equal(_bits(first[k]), _bits(a[k].grad)) and torch.equal(_bits(first[k]), _bits(direct[k])), k
        # the other side alone, and both
        b = [t.clone().requires_grad_(True) for t in f1]
        (LP.lpips_criterion(f0, b, lins).reshape(-1) * coef).sum().backward()
        assert calls[-1] == (False, True)
        both = saved(f0, f1, w, coef, True, True)
        assert all(torch.equal(_bits(t.grad), _bits(g)) for t, g in zip(b, both[1]))
        n = len(calls)
        # a lin that requires grad, and the switch, send the call to the torch lines
        # (on two layers: each shape of the lines' convolution is one more search of the GPU library's)
        wl = [t.clone().requires_grad_(True) for t in lins[:2]]
        LP.lpips_criterion(a[:2], f1[:2], wl).sum().backward()
        assert all(t.grad is not None for t in wl) and len(calls) == n
        prev = set_native_criteria(False)
        try:
            lines = LP.lpips_criterion(a[:2], f1[:2], lins[:2])
        finally:
            set_native_criteria(prev)
        assert "Lpips" not in type(lines.grad_fn).__name__ and len(calls) == n
        assert torch.allclose(lines, MF.lpips_torch_lines(a[:2], f1[:2], lins[:2]), rtol=1e-5, atol=0)
    finally:
        MF.lpips_layers_backward = saved


# ---------------------------------------------------------------------------------------------- end to end ---
def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _measure(native, lines, ref):
    """(native error, the fp32 lines' own error, one fp32 ulp of the reference's maximum) of one result"""
    ref = ref.detach().double().cpu()
    en = float((native.detach().double().cpu() - ref).abs().max())
    el = float((lines.detach().double().cpu() - ref).abs().max())
    return en, el, _ulp(ref.abs().max())


def test_native_lpips_against_fp64_on_a_random_vgg16(dev):
    from ssl_amd import metrics_feat as MF
    from ssl_amd.losses import lpips as LP, set_native_criteria
    net = LP.LPIPS(FC.lpips_state('vgg')[0]).to(dev)
    net64 = copy.deepcopy(net).double()
    x, y = (t.to(dev) for t in C.images((2, 3, 32, 32)))
    calls, saved = [], MF.lpips_layers_backward

    def spy(*args):
        calls.append(1)
        return saved(*args)

    def grad_of(module, a, b):
        a = a.clone().requires_grad_(True)
        out = module(a, b)
        out.sum().backward()
        return out.detach(), a.grad

    MF.lpips_layers_backward = spy
    try:
        v_n, g_n = grad_of(net, x, y)
        assert len(calls) == 1                                   # the hot path took the kernel, once
        prev = set_native_criteria(False)
        try:
            v_l, g_l = grad_of(net, x, y)
        finally:
            set_native_criteria(prev)
        assert len(calls) == 1
    finally:
        MF.lpips_layers_backward = saved
    v_r, g_r = grad_of(net64, x.double(), y.double())
    assert bool(torch.isfinite(g_r).all()) and float(g_r.abs().max()) > 0
    for what, (en, el, ulp) in (("value", _measure(v_n, v_l, v_r)), ("image gradient", _measure(g_n, g_l, g_r))):
        print(f"lpips end to end, {what}: native error {en:.3g}, torch fp32 lines' error {el:.3g}, one ulp of the maximum "
              f"{ulp:.3g}: native / (2 lines + ulp) = {en / (2 * el + ulp):.3g}")
        assert en <= 2 * el + ulp, (what, en, el, ulp)


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


def _criterion_runs(dev, name, t, plug_stand_ins, state):
    """(native on the GPU, fp32 lines on the GPU, fp64 lines on the CPU) of one case"""
    from ssl_amd import distributions as D
    from ssl_amd.losses import contperceptual as CP, set_native_criteria

    def module(dtype, device):
        loss = CC.build(CP.LPIPSWithDiscriminator, name, lpips_weights=state)
        if plug_stand_ins:
            return CC.plug(loss, t, dtype, device)
        torch.manual_seed(3)
        loss.discriminator = CC.StandInDiscriminator().apply(CP.weights_init)
        with torch.no_grad():
            for p in loss.discriminator.parameters():
                p.mul_(20.0)
        return loss.to(device=device, dtype=dtype)

    native = CC.run_case(module(torch.float32, dev), D.DiagonalGaussianDistribution, t, name, torch.float32, dev)
    prev = set_native_criteria(False)
    try:
        lines = CC.run_case(module(torch.float32, dev), D.DiagonalGaussianDistribution, t, name, torch.float32, dev)
    finally:
        set_native_criteria(prev)
    ref = CC.run_case(module(torch.float64, "cpu"), D.DiagonalGaussianDistribution, t, name, torch.float64, "cpu")
    return native, lines, ref


def _hold(name, native, lines, ref):
    assert set(native) == set(lines) == set(ref), (sorted(native), sorted(ref))
    for key in sorted(ref):
        en, el, ulp = _measure(native[key], lines[key], ref[key])
        print(f"criterion {name} {key}: native error {en:.3g}, torch fp32 lines' error {el:.3g}, ulp {ulp:.3g}: "
              f"native / (2 lines + ulp) = {en / (2 * el + ulp) if el + ulp > 0 else 0.0:.3g}")
        assert native[key].shape == ref[key].shape
        assert en <= 2 * el + ulp, (name, key, en, el, ulp)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_criterion_on_the_gpu_against_its_cpu_lines_in_fp64(dev, golden, name):
    from ssl_amd import engine
    from ssl_amd.losses import gan_loss
    t = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    calls, saved = [], (engine.pixel_loss, gan_loss._sums)
    engine.pixel_loss = lambda *a, **k: (calls.append("pixel"), saved[0](*a, **k))[1]
    gan_loss._sums = lambda *a, **k: (calls.append("gan"), saved[1](*a, **k))[1]
    try:
        native, lines, ref = _criterion_runs(dev, name, t, True, FC.lpips_state('vgg')[0])
    finally:
        engine.pixel_loss, gan_loss._sums = saved
    # the native run went through the kernels (the generator: L1 and -mean(logits); the discriminator: its two terms),
    # the other two through none
    assert calls == (["pixel", "gan"] if CC.CASES[name][0] == 0 else ["gan", "gan"]), calls
    _hold(name, native, lines, ref)


def test_discriminator_criterion_is_chosen_at_the_call(dev, golden):
    """a module built with "hinge" and handed `vanilla_d_loss` afterwards takes the vanilla kernels, not the hinge ones"""
    from ssl_amd import distributions as D
    from ssl_amd.losses import contperceptual as CP, gan_loss
    t = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    built = {}
    for kind in ("hinge", "vanilla"):
        name = f"disc_{kind}_{'kl' if kind == 'hinge' else 'nokl'}_late"
        built[kind] = CC.plug(CC.build(CP.LPIPSWithDiscriminator, name, lpips_weights=FC.lpips_state('vgg')[0]), t,
                              torch.float32, dev)
    built["hinge"].disc_loss = CP.vanilla_d_loss
    kinds, saved = [], gan_loss._sums
    gan_loss._sums = lambda x, spec, *a: (kinds.append(spec[0]), saved(x, spec, *a))[1]
    try:
        got = CC.run_case(built["hinge"], D.DiagonalGaussianDistribution, t, "disc_vanilla_nokl_late", torch.float32, dev)
        want = CC.run_case(built["vanilla"], D.DiagonalGaussianDistribution, t, "disc_vanilla_nokl_late", torch.float32, dev)
    finally:
        gan_loss._sums = saved
    assert kinds == [gan_loss.SOFTPLUS] * 4, kinds
    assert torch.equal(_bits(got["loss"]), _bits(want["loss"]))
    built["hinge"].disc_loss = lambda real, fake: CP.hinge_d_loss(real, fake)      # not a criterion the kernels express
    kinds.clear()
    lines = CC.run_case(built["hinge"], D.DiagonalGaussianDistribution, t, "disc_hinge_kl_late", torch.float32, dev)
    assert kinds == [] and bool(torch.isfinite(lines["loss"]))


def test_criterion_with_the_native_lpips_inside(dev, golden):
    """the generator's pass with ssl_amd.losses.lpips.LPIPS itself (random-weight VGG16) as the perceptual term: the L1
    kernel, the LPIPS kernels each way (twice backward: the adaptive weight and backward()) and the GAN kernel"""
    from ssl_amd import metrics_feat as MF
    t = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    calls, saved = [], MF.lpips_layers_backward
    MF.lpips_layers_backward = lambda *a: (calls.append(a[-2:]), saved(*a))[1]
    try:
        native, lines, ref = _criterion_runs(dev, "gen_hinge_kl_late", t, False, FC.lpips_state('vgg')[0])
    finally:
        MF.lpips_layers_backward = saved
    assert calls == [(False, True), (False, True)], calls
    _hold("gen_hinge_kl_late (native LPIPS)", native, lines, ref)


# ---------------------------------------------------------------------------------------------- LDS poison ---
def poison_cases():
    """every output of the gradient kernel on every case, the second grid trip included (the one case in which a
    workgroup writes `sh` again, trip after trip), for test_gpu_lpips_grad_poison.py"""
    from ssl_amd import metrics_feat as MF
    dev = torch.device("cuda:0")
    out = []
    for name in NAMES:
        _, (f0, f1, w, coef), _ = grad_set(name, dev)
        g0, g1 = MF.lpips_layers_backward(f0, f1, w, coef)
        out += g0 + g1
    return out
