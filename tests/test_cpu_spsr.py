"""The restatement and bound of SPSR's gradient map and its losses (tests/spsr_reference.py) against the reference's
recorded results (tests/golden/f33_spsr.npz, written by make_golden_spsr.py) and against fp64 autograd, and what of
ssl_amd.losses.spsr, ssl_amd.engine and the C ABI can be checked without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spsr_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f33_spsr.npz")
N = int(np.prod(R.FIXTURE_SHAPE))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _leaf(t):
    return t.clone().requires_grad_(True)


def test_fixture_holds_numbers_only_and_stays_small(golden):
    assert all(v.dtype == torch.float32 for v in golden.values())
    assert os.path.getsize(GOLDEN) < 128 * 1024
    assert len(R.PIXEL_CASES) == 12
    assert sum(1 for k in golden if k.endswith("_loss")) == len(R.PIXEL_CASES) + 2 and "sr_loss_map" in golden
    for k, v in R.fixture_inputs().items():
        assert torch.equal(golden[k], v), k
    # the reference's two classes are one arithmetic
    assert torch.equal(golden["map_gt"], golden["nopad_gt"]) and torch.equal(golden["map_grad"], golden["nopad_grad"])


def test_every_recorded_result_lies_within_the_bound(golden):
    sr, gt, cot = golden["sr"], golden["gt"], golden["cot"]
    shares = {}

    def hold(name, got, want, bound):
        shares[name] = max(shares.get(name, 0.0), R.share(got, want, bound))

    hold("map", golden["map_sr"], R.gmap(sr), R.map_bound(sr))
    hold("map", golden["map_gt"], R.gmap(gt), R.map_bound(gt))
    hold("map gradient", golden["map_grad"], R.adjoint(sr, cot)[0], R.adjoint_bound(sr, cot))
    for key, g_map in (("", None), ("_map", cot)):
        want = R.gradient_loss(sr, gt, "mse", 0.0, R.W_GRADSR / N, g_map=g_map)
        hold("line 363 loss", golden["sr_loss" + key], want.loss, want.loss_bound(reference_sum=True))
        hold("line 363 gradient", golden["sr_grad" + key], want.grad, want.grad_bound)
    want = R.branch_loss(golden["branch"], gt, "l1", 0.0, R.W_BRANCH / N)
    hold("line 368 loss", golden["br_loss"], want.loss, want.loss_bound(reference_sum=True))
    hold("line 368 gradient", golden["br_grad"], want.grad, want.grad_bound)
    for k, (name, reduction, weighted) in enumerate(R.PIXEL_CASES):
        if reduction != "none" and not weighted:
            want = R.pixel(sr, gt, R.PIXEL_KIND[name], R.PIXEL_EPS, R.scale_of(reduction, R.PIXEL_WEIGHT, N))
            hold("criterion loss", golden[f"c{k}_loss"], want.loss, want.loss_bound(reference_sum=True))
            hold("criterion gradient", golden[f"c{k}_grad"], want.grad, want.grad_bound)
    for name, s in shares.items():
        print(f"{name}: the reference uses at most {s:.3e} of the bound")
    assert len(shares) == 8 and max(shares.values()) <= 1.0
    assert min(shares.values()) > 0.0          # (a bound nothing comes near would hold anything)


@pytest.mark.parametrize("shape", [(2, 3, 9, 11), (1, 1, 1, 7), (1, 2, 7, 1), (1, 1, 1, 1), (3, 2, 2)])
def test_the_restated_adjoint_is_the_transpose_of_the_restated_jacobian(shape):
    g = torch.Generator().manual_seed(7)
    x, u, w = (torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(3))
    lhs, rhs = float((R.jvp(x, u) * w).sum()), float((u * R.adjoint(x, w)[0]).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, float((R.jvp(x, u) * w).abs().sum()))
    # and the Jacobian is the map's: a central difference in fp64
    h = 1e-6
    fd = (R.gmap(x + h * u) - R.gmap(x - h * u)) / (2 * h)
    assert float((fd - R.jvp(x, u)).abs().max()) <= 1e-5 * max(1.0, float(R.jvp(x, u).abs().max()))


@pytest.mark.parametrize("kind", R.KINDS)
def test_restated_losses_equal_fp64_autograd_through_the_torch_expressions(golden, kind):
    from ssl_amd.losses import spsr as M
    eps = float(np.float32(1e-4))          # (an eps whose fp32 rounding is itself: the restatement rounds it)
    sr, gt, cot, br = (golden[k].double() for k in ("sr", "gt", "cot", "branch"))
    s = 0.3 / N
    x = _leaf(sr)
    m = M._torch_map(x)
    loss = M._torch_criterion(kind, m, M._torch_map(gt), None, eps, 0.3, "mean")
    (loss + (m * cot).sum()).backward()
    want = R.gradient_loss(sr, gt, kind, eps, s, g_map=cot)
    # (torch's fp64 map adds the double 1e-6, the restatement the fp32 value of it: 2.6e-14 apart under the root)
    assert abs(float(loss.detach()) - float(want.loss)) <= 1e-9 * abs(float(want.loss))
    assert float((x.grad - want.grad).abs().max()) <= 1e-8 * float(want.grad.abs().max())
    b = _leaf(br)
    loss = M._torch_criterion(kind, b, M._torch_map(gt), None, eps, 0.3, "sum")
    loss.backward()
    want = R.branch_loss(br, gt, kind, eps, 0.3)
    assert abs(float(loss.detach()) - float(want.loss)) <= 1e-9 * abs(float(want.loss))
    assert float((b.grad - want.grad).abs().max()) <= 1e-8 * float(want.grad.abs().max())
    p = _leaf(sr)
    M._torch_criterion(kind, p, gt, None, eps, 0.3, "mean").backward()
    want = R.pixel(sr, gt, kind, eps, s)
    assert float((p.grad - want.grad).abs().max()) <= 1e-12 * float(want.grad.abs().max())


def test_torch_fallbacks_on_cpu_tensors_reproduce_the_fixture_bit_for_bit(golden):
    from ssl_amd import losses as L
    sr, gt, cot = golden["sr"], golden["gt"], golden["cot"]
    for cls, key in ((L.Get_gradient, "map"), (L.Get_gradient_nopadding, "nopad")):
        mod = cls()
        assert not list(mod.parameters()) and not list(mod.buffers())
        x = _leaf(sr)
        m = mod(x)
        (m * cot).sum().backward()
        assert torch.equal(m.detach(), golden["map_sr"]) and torch.equal(x.grad, golden[key + "_grad"])
        assert torch.equal(mod(gt), golden[key + "_gt"])
    # line 363 as the model writes it, then as one call, alone and with the map's second consumer
    x = _leaf(sr)
    loss = L.MSELoss(loss_weight=R.W_GRADSR)(L.Get_gradient()(x), L.Get_gradient()(gt))
    loss.backward()
    assert torch.equal(loss.detach(), golden["sr_loss"]) and torch.equal(x.grad, golden["sr_grad"])
    crit = L.GradientLoss("mse", loss_weight=R.W_GRADSR)
    x = _leaf(sr)
    loss = crit(x, gt)
    loss.backward()
    assert torch.equal(loss.detach(), golden["sr_loss"]) and torch.equal(x.grad, golden["sr_grad"])
    x = _leaf(sr)
    loss, m = crit(x, gt, return_map=True)
    (loss + (m * cot).sum()).backward()
    assert torch.equal(loss.detach(), golden["sr_loss_map"]) and torch.equal(m.detach(), golden["map_sr"])
    assert torch.equal(x.grad, golden["sr_grad_map"])
    # line 368
    for run in (lambda b: L.L1Loss(loss_weight=R.W_BRANCH)(b, L.Get_gradient_nopadding()(gt)),
                lambda b: L.GradientLoss("l1", loss_weight=R.W_BRANCH).branch(b, gt)):
        b = _leaf(golden["branch"])
        loss = run(b)
        loss.backward()
        assert torch.equal(loss.detach(), golden["br_loss"]) and torch.equal(b.grad, golden["br_grad"])
    # the criteria, every reduction, with and without a weight
    for k, (name, reduction, weighted) in enumerate(R.PIXEL_CASES):
        kw = dict(eps=R.PIXEL_EPS) if name == "CharbonnierLoss" else {}
        crit = getattr(L, name)(loss_weight=R.PIXEL_WEIGHT, reduction=reduction, **kw)
        x = _leaf(sr)
        loss = crit(x, gt, weight=golden["weight"] if weighted else None)
        loss.sum().backward()
        assert torch.equal(loss.detach(), golden[f"c{k}_loss"]) and torch.equal(x.grad, golden[f"c{k}_grad"]), (k, name)


def test_constructors_follow_the_reference():
    from ssl_amd import losses as L
    for cls in (L.MSELoss, L.CharbonnierLoss, L.GradientLoss):
        with pytest.raises(ValueError, match="Unsupported reduction mode: batchmean"):
            cls(reduction="batchmean")
    assert (L.MSELoss().loss_weight, L.MSELoss().reduction) == (1.0, "mean")
    c = L.CharbonnierLoss(0.5, "sum", 1e-6)
    assert (c.loss_weight, c.reduction, c.eps) == (0.5, "sum", 1e-6) and L.CharbonnierLoss().eps == 1e-12
    g = L.GradientLoss()
    assert (g.criterion, g.loss_weight, g.reduction, g.eps) == ("mse", 1.0, "mean", 1e-12)
    with pytest.raises(ValueError):
        L.GradientLoss("huber")
    x = torch.rand(1, 4, 5, 6)           # any C, not only 3; extra keyword arguments are accepted as the reference's
    assert L.Get_gradient()(x).shape == x.shape
    assert float(L.MSELoss()(x, x * 0.5, unused=1)) > 0
    from ssl_amd import engine
    with pytest.raises(RuntimeError, match="GPU"):
        engine.gradient_map(x)           # the engine itself has no CPU path; the classes choose the torch expressions


# -------------------------------------------------------------------------------------------------- host checks ---
NAMES = ("ssg_spsr_workspace_bytes", "ssg_spsr_grid_cap", "ssg_spsr_map", "ssg_spsr_map_backward", "ssg_spsr_loss",
         "ssg_spsr_loss_backward", "ssg_spsr_branch_loss", "ssg_spsr_branch_grad", "ssg_pixel_sums", "ssg_pixel_grad")
FAKE = [ctypes.c_void_p(k << 20) for k in range(1, 7)]     # non-null, aligned addresses a refused call never touches


def _declaration(hdr, name):
    m = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
    assert m, name
    text = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in text.split(",") if a.strip() != "void"]


def test_symbols_exported_declared_and_bound():
    from ssl_amd import _lib, losses
    from ssl_amd.losses import spsr as M
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.HEADER).read()
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    for name in NAMES:
        assert hasattr(L, name)
        res, args = _lib.PROTOTYPES[name]
        decl = _declaration(hdr, name)
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):
            want = ctypes.c_void_p if ("*" in d or d.startswith("ssg_stream_t")) else kinds[d.split()[0]]
            assert a is want, (name, d)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
    assert L.ssg_abi_version() == 6
    assert [_lib.CONSTANTS["SSG_PIX_" + k] for k in ("L1", "MSE", "CHARBONNIER")] == [0, 1, 2]
    for name in ("Get_gradient", "Get_gradient_nopadding", "GradientLoss", "MSELoss", "CharbonnierLoss"):
        assert getattr(losses, name) is getattr(M, name) and name in M.__all__
    from ssl_amd import engine
    for name in ("gradient_map", "gradient_loss", "gradient_branch_loss"):
        assert callable(getattr(engine, name))


def test_workspace_follows_the_grid_cap_and_the_trip_shape_follows_both():
    """spsr_cases.py's largest shape is computed from the exported cap: every workgroup of the capped grid walks a
    second time and a scalar tail remains."""
    from ssl_amd import _lib
    import spsr_cases as C
    L = _lib.lib()
    cap = L.ssg_spsr_grid_cap()
    assert cap >= 1 and L.ssg_spsr_workspace_bytes() == 8 * cap
    n = int(np.prod(C.trip_shape(cap)))
    per = C.WORKGROUP * C.PER_THREAD
    assert (2 * cap - 1) * per < n < 2 ** 31 and n % C.PER_THREAD != 0
    assert n * 4 <= 64 << 20                                     # a few megabytes: the test stays quick


def test_c_abi_refuses_before_any_launch():
    from ssl_amd import _lib
    L = _lib.lib()
    BAD, ALIGN = -1, -5
    a, b, c, out, work, coef = FAKE
    odd = ctypes.c_void_p((1 << 20) + 2)
    half = ctypes.c_void_p((5 << 20) + 4)

    ALL = ("map", "map_backward", "loss", "loss_backward", "branch_loss", "branch_grad")
    WITH_KIND = ALL[2:]

    def plane_calls(only, planes=6, H=9, W=11, kind=1, eps=1e-12, p=a, q=b, r=out, w=work, k=coef, m=c):
        """The statuses of the plane entry points named in `only` for one set of arguments.  Only calls that must be
        refused are ever made: the addresses are fakes, and a call that passed the checks would launch on them."""
        calls = {"map": lambda: L.ssg_spsr_map(p, planes, H, W, r, None),
                 "map_backward": lambda: L.ssg_spsr_map_backward(p, q, planes, H, W, r, None),
                 "loss": lambda: L.ssg_spsr_loss(p, q, planes, H, W, kind, eps, m, w, r, None),
                 "loss_backward": lambda: L.ssg_spsr_loss_backward(p, q, m, k, planes, H, W, kind, eps, r, None),
                 "branch_loss": lambda: L.ssg_spsr_branch_loss(p, q, planes, H, W, kind, eps, w, r, None),
                 "branch_grad": lambda: L.ssg_spsr_branch_grad(p, q, planes, H, W, kind, eps, k, r, None)}
        return {calls[name]() for name in only}

    def flat_calls(only=("pixel_sums", "pixel_grad"), n=70, kind=1, eps=1e-12, p=a, q=b, r=out, w=work, k=coef):
        calls = {"pixel_sums": lambda: L.ssg_pixel_sums(p, q, n, kind, eps, w, r, None),
                 "pixel_grad": lambda: L.ssg_pixel_grad(p, q, n, kind, eps, k, r, None)}
        return {calls[name]() for name in only}

    for bad in (dict(planes=0), dict(H=0), dict(W=-3), dict(planes=1 << 11, H=1 << 10, W=1 << 10),
                dict(planes=46341, H=46341, W=1), dict(p=None), dict(r=None)):
        assert plane_calls(ALL, **bad) == {BAD}, bad
    for bad in (dict(kind=-1), dict(kind=3), dict(eps=-1e-12), dict(eps=float("nan")), dict(eps=float("inf"))):
        assert plane_calls(WITH_KIND, **bad) == {BAD}, bad
        assert flat_calls(**bad) == {BAD}, bad
    for bad in (dict(n=0), dict(p=None), dict(q=None), dict(r=None)):
        assert flat_calls(**bad) == {BAD}, bad
    assert plane_calls(WITH_KIND + ("map_backward",), q=None) == {BAD}
    assert plane_calls(("loss", "branch_loss"), w=None) == {BAD}
    assert plane_calls(("loss_backward", "branch_grad"), k=None) == {BAD}
    assert flat_calls(("pixel_sums",), w=None) == {BAD} and flat_calls(("pixel_grad",), k=None) == {BAD}
    # just under 2^31 elements passes the size check (and is then refused for its alignment, still before a launch)
    assert L.ssg_spsr_map(odd, (1 << 11) - 1, 1 << 10, 1 << 10, out, None) == ALIGN
    assert plane_calls(ALL, p=odd) == {ALIGN} and flat_calls(q=odd) == {ALIGN}
    assert plane_calls(("loss", "branch_loss"), w=half) == {ALIGN}
    assert plane_calls(("loss_backward", "branch_grad"), k=half) == {ALIGN}
    assert L.ssg_spsr_loss(a, b, 6, 9, 11, 1, 0.0, c, work, half, None) == ALIGN
    # two things wrong at once: null pointers, then the shape, then kind and eps, then every alignment
    for bad in (dict(planes=0), dict(W=-3), dict(planes=1 << 11, H=1 << 10, W=1 << 10)):
        assert plane_calls(ALL, p=odd, **bad) == {BAD}, bad
        assert plane_calls(("loss", "branch_loss"), w=half, **bad) == {BAD}, bad
    for bad in (dict(kind=3), dict(eps=float("nan"))):
        assert plane_calls(WITH_KIND, p=odd, **bad) == {BAD}, bad
        assert flat_calls(q=odd, **bad) == {BAD}, bad
    assert plane_calls(ALL, p=odd, r=None) == {BAD} and plane_calls(ALL, p=None, r=odd) == {BAD}
    assert flat_calls(p=odd, n=0) == {BAD} and flat_calls(p=odd, r=None) == {BAD}
    assert plane_calls(("loss_backward", "branch_grad"), p=odd, k=None) == {BAD}
