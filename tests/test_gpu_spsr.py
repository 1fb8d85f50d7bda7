"""SPSR's gradient map, its adjoint, the fused gradient-space losses and the streaming pixel criteria on the MI355X
(ssl_amd/csrc/ssg_spsr.hip) against the fp64 restatement tests/spsr_reference.py, every element, within its bound; the
largest share of each bound is printed (profiles/spsr_parity.txt records a run)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import spsr_cases as C
import spsr_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f33_spsr.npz")
WEIGHT, UPSTREAM = 0.3, 1.7          # a loss weight and an upstream gradient that are not 1
EPS = {"l1": 0.0, "mse": 0.0, "charbonnier": 1e-12}
SHARES = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def hold(name, got, want, bound):
    s = R.share(got.detach().cpu(), want, bound)
    SHARES[name] = max(SHARES.get(name, 0.0), s)
    print(f"{name}: {s:.3e} of the bound")
    assert s <= 1.0, (name, s)


def _leaf(t):
    return t.detach().requires_grad_(True)


def run_case(xc, tc, how, dev, kinds=R.KINDS, reduction="mean", check=True):
    """Every entry point of the family on the pair (xc, tc), laid out on the device as `how` says; held to the
    restatement when `check`; returns the outputs (for the bit comparisons of repeat calls and of the LDS poison)."""
    from ssl_amd import engine
    hx, ht = ("plain", "view") if how == "mixed" else (how, how)     # mixed: the target alone sits off a boundary
    x, t = C.place(xc, hx, dev), C.place(tc, ht, dev)
    n = xc.numel()
    s = R.scale_of(reduction, WEIGHT, n)
    cotc, brc = C.cotangent(xc.shape), C.branch_for(tc)
    cot, br = cotc.to(dev), C.place(brc, hx, dev)
    outs = []
    keep = (lambda *ts: outs.extend(v.detach().clone() for v in ts))
    held = hold if check else (lambda *a: None)
    # the map and its adjoint
    xl = _leaf(x)
    m = engine.gradient_map(xl)
    m.backward(cot)
    keep(m, xl.grad)
    held("map", m, R.gmap(xc), R.map_bound(xc))
    held("map gradient", xl.grad, R.adjoint(xc, cotc)[0], R.adjoint_bound(xc, cotc))
    assert torch.equal(_bits(engine.gradient_map(t)), _bits(engine.gradient_map(t.clone())))
    for kind in kinds:
        eps = EPS[kind]
        # the fused SR-side loss, alone
        xl = _leaf(x)
        loss = engine.gradient_loss(xl, t, kind, eps, WEIGHT, reduction)
        loss.backward()
        keep(loss, xl.grad)
        want = R.gradient_loss(xc, tc, kind, eps, s)
        held(f"gradient loss {kind}", loss, want.loss, want.loss_bound())
        held(f"gradient loss {kind} gradient", xl.grad, want.grad, want.grad_bound)
        # ... with the map beside it: the same loss bits, the map op's bits, both paths in one backward launch
        xm = _leaf(x)
        loss2, m2 = engine.gradient_loss(xm, t, kind, eps, WEIGHT, reduction, want_map=True)
        assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(m2), _bits(m))
        (UPSTREAM * loss2 + (m2 * cot).sum()).backward()
        keep(xm.grad)
        want = R.gradient_loss(xc, tc, kind, eps, s, c=UPSTREAM * s, g_map=cotc)
        held(f"gradient loss {kind} gradient with g_map", xm.grad, want.grad, want.grad_bound)
        # ... and composed: the map op under the streaming criterion
        xk = _leaf(x)
        mk = engine.gradient_map(xk)
        assert torch.equal(_bits(mk), _bits(m))
        comp = engine.pixel_loss(mk, engine.gradient_map(t), kind, eps, WEIGHT, reduction)
        comp.backward()
        want = R.gradient_loss(xc, tc, kind, eps, s)
        held(f"composed loss {kind}", comp, want.loss, want.loss_bound())
        held(f"composed loss {kind} gradient", xk.grad, want.grad, want.grad_bound)
        # the branch-side loss
        bl = _leaf(br)
        loss = engine.gradient_branch_loss(bl, t, kind, eps, WEIGHT, reduction)
        (UPSTREAM * loss).backward()
        keep(loss, bl.grad)
        want = R.branch_loss(brc, tc, kind, eps, s, c=UPSTREAM * s)
        held(f"branch loss {kind}", loss, want.loss, want.loss_bound())
        held(f"branch loss {kind} gradient", bl.grad, want.grad, want.grad_bound)
        # the streaming criterion
        xl = _leaf(x)
        loss = engine.pixel_loss(xl, t, kind, eps, WEIGHT, reduction)
        loss.backward()
        keep(loss, xl.grad)
        want = R.pixel(xc, tc, kind, eps, s)
        held(f"pixel loss {kind}", loss, want.loss, want.loss_bound())
        held(f"pixel loss {kind} gradient", xl.grad, want.grad, want.grad_bound)
    return outs


@pytest.mark.parametrize("name", list(C.SHAPES))
def test_every_entry_point_on_the_smallest_shapes(dev, name):
    how = name if name in ("view", "strided", "mixed") else "plain"
    for seed, reduction in ((0, "mean"), (1, "sum")):
        xc, tc = C.content("uniform", C.SHAPES[name], seed)
        run_case(xc, tc, how, dev, reduction=reduction)


@pytest.mark.parametrize("name", [c for c in C.CONTENTS if c != "uniform"])
@pytest.mark.parametrize("shape", ["2x3x9x11", "1x3x5x65"])
def test_contents(dev, name, shape):
    from ssl_amd import engine
    xc, tc = C.content(name, C.SHAPES[shape])
    run_case(xc, tc, "plain", dev)
    x, t = xc.to(dev), tc.to(dev)
    if name == "flat":
        m = engine.gradient_map(x)
        assert bool((m[..., 1:-1, 1:-1] == float(np.sqrt(np.float32(1e-6), dtype=np.float32))).all())
        assert abs(float(m[0, 0, 2, 2]) - 1e-3) < 1e-9
        xl = _leaf(x)
        engine.gradient_map(xl).backward(C.cotangent(xc.shape).to(dev))
        assert bool((xl.grad[..., 2:-2, 2:-2] == 0).all()) and bool((xl.grad != 0).any())
    if name == "same":                     # the map difference is exactly 0: sign(0) = 0, nothing flows
        for kind in R.KINDS:
            xl = _leaf(x)
            loss = engine.gradient_loss(xl, t, kind, EPS[kind], WEIGHT)
            loss.backward()
            # (charbonnier's loss at d = 0 is sqrt(eps) per element, its derivative 0 / sqrt(eps) = 0)
            assert (float(loss.detach()) == 0.0 or kind == "charbonnier") and bool((xl.grad == 0).all()), kind
        cot = C.cotangent(xc.shape).to(dev)
        xa, xb = _leaf(x), _leaf(x)
        loss, m = engine.gradient_loss(xa, t, "l1", 0.0, WEIGHT, want_map=True)
        (loss + (m * cot).sum()).backward()
        engine.gradient_map(xb).backward(cot)
        assert torch.equal(_bits(xa.grad), _bits(xb.grad))


def test_a_plane_of_a_batch_is_the_plane_alone_bit_for_bit(dev):
    from ssl_amd import engine
    xc, tc = C.isolation_batch()
    cotc, brc = C.cotangent(xc.shape), C.branch_for(tc)

    def outputs(sel):
        x, t, cot, br = (v[:, sel].contiguous().to(dev) for v in (xc, tc, cotc, brc))
        outs = []
        xl = _leaf(x)
        m = engine.gradient_map(xl)
        m.backward(cot)
        outs += [m.detach(), xl.grad]
        for kind in R.KINDS:
            xl, bl = _leaf(x), _leaf(br)
            loss, m2 = engine.gradient_loss(xl, t, kind, 1e-12, WEIGHT, "sum", want_map=True)
            (loss + (m2 * cot).sum()).backward()
            engine.gradient_branch_loss(bl, t, kind, 1e-12, WEIGHT, "sum").backward()
            outs += [m2.detach(), xl.grad, bl.grad]
        return outs

    whole = outputs(slice(0, 3))
    hold("map", whole[0], R.gmap(xc), R.map_bound(xc))
    hold("map gradient", whole[1], R.adjoint(xc, cotc)[0], R.adjoint_bound(xc, cotc))
    for p in range(3):
        alone = outputs(slice(p, p + 1))
        for k, (a, b) in enumerate(zip(whole, alone)):
            assert torch.equal(_bits(a[:, p:p + 1]), _bits(b)), (p, k)


def test_a_second_grid_trip(dev):
    """A shape computed from the exported grid cap: every workgroup walks again and a tail remains.  Held to the
    restatement; the loss-only and the map-emitting forms are bit-equal (run_case asserts it)."""
    from ssl_amd import _lib
    shape = C.trip_shape(_lib.lib().ssg_spsr_grid_cap())
    xc, tc = C.content("uniform", shape, 3)
    run_case(xc, tc, "plain", dev, kinds=("mse",))
    run_case(xc, tc, "view", dev, kinds=("l1",), check=False)     # (its own asserts: loss and map bits of both forms)


@pytest.mark.parametrize("how", list(C.OFFSET_VIEWS))
def test_heads_and_tails_of_one_two_and_three(dev, how):
    """Eleven elements 1, 2 and 3 floats behind a 16-byte boundary: a scalar head of 3, 2 and 1, two groups of four, a
    tail of 0, 1 and 2, in every kernel built on the shared walk (the outputs are aligned: stored one by one)."""
    xc, tc = C.content("uniform", C.HEADS_SHAPE, 13)
    run_case(xc, tc, how, dev)


@pytest.mark.parametrize("how", list(C.OFFSET_VIEWS))
def test_offset_outputs_take_the_wide_stores_to_the_same_bits(dev, how):
    """Through the C ABI an output with the input's own misalignment is stored 16 bytes wide behind the scalar head, one
    a float further element by element: the same bits, nothing outside the eleven elements, and within the bound."""
    from ssl_amd import _lib
    L = _lib.lib()
    k, n = C.OFFSET_VIEWS[how], int(np.prod(C.HEADS_SHAPE))
    xc, tc = C.content("uniform", C.HEADS_SHAPE, 13)
    brc = C.branch_for(tc)
    x, t, br = (C.place(v, how, dev) for v in (xc, tc, brc))
    coef = torch.tensor([0.25], dtype=torch.float64, device=dev)
    work = torch.empty(L.ssg_spsr_workspace_bytes(), dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    H, W = C.HEADS_SHAPE[2:]
    calls = {
        "map": lambda o: L.ssg_spsr_map(x.data_ptr(), 1, H, W, o, stream),
        "loss map": lambda o: L.ssg_spsr_loss(x.data_ptr(), t.data_ptr(), 1, H, W, 1, 0.0, o, work.data_ptr(),
                                              total.data_ptr(), stream),
        "branch grad": lambda o: L.ssg_spsr_branch_grad(br.data_ptr(), t.data_ptr(), 1, H, W, 0, 0.0, coef.data_ptr(), o,
                                                        stream),
        "pixel grad": lambda o: L.ssg_pixel_grad(x.data_ptr(), t.data_ptr(), n, 2, 1e-12, coef.data_ptr(), o, stream),
    }
    outs = {}
    for name, call in calls.items():
        got = []
        for off in (k, (k + 1) % 4):           # the input's own offset: wide; a float further: one by one
            buf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
            _lib.check(call(buf[off:].data_ptr()))
            assert not bool(buf[:off].any()) and not bool(buf[off + n:].any()), (name, off)
            got.append(buf[off:off + n].clone())
        assert torch.equal(_bits(got[0]), _bits(got[1])), name
        outs[name] = got[0].view(C.HEADS_SHAPE)
    hold("map", outs["map"], R.gmap(xc), R.map_bound(xc))
    hold("map", outs["loss map"], R.gmap(xc), R.map_bound(xc))
    want = R.branch_loss(brc, tc, "l1", 0.0, 0.25)
    hold("branch loss l1 gradient", outs["branch grad"], want.grad, want.grad_bound)
    want = R.pixel(xc, tc, "charbonnier", 1e-12, 0.25)
    hold("pixel loss charbonnier gradient", outs["pixel grad"], want.grad, want.grad_bound)


def test_one_nan_pixel_reaches_its_four_neighbours_and_the_loss(dev):
    from ssl_amd import engine
    xc, tc = C.content("uniform", C.SHAPES["2x3x9x11"], 5)
    xc[1, 2, 4, 5] = float("nan")
    x, t = xc.to(dev), tc.to(dev)
    m = engine.gradient_map(x)
    where = torch.isnan(m).nonzero().tolist()
    assert sorted(where) == sorted([[1, 2, 3, 5], [1, 2, 5, 5], [1, 2, 4, 4], [1, 2, 4, 6]])
    for kind in R.KINDS:
        loss, m2 = engine.gradient_loss(x, t, kind, 1e-12, want_map=True)
        assert bool(torch.isnan(loss)) and torch.equal(torch.isnan(m2), torch.isnan(m)), kind
        assert bool(torch.isnan(engine.pixel_loss(x, t, kind, 1e-12))), kind
        assert bool(torch.isnan(engine.gradient_branch_loss(t, x, kind, 1e-12))), kind


def test_repeat_calls_are_bit_equal(dev):
    for name in ("2x3x9x11", "folded"):
        xc, tc = C.content("uniform", C.SHAPES[name], 7)
        a, b = run_case(xc, tc, "plain", dev, check=False), run_case(xc, tc, "plain", dev, check=False)
        assert len(a) == len(b) == 2 + 7 * len(R.KINDS)
        for k, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(_bits(u), _bits(v)), (name, k)


def poison_cases():
    """The outputs test_gpu_spsr_poison.py compares between the product build and the poisoned profiling build: a
    shape of one workgroup, one that folds partials, an offset view."""
    dev = torch.device("cuda:0")
    outs = []
    for name in ("2x3x9x11", "folded", "view"):
        xc, tc = C.content("uniform", C.SHAPES[name], 9)
        outs += run_case(xc, tc, name if name == "view" else "plain", dev, check=False)
    return outs


def test_modules_dispatch_and_fall_back(dev):
    """The classes take the kernels for fp32 GPU tensors under 'mean' / 'sum' and the torch expressions otherwise: fp64,
    a weight, 'none', a target that requires grad, set_native_criteria(False)."""
    from ssl_amd import losses as L
    xc, tc = C.content("uniform", C.SHAPES["2x3x9x11"], 11)
    x, t = xc.to(dev), tc.to(dev)
    n = xc.numel()
    native = lambda v: "Fn" in type(v.grad_fn).__name__   # noqa: E731  (the engine's autograd nodes)
    for crit, kind in ((L.MSELoss(WEIGHT), "mse"), (L.CharbonnierLoss(WEIGHT, eps=1e-6), "charbonnier")):
        eps = 1e-6 if kind == "charbonnier" else 0.0
        xl = _leaf(x)
        loss = crit(xl, t)
        assert native(loss)
        loss.backward()
        want = R.pixel(xc, tc, kind, eps, WEIGHT / n)
        hold(f"pixel loss {kind}", loss, want.loss, want.loss_bound())
        hold(f"pixel loss {kind} gradient", xl.grad, want.grad, want.grad_bound)
        for other in (crit(_leaf(x.double()), t.double()), crit(_leaf(x), t, weight=torch.ones_like(x)),
                      crit(_leaf(x), _leaf(t))):
            assert not native(other)
            assert abs(float(other.detach()) - float(want.loss)) <= want.loss_bound(reference_sum=True)
        assert type(crit)(WEIGHT, "none")(_leaf(x), t).shape == x.shape
        prev = L.set_native_criteria(False)
        try:
            assert not native(crit(_leaf(x), t)) and L.Get_gradient()(_leaf(x)).grad_fn is not None
            assert not native(L.GradientLoss(kind)(_leaf(x), t))
        finally:
            L.set_native_criteria(prev)
    g = L.GradientLoss("charbonnier", WEIGHT, "sum", 1e-12)
    xl = _leaf(x)
    loss, m = g(xl, t, return_map=True)
    assert native(loss) and native(m) and torch.equal(_bits(m), _bits(L.Get_gradient()(x)))
    want = R.gradient_loss(xc, tc, "charbonnier", 1e-12, WEIGHT)
    hold("gradient loss charbonnier", loss, want.loss, want.loss_bound())
    assert not native(g(_leaf(x.double()), t.double())) and not native(g(_leaf(x), _leaf(t)))
    assert not native(L.GradientLoss(reduction="none")(_leaf(x), t))
    assert native(g.branch(_leaf(x), t)) and not native(g.branch(_leaf(x).double(), t.double()))
    half = L.Get_gradient()(x.half())          # not fp32: the torch expressions, in the input's dtype
    assert half.dtype == torch.float16 and half.grad_fn is None


def _integration_blocks():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## SPSR's gradient map"):]
    section = section[:section.index("\n## ", 4)]
    return re.findall(r"```python\n(.*?)```", section, re.S)


def test_the_drop_in_lines_of_integration_md_as_written(dev):
    """INTEGRATION.md's two code blocks, the drop-in and the fused form, executed as they stand on the fixture's tensors:
    the losses against the reference's recorded ones, within the bound; the fused form's tensors against the drop-in's."""
    with np.load(GOLDEN) as z:
        gold = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    blocks = _integration_blocks()
    assert len(blocks) == 2
    train_opt = dict(pixel_gradSR_opt=dict(type="MSELoss", loss_weight=R.W_GRADSR, reduction="mean"),
                     pixel_gradBranch_opt=dict(type="L1Loss", loss_weight=R.W_BRANCH, reduction="mean"))
    n = gold["sr"].numel()
    got = []
    for block in blocks:
        me = types.SimpleNamespace(device=dev, gt=gold["gt"].to(dev), output=_leaf(gold["sr"].to(dev)),
                                   fake_H_branch=_leaf(gold["branch"].to(dev)))
        me.ref = me.gt
        if got:
            me.get_grad = got[0][0].get_grad
        scope = dict(self=me, train_opt=train_opt, torch=torch)
        exec(block, scope)
        (scope["l_pix_gradSR"] + scope["l_pix_gradBranch"]).backward()
        got.append((me, scope["l_pix_gradSR"], scope["l_pix_gradBranch"]))
        want = R.gradient_loss(gold["sr"], gold["gt"], "mse", 0.0, R.W_GRADSR / n)
        for name, mine, ref, w in (("line 363", scope["l_pix_gradSR"], gold["sr_loss"], want),
                                   ("line 368", scope["l_pix_gradBranch"], gold["br_loss"],
                                    R.branch_loss(gold["branch"], gold["gt"], "l1", 0.0, R.W_BRANCH / n))):
            # both lie within their bounds of the fp64 value, the recorded one with its fp32 sum's share
            hold(name + " loss", mine, w.loss, w.loss_bound())
            assert abs(float(mine.detach()) - float(ref)) <= w.loss_bound() + w.loss_bound(reference_sum=True)
        hold("line 363 gradient", me.output.grad, want.grad, want.grad_bound)
        assert R.share(gold["sr_grad"], want.grad, want.grad_bound) <= 1.0
        for key in ("var_H_grad", "var_ref_grad", "var_H_grad_nopadding"):
            hold("map", getattr(me, key), R.gmap(gold["gt"]), R.map_bound(gold["gt"]))
            assert not getattr(me, key).requires_grad
        assert me.fake_H_grad.requires_grad
    a, b = got[0][0], got[1][0]
    assert torch.equal(_bits(a.fake_H_grad), _bits(b.fake_H_grad)) and torch.equal(_bits(a.var_H_grad), _bits(b.var_H_grad))
    assert b.var_H_grad is b.var_ref_grad is b.var_H_grad_nopadding


def test_zz_the_largest_shares(dev):
    """Prints what the module's cases used of each bound (they ran before this one: pytest keeps the file's order)."""
    for name in sorted(SHARES):
        print(f"largest share, {name}: {SHARES[name]:.3e}")
    assert max(SHARES.values(), default=0.0) <= 1.0
