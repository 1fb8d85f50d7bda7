"""BebyGAN's back-projection loss and its imresize on the MI355X (ssl_amd/csrc/ssg_bp.hip) against the fp64 restatement
of the contract (bp_reference.py, which test_cpu_bp.py pins to the reference's own outputs, tests/golden/f20_bp.npz).

Every bound is derived, not measured, and evaluated per element by bp_reference.py (u = 2^-24):
    imresize values      |y - y64|_o <= T_o = (K^2 + 8) u A_o
    loss                 |L - L64|   <= lambda mean_o(T_o + 2u (|y64| + |lq|)) + 2u |L64|   (or the sum)
    gradient / backward  |d|_h       <= 152 u (|K|^T |g|)_h, g = lambda / M sgn(y64 - lq) for the loss
    adjoint              fp64 <y, g> and <x, grad> of the GPU's fp32 y and grad agree to 1e-5 of the larger: both are
                         within a few hundred u of sum |terms|, and g = 1 + N(0,1) on x in [0, 1] keeps the inner
                         product at a fixed share of sum |terms| (no cancellation)
The sign of y - lq is taken from fp64; an output with |y64 - lq| <= T_o + u |lq| is ambiguous at fp32 and the input
pixels under its window are left out of the gradient comparison; every input must leave at most 0.2 % of its outputs
ambiguous (asserted on the reference alone).

Every comparison prints one `BP64` line (pytest -s) with the worst error over its bound."""
import functools

import numpy as np
import pytest
import torch

import bp_reference as R
from raw_loss import RawLoss, replays_as_hip_graph, side_stream_equals_default_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# forward tile 16 x 8 outputs, backward tile 64 x 32 pixels: 45 x 83 at s = 4 (11 x 20 outputs) exceeds both by a
# remainder on both axes
SWEEP = [(4, (2, 3, 48, 40)), (4, (1, 3, 50, 43)), (4, (1, 1, 6, 7)), (4, (1, 3, 8, 9)), (4, (3, 3, 6, 6)),
         (4, (1, 3, 70, 67)), (4, (1, 3, 200, 136)), (4, (1, 2, 45, 83)),
         (3, (1, 3, 27, 31)), (3, (1, 3, 4, 5)), (3, (2, 3, 64, 47)),
         (2, (2, 1, 24, 26)), (2, (1, 3, 3, 4)), (2, (1, 3, 37, 90))]
# more forward tiles (16 x 8 outputs each) than the 4,096 workgroups bp_fwd gets: a workgroup's second tile, and bp_bwd
# folding 4,096 partial sums.  One-tile planes at s = 4, 3 and 2, then many ragged tiles per plane (33 x 28 on 6 planes)
TRIPS = [(4, (1367, 3, 8, 9)), (3, (1366, 3, 7, 10)), (2, (1400, 3, 5, 6)), (2, (2, 3, 700, 650))]
SMOOTH = [(4, (1, 3, 50, 43)), (3, (1, 3, 27, 31)), (2, (1, 3, 37, 90))]
WEIGHTS = [('mean', 1.0), ('mean', 0.37), ('sum', 1.0), ('sum', 0.37)]


@functools.lru_cache(maxsize=None)
def inputs(s, shape, kind="noise"):
    """(x, lq, g) on the CPU, fp32, seeded: x uniform noise or a smooth field, lq = y64 + 0.05 N(0,1), g = 1 + N(0,1)
    the upstream of the generic backward."""
    gen = torch.Generator().manual_seed(1000 * s + shape[0] + 7 * shape[2] + 13 * shape[3] + (kind == "smooth"))
    x = torch.rand(shape, generator=gen) if kind == "noise" else R.smooth_field(shape, 5 * s)
    y64 = R.forward(x, s)
    lq = (y64 + 0.05 * torch.randn(y64.shape, generator=gen, dtype=torch.float64)).float()
    g = (1 + torch.randn(y64.shape, generator=gen, dtype=torch.float64)).float()
    return x, lq, g


@functools.lru_cache(maxsize=None)
def reference(s, shape, kind="noise"):
    """What the fp64 contract says about inputs(...), computed once: y64, T_o, the ambiguous outputs and the pixels
    under them, the generic backward and its bound."""
    x, lq, g = inputs(s, shape, kind)
    H, W = shape[-2:]
    y64 = R.forward(x, s)
    amb, under = R.ambiguous(x, lq, s, y64)
    return dict(y64=y64, T=R.forward_bound(x, s), amb=amb, under=under, gx64=R.adjoint(g, s, H, W),
                gbound=R.backward_bound(g, s, H, W))


def hip_loss(x, lq, s, reduction='mean', lw=1.0):
    from ssl_amd.losses import BackProjectionLoss
    xs = x.to(DEV).requires_grad_(True)
    loss = BackProjectionLoss(lw, reduction, s)(xs, lq.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), xs.grad.cpu()


def ratio(err, bound):
    """Worst err / bound; an element whose bound is 0 must have no error."""
    assert bool((err[bound == 0] == 0).all())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def check(name, s, shape, kind="noise", weights=WEIGHTS):
    from ssl_amd.losses import imresize
    x, lq, g = inputs(s, shape, kind)
    ref = reference(s, shape, kind)
    H, W = shape[-2:]
    share = float(ref["amb"].double().mean())
    assert share <= 0.002, (name, share)                              # the condition on the input
    xs = x.to(DEV).requires_grad_(True)
    y = imresize(xs, scale=1 / s)
    assert y.shape == shape[:-2] + (H // s, W // s) and y.dtype == torch.float32
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    y, gx = y.detach().cpu().double(), xs.grad.cpu().double()
    r_fwd = ratio((y - ref["y64"]).abs(), ref["T"])
    r_bwd = ratio((gx - ref["gx64"]).abs(), ref["gbound"])
    a, b = float((y * g.double()).sum()), float((x.double() * gx).sum())
    r_adj = abs(a - b) / max(abs(a), abs(b))
    print(f"BP64 {name}: s {s} shape {shape} {kind} forward {r_fwd:.4f} T_o backward {r_bwd:.4f} bound "
          f"adjoint {r_adj:.2e} ambiguous {share:.5f}")
    assert r_fwd <= 1 and r_bwd <= 1 and r_adj <= 1e-5, (name, r_fwd, r_bwd, r_adj)
    for reduction, lw in weights:
        lw32 = float(np.float32(lw))                                  # the C ABI takes it as a float
        loss64, grad64, y64, up = R.loss_and_grad(x, lq, s, lw32, reduction)
        loss, grad = hip_loss(x, lq, s, reduction, lw)
        lb = R.loss_bound(x, lq, s, y64, loss64, lw32, reduction)
        r_loss = abs(float(loss) - float(loss64)) / lb
        keep = ~ref["under"]
        r_grad = ratio((grad.double() - grad64).abs()[keep], R.backward_bound(up, s, H, W)[keep])
        print(f"BP64 {name}: {reduction} lambda {lw} loss {float(loss):.8g} fp64 {float(loss64):.8g} "
              f"err {r_loss:.4f} bound gradient {r_grad:.4f} bound (pixels compared {float(keep.double().mean()):.4f})")
        assert r_loss <= 1 and r_grad <= 1, (name, reduction, lw, r_loss, r_grad)
        assert grad.shape == x.shape and bool(torch.isfinite(grad).all())


# --------------------------------------------------------------------------------------------- the fixture ----
def test_hip_against_the_reference_fixture(golden):
    """F20: the reference's own fp32 outputs.  Two fp32 evaluations are compared, each within its bound of fp64, so
    every tolerance is the kernel's bound plus the pin tolerance of test_cpu_bp.py (the reference's bound plus what
    its s = 3 table moves); dtype and shape of the fp16, 3-D and 2-D cases."""
    from ssl_amd.losses import imresize
    z = golden("f20_bp")
    for i in range(int(z["n_cases"])):
        c = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        x, lq, s = torch.from_numpy(c["x"]), torch.from_numpy(c["lq"]), int(c["s"])
        H, W = x.shape[-2:]
        table, w = torch.from_numpy(z[f"table_s{s}"]), R.taps(s)
        T, pin = R.forward_bound(x, s), R.pin_bound(x, s, table)
        y = imresize(x.to(DEV), scale=1 / s).cpu()
        assert y.shape == c["y"].shape
        assert bool(((y.double() - torch.from_numpy(c["y"]).double()).abs() <= T + pin).all()), i
        loss64, _, y64, g = R.loss_and_grad(x, lq, s)
        assert int(R.ambiguous(x, lq, s, y64)[0].sum()) == 0
        loss, grad = hip_loss(x, lq, s)
        lb = 2 * R.loss_bound(x, lq, s, y64, loss64) + float((pin - T).mean())
        assert abs(float(loss) - float(c["loss"])) <= lb, i
        gb = 2 * R.backward_bound(g, s, H, W) + R.adjoint(g.abs(), s, H, W, table=(table.double() - torch.outer(w, w)).abs())
        assert bool(((grad.double() - torch.from_numpy(c["grad"]).double()).abs() <= gb).all()), i
    for key, s in (("h", 4), ("d3", 3), ("d2", 2)):
        x, want = torch.from_numpy(z[f"{key}_x"]), torch.from_numpy(z[f"{key}_y"])
        y = imresize(x.to(DEV), scale=1 / s).cpu()
        assert y.dtype == want.dtype and y.shape == want.shape
        tol = R.forward_bound(x, s) + R.pin_bound(x, s, torch.from_numpy(z[f"table_s{s}"]))
        if key == "h":
            tol = tol + 2.0 ** -10 * (want.double().abs() + tol)      # each side's cast back to half
        assert bool(((y.double() - want.double()).abs() <= tol).all()), key


# ------------------------------------------------------------------------------------------------ the sweep ----
@pytest.mark.parametrize("s,shape", SWEEP + TRIPS, ids=[f"s{s}-" + "x".join(map(str, sh)) for s, sh in SWEEP + TRIPS])
def test_shape_sweep(s, shape):
    if (s, shape) in TRIPS:      # (what these are for is the second trip, not the weights: one mean, one sum)
        check("trips", s, shape, weights=WEIGHTS[:1] + WEIGHTS[3:])
    else:
        check("sweep", s, shape)


@pytest.mark.parametrize("s,shape", SMOOTH, ids=[f"s{s}" for s, _ in SMOOTH])
def test_smooth_field(s, shape):
    check("smooth", s, shape, kind="smooth", weights=WEIGHTS[:1])


def test_configured_size():
    """16 x 3 x 192 x 192 at s = 4, once."""
    check("configured", 4, (16, 3, 192, 192), weights=[('mean', 1.0)])


# ------------------------------------------------------------------------------------------ impulse response ----
@pytest.mark.parametrize("s", [2, 3, 4])
def test_impulse_response(s):
    """A single 1.0 at the four corners, at (p-1, p), at the centre and at (1, W-2) of a (p + 2K)^2 image: every
    output within T_o (1.6e-5 relative to the tap itself at s = 4), every output outside the support exactly 0.  A
    dropped or mis-mirrored tap, which random inputs could hide under A_o, shows here."""
    from ssl_amd.losses import imresize
    K, p = R.geometry(s)
    n = p + 2 * K
    spots = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (p - 1, p), (n // 2, n // 2), (1, n - 2)]
    x = torch.zeros((len(spots), 1, n, n))
    for i, (r, c) in enumerate(spots):
        x[i, 0, r, c] = 1.0
    y = imresize(x.to(DEV), scale=1 / s).cpu().double()
    y64, T = R.forward(x, s), R.forward_bound(x, s)
    off = y64 == 0
    assert bool((~off).flatten(1).any(1).all()) and bool(off.flatten(1).any(1).all())    # every impulse is seen, and ends
    assert bool((y[off] == 0).all())
    worst = ratio((y - y64).abs(), T)
    print(f"BP64 impulse: s {s} side {n} forward {worst:.4f} T_o, support {int((~off).sum())} outputs")
    assert worst <= 1


# --------------------------------------------------------------------------------------------- further cases ----
def test_zero_input_gives_exact_zeros():
    x, lq = torch.zeros(2, 3, 50, 43), torch.zeros(2, 3, 12, 10)
    for reduction in ('mean', 'sum'):
        loss, grad = hip_loss(x, lq, 4, reduction)
        assert float(loss) == 0 and bool((grad == 0).all())


def test_two_runs_are_bit_identical():
    x, lq, _ = inputs(4, (2, 3, 48, 40))
    a, b = hip_loss(x, lq, 4), hip_loss(x, lq, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_non_contiguous_and_half_inputs():
    from ssl_amd.losses import BackProjectionLoss, imresize
    x, lq, g = inputs(4, (2, 3, 48, 40))
    xd, lqd, gd = x.to(DEV), lq.to(DEV), g.to(DEV)
    want = imresize(xd, scale=0.25)
    xc = xd.contiguous(memory_format=torch.channels_last)
    big = torch.zeros((2, 3, 48, 80), device=DEV)
    big[..., ::2] = xd
    lbig = torch.zeros((2, 3, 12, 20), device=DEV)
    lbig[..., ::2] = lqd
    assert not xc.is_contiguous() and not big[..., ::2].is_contiguous() and not lbig[..., ::2].is_contiguous()
    for v in (xc, big[..., ::2]):
        assert torch.equal(imresize(v, scale=0.25), want)
    l0, g0 = hip_loss(x, lq, 4)
    v = big[..., ::2].detach().requires_grad_(True)
    l1 = BackProjectionLoss()(v, lbig[..., ::2])
    l1.backward()
    assert torch.equal(l1.detach().cpu(), l0) and torch.equal(v.grad.cpu(), g0)
    # half and bfloat16: computed in fp32 on the widened values, cast back
    for dt in (torch.float16, torch.bfloat16):
        xh = xd.to(dt).requires_grad_(True)
        yh = imresize(xh, scale=0.25)
        assert yh.dtype == dt and torch.equal(yh, imresize(xh.detach().float(), scale=0.25).to(dt))
        yh.backward(gd.to(dt))
        x32 = xh.detach().float().requires_grad_(True)
        imresize(x32, scale=0.25).backward(gd.to(dt).float())
        assert xh.grad.dtype == dt and torch.equal(xh.grad, x32.grad.to(dt))
        xl = xd.to(dt).requires_grad_(True)
        lh = BackProjectionLoss()(xl, lqd.to(dt))
        lh.backward()
        x32 = xd.to(dt).float().requires_grad_(True)
        l32 = BackProjectionLoss()(x32, lqd.to(dt).float())
        l32.backward()
        assert torch.equal(lh, l32) and torch.equal(xl.grad, x32.grad.to(dt))
    # 3-D and 2-D tensors are planes like any other
    assert torch.equal(imresize(xd[0], scale=0.25), want[0]) and torch.equal(imresize(xd[1, 2], scale=0.25), want[1, 2])


def test_python_layer_refusals_on_the_device():
    from ssl_amd.losses import BackProjectionLoss, imresize
    x, lq, _ = inputs(4, (2, 3, 48, 40))
    xd, lqd = x.to(DEV), lq.to(DEV)
    with pytest.raises(ValueError, match="lq"):
        BackProjectionLoss()(xd, lqd.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="lq must be"):
        BackProjectionLoss()(xd, lqd[..., :9])
    with pytest.raises(ValueError, match="lq must be"):
        BackProjectionLoss(scale=2)(xd, lqd)
    with pytest.raises(RuntimeError, match="GPU"):
        BackProjectionLoss()(x, lq)
    with pytest.raises(ValueError, match="smaller"):
        imresize(torch.zeros(1, 1, 5, 9, device=DEV), scale=0.25)
    assert not BackProjectionLoss()(xd, lqd).requires_grad


def test_best_buddy_and_back_projection_terms_together():
    """BebyGAN's two pixel terms on one output, one backward: out.grad is the sum of the two separate gradients bit
    for bit."""
    from ssl_amd.losses import BackProjectionLoss, BestBuddyLoss
    x, lq, _ = inputs(4, (2, 3, 48, 40))
    gt = torch.rand(2, 3, 48, 40, generator=torch.Generator().manual_seed(9)).to(DEV)
    bb, bp = BestBuddyLoss(), BackProjectionLoss()
    out = x.to(DEV).requires_grad_(True)
    total = bb(out, gt) + bp(out, lq.to(DEV))
    total.backward()
    parts = []
    for crit, target in ((bb, gt), (bp, lq.to(DEV))):
        o = x.to(DEV).requires_grad_(True)
        crit(o, target).backward()
        parts.append(o.grad)
    assert torch.equal(out.grad, parts[0] + parts[1])
    assert float(parts[0].abs().max()) > 0 and float(parts[1].abs().max()) > 0


# ----------------------------------------------------------------------------------- streams and graphs (C ABI) ----
def _raw_loss(shape, s=4):
    """ssg_bp_loss through the C ABI (raw_loss.RawLoss): loss, grad and y, the last two pre-filled with NaN."""
    from ssl_amd import _lib
    B, C, H, W = shape
    L = _lib.lib()
    nb = L.ssg_bp_workspace_bytes(B * C, H, W, s)
    assert 0 < nb <= 2 * B * C * (H // s) * (W // s) * 4 + 65536
    return RawLoss(L.ssg_bp_loss, nb, lambda x, lq: (x.data_ptr(), lq.data_ptr(), B * C, H, W, s, 1.0, 1),
                   (torch.zeros(1, device=DEV), torch.full(shape, float('nan'), device=DEV),
                    torch.full((B, C, H // s, W // s), float('nan'), device=DEV)))


def _dev_inputs(shape, s=4):
    x, lq, _ = inputs(s, shape)
    return x.to(DEV), lq.to(DEV)


@pytest.mark.parametrize("s,shape", [(4, (1, 3, 70, 67)), (4, (1, 3, 8, 9)), (3, (1, 3, 4, 5)), (2, (1, 3, 37, 90)),
                                     (4, (1367, 3, 8, 9))])
def test_every_gradient_element_is_written(s, shape):
    """grad_x and y_out pre-filled with NaN: the call leaves none, and equals the Python layer bit for bit."""
    x, lq = _dev_inputs(shape, s)
    raw = _raw_loss(shape, s)
    raw(x, lq)
    torch.cuda.synchronize()
    loss, grad, y = raw.outputs()
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(y).all())
    l2, g2 = hip_loss(x.cpu(), lq.cpu(), s)
    assert torch.equal(loss[0].cpu(), l2) and torch.equal(grad.cpu(), g2)
    from ssl_amd.losses import imresize
    assert torch.equal(y, imresize(x, scale=1 / s))


def test_side_stream_equals_default_stream():
    shape = (2, 3, 48, 40)
    side_stream_equals_default_stream(lambda: _raw_loss(shape), _dev_inputs(shape))


def test_loss_replays_as_hip_graph():
    """The captured call is a single chain of two launches on one stream."""
    shape = (2, 3, 48, 40)
    first = _dev_inputs(shape)
    second = tuple(t.flip(0).contiguous() * 0.9 for t in first)
    want = replays_as_hip_graph(lambda: _raw_loss(shape), (first, second))
    first_run = _raw_loss(shape)
    first_run(*first)
    torch.cuda.synchronize()
    assert not torch.equal(first_run.outputs()[1], want[1])      # the second batch really differs


def test_c_abi_refusals_on_the_device():
    """The refusals of test_cpu_bp.py with real device pointers: nothing is launched, the outputs stay untouched."""
    from ssl_amd import _lib
    L = _lib.lib()
    x, lq = _dev_inputs((1, 3, 8, 9))
    grad = torch.full((1, 3, 8, 9), -7.0, device=DEV)
    out = torch.full((1,), -7.0, device=DEV)
    nb = L.ssg_bp_workspace_bytes(3, 8, 9, 4)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)

    def loss(H=8, W=9, s=4, lw=1.0, wsp=ws.data_ptr(), n=nb):
        return L.ssg_bp_loss(x.data_ptr(), lq.data_ptr(), 3, H, W, s, lw, 1, out.data_ptr(), grad.data_ptr(), None,
                             wsp, n, None)

    assert loss(s=1) == -1 and loss(lw=float('nan')) == -1 and loss(s=5) == -2 and loss(H=5) == -4 and loss(W=3) == -4
    assert loss(n=nb - 1) == -3 and loss(wsp=ws.data_ptr() + 4) == -5
    assert L.ssg_bp_downsample_backward(lq.data_ptr(), 3, 5, 9, 4, grad.data_ptr(), None) == -4
    torch.cuda.synchronize()
    assert int((grad != -7).sum()) == 0 and float(out) == -7
    assert loss() == 0
    torch.cuda.synchronize()
    assert int((grad == -7).sum()) == 0 and float(out) != -7


# ------------------------------------------------------------------------- shared with test_gpu_bp_poison.py ----
def poison_cases():
    """What the LDS-poison test runs on the product build and again on the poisoned profiling build: the output, the
    generic backward, the loss and its gradient at the smallest sides, under both mirrors, at odd shapes of every
    factor, past one tile on both axes and past one trip of the forward's 4,096 workgroups."""
    from ssl_amd import engine
    out = []
    for s, shape in ((4, (1, 1, 6, 7)), (4, (1, 3, 8, 9)), (4, (1, 2, 45, 83)), (3, (2, 3, 64, 47)), (2, (1, 3, 37, 90)),
                     (4, (1367, 3, 8, 9))):
        x, lq, g = (t.to(DEV) for t in inputs(s, shape))
        xs = x.clone().requires_grad_(True)
        y = engine.bp_downsample(xs, s)
        y.backward(g)
        out += [y.detach(), xs.grad]
        xs = x.clone().requires_grad_(True)
        loss = engine.bp_loss(xs, lq, s, 0.37, 'sum')
        loss.backward()
        out += [loss.detach().reshape(1), xs.grad]
    torch.cuda.synchronize()
    return out
