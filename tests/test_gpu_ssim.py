"""The SSIM criterion's kernels (ssl_amd/csrc/ssg_ssim.hip behind ssl_amd.losses.ssim / SSIMLoss) against the fp64
restatement tests/ssim_reference.py, each result within the per-element bound derived there (the one the reference's own
fp32 results are held to in test_cpu_ssim.py): the loss, the per-image losses and the gradient, over the shapes at which
the tile pass changes its path (a tile is 32 rows x 64 columns: all padding, sides below the window, one tile, a tile
and a sliver, nine tiles, a second trip of the capped grid), the window sizes, the contents whose conditioning differs by two orders of
magnitude, either argument's gradient, layouts and dtypes, and the bit-for-bit promises."""
import functools

import pytest
import torch

import ssim_reference as R

TH, TW = 32, 64        # the tile: rows, columns
# 260 planes of two tiles (32 rows and a one-row sliver) = 520 tiles: 8 workgroups make a second trip beside 504 that make
# one (test_cpu_ssim.py ties the shape to the exported cap); narrow planes keep the fp64 yardstick at a few seconds
TRIP_SHAPE = (1, 260, TH + 1, 7)

# three planes of 14 x 14 tiles = 588: the 76 tiles of the second trip are rows 8 to 13 of the last plane, most of them
# interior tiles with eight neighbours; held bit for bit to the planes run alone (one trip each), no fp64 yardstick
INTERIOR_TRIP_SHAPE = (1, 3, 14 * TH, 14 * TW)

# (shape, window_size, content)
SHAPES = [((1, 1, 1, 1), 11, "uniform01"),
          ((1, 1, 7, 5), 11, "uniform11"),
          ((1, 3, 11, 11), 1, "uniform01"),
          ((1, 3, 11, 11), 3, "uniform01"),
          ((1, 3, 11, 11), 7, "uniform01"),
          ((1, 3, 11, 11), 11, "uniform01"),
          ((1, 1, TH, TW), 11, "uniform01"),
          ((1, 1, TH + 1, TW - 1), 11, "uniform01"),
          ((2, 3, 40, 37), 11, "uniform01"),
          (TRIP_SHAPE, 11, "uniform01")]
CONTENT_SHAPE = (1, 1, 3 * TH, 3 * TW)
CASES = SHAPES + [(CONTENT_SHAPE, 11, name) for name in R.CONTENTS]


def _id(case):
    shape, ws, name = case
    return "x".join(map(str, shape)) + f"-w{ws}-{name}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda")


def _upstream(B):
    """Unequal upstream gradients per image."""
    return torch.tensor([0.7, -1.3, 2.1, 0.4][:B], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _yardstick(case):
    """Computed once per case and shared: inputs, fp64 losses, per-image gradients of L = sum_b g_b mean_b(S) and the
    bounds.  The scalar mean's gradient and bound are the per-image ones with every g_b = 1 / B."""
    shape, ws, name = case
    x, y = R.content(name, shape, seed=len(name) + sum(shape))
    B, n_img = shape[0], shape[1] * shape[2] * shape[3]
    g = _upstream(B)
    out = {"x": x, "y": y, "g": g, "mean": R.ssim(x, y, ws, True), "per_image": R.ssim(x, y, ws, False)}
    # gradient and bound are linear in each image's coefficient (the bound in its magnitude): one evaluation at 1
    unit = torch.ones(B, dtype=torch.float64)
    gx, gy = R.gradients(x, y, ws, unit)
    out["lb"], bx, by = R.bounds(x, y, ws, unit)
    for key, coef in (("avg", torch.full((B,), 1.0 / (B * n_img), dtype=torch.float64)), ("img", g / n_img)):
        c = coef.reshape(B, 1, 1, 1)
        out["gx_" + key], out["gy_" + key] = gx * c, gy * c
        out["bx_" + key], out["by_" + key] = bx * c.abs(), by * c.abs()
    return out


def _run(dev, x, y, ws, avg, gout, need=(True, False)):
    """ssim on the GPU; (loss, grad_x or None, grad_y or None) on the CPU."""
    from ssl_amd.losses import ssim
    a = x.to(dev).requires_grad_(need[0])
    b = y.to(dev).requires_grad_(need[1])
    loss = ssim(a, b, ws, avg)
    if any(need):
        (loss.double() * gout.to(dev)).sum().backward()
    return loss.detach().cpu(), None if a.grad is None else a.grad.cpu(), None if b.grad is None else b.grad.cpu()


def _within(got, want, bound, what):
    d = (got.double() - want).abs()
    share = R.share(got, want, bound)
    print(f"{what}: max |diff| {float(d.max()):.3e}, share of the bound {share:.3e}")
    assert bool(torch.isfinite(got.double()).all()), what
    assert bool((d <= bound).all()), (what, share)
    return share


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_loss_and_gradient_within_the_bound(dev, case):
    shape, ws, _ = case
    Y = _yardstick(case)
    one = torch.ones((), dtype=torch.float64)
    loss, gx, _ = _run(dev, Y["x"], Y["y"], ws, True, one)
    assert loss.shape == () and loss.dtype == torch.float32 and gx.shape == shape and gx.dtype == torch.float32
    _within(loss, Y["mean"], Y["lb"].mean(), "loss")
    _within(gx, Y["gx_avg"], Y["bx_avg"], "grad_x")
    per, gxi, _ = _run(dev, Y["x"], Y["y"], ws, False, Y["g"])
    assert per.shape == (shape[0],)
    _within(per, Y["per_image"], Y["lb"], "per-image losses")
    _within(gxi, Y["gx_img"], Y["bx_img"], "grad_x, per-image upstream")
    if case[2] == "zero":
        assert float(loss) == 1.0 and not bool(gx.any())
    if case[2] == "equal":
        assert float(loss) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[8], (CONTENT_SHAPE, 11, "smooth")], ids=_id)
def test_gradient_on_the_second_argument_and_on_both(dev, case):
    shape, ws, _ = case
    Y = _yardstick(case)
    l2, none, gy = _run(dev, Y["x"], Y["y"], ws, False, Y["g"], need=(False, True))
    assert none is None
    _within(gy, Y["gy_img"], Y["by_img"], "grad_y alone")
    l3, gx, gy2 = _run(dev, Y["x"], Y["y"], ws, False, Y["g"], need=(True, True))
    _within(gx, Y["gx_img"], Y["bx_img"], "grad_x of both")
    assert torch.equal(gy2, gy)
    l0, _, _ = _run(dev, Y["x"], Y["y"], ws, False, Y["g"], need=(False, False))      # the loss-only kernel
    _within(l0, Y["per_image"], Y["lb"], "loss-only")
    # the map is symmetric operation by operation and every pixel has one owner: the same sums from every entry
    assert torch.equal(l2, l3) and torch.equal(l0, l3)


@pytest.mark.gpu
def test_module_channels_last_and_bf16(dev):
    from ssl_amd.losses import SSIMLoss
    case = CASES[8]
    Y = _yardstick(case)
    one = torch.ones((), dtype=torch.float64)
    want_loss, want_gx, _ = _run(dev, Y["x"], Y["y"], 11, True, one)
    crit = SSIMLoss()
    assert (crit.window_size, crit.size_average, crit.channel) == (11, True, 1) and crit.window.shape == (1, 1, 11, 11)
    a = Y["x"].to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b = Y["y"].to(dev).contiguous(memory_format=torch.channels_last)
    assert not a.is_contiguous()
    loss = crit(a, b)
    loss.backward()
    assert crit.channel == 3 and crit.window.shape == (3, 1, 11, 11) and crit.window.device == a.device
    assert torch.equal(loss.detach().cpu(), want_loss) and torch.equal(a.grad.cpu(), want_gx)
    # bf16: computed in fp32 on the bf16 values, the fp32 gradient (within the bound of fp64) then rounded to bf16, whose
    # 8-bit significand has the unit roundoff 2^-8
    xb, yb = Y["x"].to(torch.bfloat16), Y["y"].to(torch.bfloat16)
    n = xb.numel()
    coef = torch.full((2,), 1.0 / n, dtype=torch.float64)
    lb, gb, _ = _run(dev, xb, yb, 11, True, one)
    assert gb.dtype == torch.bfloat16 and lb.dtype == torch.float32
    gx64, _ = R.gradients(xb, yb, 11, coef)
    bl, bx, _ = R.bounds(xb, yb, 11, coef)
    _within(lb, R.ssim(xb, yb, 11, True), bl.mean(), "bf16 loss")
    _within(gb, gx64, bx + 2.0 ** -8 * (gx64.abs() + bx), "bf16 grad_x")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.mark.gpu
def test_repeat_and_batch_bit_equality(dev):
    Y = _yardstick(CASES[8])
    g = Y["g"]
    l1, g1, _ = _run(dev, Y["x"], Y["y"], 11, False, g)
    l2, g2, _ = _run(dev, Y["x"], Y["y"], 11, False, g)
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(g1), _bits(g2))
    for b in range(2):
        lb, gb, _ = _run(dev, Y["x"][b:b + 1], Y["y"][b:b + 1], 11, False, g[b:b + 1])
        assert torch.equal(_bits(lb), _bits(l1[b:b + 1])) and torch.equal(_bits(gb), _bits(g1[b:b + 1]))
    # past the grid cap too: two calls bit-equal
    Yt = _yardstick(CASES[9])
    one = torch.ones((), dtype=torch.float64)
    a = _run(dev, Yt["x"], Yt["y"], 11, True, one)
    b = _run(dev, Yt["x"], Yt["y"], 11, True, one)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.gpu
def test_second_trip_over_interior_tiles_equals_the_planes_alone(dev):
    """A pixel's gradient and map value do not depend on which workgroup, or which of its trips, forms them: the batch
    of three planes (588 tiles under the cap of 512) against each plane alone (196 tiles, one trip), gradient bit for
    bit and the sum to fp64 rounding."""
    from ssl_amd import engine
    x, y = (t.to(dev) for t in R.content("smooth", INTERIOR_TRIP_SHAPE, seed=7))
    sums, grad = engine._ssim_sums(x, y, 11, True)
    alone = [engine._ssim_sums(x[:, c:c + 1].contiguous(), y[:, c:c + 1].contiguous(), 11, True) for c in range(3)]
    for c, (s_c, g_c) in enumerate(alone):
        assert torch.equal(_bits(grad[:, c:c + 1]), _bits(g_c)), c
    total = sum(float(s_c[1]) for s_c, _ in alone)
    assert float(sums[0]) == float(sums[1]) and abs(float(sums[1]) - total) <= 1e-12 * abs(total)
    assert torch.equal(_bits(engine._ssim_sums(x, y, 11, False)[0]), _bits(sums))      # the loss-only form, same trips


@pytest.mark.gpu
def test_refusals_on_the_device(dev):
    from ssl_amd.losses import SSIMLoss, ssim
    x = torch.rand(1, 3, 16, 16, device=dev, requires_grad=True)
    y = torch.rand(1, 3, 16, 16, device=dev)
    for ws in (4, 13):
        with pytest.raises(ValueError, match="up to 11"):
            ssim(x, y, ws)
        with pytest.raises(ValueError, match="up to 11"):
            SSIMLoss(ws)
    with pytest.raises(ValueError, match="one shape"):
        ssim(x, y[:, :, :8])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ssim(x.detach().cpu(), y.cpu())
    # double backward: the gradient carries no graph of its own, and where the upstream gradient has one (a learnable
    # weight on the loss) differentiating through it raises
    g, = torch.autograd.grad(ssim(x, y), x, create_graph=True)
    assert not g.requires_grad
    w = torch.ones((), device=dev, requires_grad=True)
    g, = torch.autograd.grad(ssim(x, y) * w, x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def poison_cases():
    """The outputs the LDS-poison test compares bit for bit (test_gpu_ssim_poison.py): every kernel, both tile forms."""
    dev = torch.device("cuda")
    out = []
    for case, avg, need in ((CASES[1], True, (True, False)), (CASES[3], True, (True, True)),
                            (CASES[7], True, (True, False)), (CASES[8], False, (True, True)),
                            (CASES[8], False, (False, False)), ((CONTENT_SHAPE, 11, "step"), True, (True, False)),
                            (CASES[9], True, (False, False)), (CASES[9], True, (True, False))):
        Y = _yardstick(case)
        gout = torch.ones((), dtype=torch.float64) if avg else Y["g"]
        out += [t for t in _run(dev, Y["x"], Y["y"], case[1], avg, gout, need) if t is not None]
    return out
