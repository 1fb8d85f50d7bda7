"""BebyGAN's back-projection loss and its imresize without a GPU: the fp64 restatement of the contract
(tests/bp_reference.py) that the GPU tests use reproduces the reference's own outputs (tests/golden/f20_bp.npz) within
the derived bounds, the new symbols are exported, the C ABI refuses bad arguments before it launches anything, and the
Python layer refuses what lies outside the native domain."""
import ctypes

import pytest
import torch

import bp_reference as R

BP_SYMBOLS = ("ssg_bp_workspace_bytes", "ssg_bp_downsample", "ssg_bp_downsample_backward", "ssg_bp_loss")
SHAPES = [((1, 3, 24, 20), 4), ((1, 3, 26, 23), 4), ((1, 1, 6, 7), 4), ((1, 3, 15, 14), 3), ((2, 1, 10, 12), 2),
          ((1, 3, 8, 9), 4)]


def _cases(golden):
    z = golden("f20_bp")
    for i in range(int(z["n_cases"])):
        yield i, {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}


def test_f20_holds_the_cases_it_must(golden):
    got = [(tuple(c["x"].shape), int(c["s"])) for _, c in _cases(golden)]
    assert got == SHAPES
    for (shape, s), (_, c) in zip(SHAPES, _cases(golden)):
        assert c["y"].shape == c["lq"].shape == shape[:2] + (shape[2] // s, shape[3] // s)
    # 8 x 9 at s = 4: p = 6 <= n < 2p, so pixels 2 .. 5 of the 8-pixel side lie under both mirrors
    _, p = R.geometry(4)
    assert p <= 8 < 2 * p


def test_taps_match_the_reference_tables(golden):
    """Closed form against discrete_kernel('cubic', 1 / s): exact at fp32 for s = 2 and 4, max |dk| <= 4e-8 for s = 3
    (the reference's fp32 linspace moves the small taps)."""
    z = golden("f20_bp")
    for s, (K, p) in ((2, (8, 3)), (3, (11, 4)), (4, (16, 6))):
        assert R.geometry(s) == (K, p)
        w = R.taps(s)
        assert abs(float(w.sum()) - 1) <= 1e-15 and torch.equal(w, w.flip(0))
        table = torch.from_numpy(z[f"table_s{s}"])
        assert table.shape == (K, K) and table.dtype == torch.float32
        k2 = torch.outer(w, w)
        if s == 3:
            assert float((k2 - table.double()).abs().max()) <= 4e-8
        else:
            assert torch.equal(k2.float(), table)


def test_symmetric_index_uses_the_edge_pixel_twice():
    assert R.sym_index(4, 1).tolist() == [0, 0, 1, 2, 3, 3]
    assert R.sym_index(6, 6).tolist() == [5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0]
    assert R.sym_index(8, 6).tolist() == [5, 4, 3, 2, 1, 0] + list(range(8)) + [7, 6, 5, 4, 3, 2]


def test_restatement_reproduces_f20(golden):
    """Output within the pin tolerance T_o + (|dk| * |x~|)_o, the loss within its bound (the forward term taken at the
    pin tolerance), the gradient within 152 u (|K|^T |g|) plus what dk moves, shapes H // s."""
    z = golden("f20_bp")
    for i, c in _cases(golden):
        x, lq, s = torch.from_numpy(c["x"]), torch.from_numpy(c["lq"]), int(c["s"])
        table = torch.from_numpy(z[f"table_s{s}"])
        H, W = x.shape[-2:]
        loss64, grad64, y64, g = R.loss_and_grad(x, lq, s)
        assert y64.shape == x.shape[:2] + (H // s, W // s) and grad64.shape == x.shape
        amb, _ = R.ambiguous(x, lq, s, y64)
        assert int(amb.sum()) == 0, i                                 # every sign of the fixture is decided
        pin = R.pin_bound(x, s, table)
        err = (y64 - torch.from_numpy(c["y"]).double()).abs()
        assert bool((err <= pin).all()), (i, float((err / pin).max()))
        dk = float((pin - R.forward_bound(x, s)).mean())
        assert abs(float(loss64) - float(c["loss"])) <= R.loss_bound(x, lq, s, y64, loss64) + dk, i
        # the reference's gradient is the adjoint with ITS table: |dk|^T |g| on top of the derived bound
        w = R.taps(s)
        gerr = (grad64 - torch.from_numpy(c["grad"]).double()).abs()
        bound = R.backward_bound(g, s, H, W) + R.adjoint(g.abs(), s, H, W, table=(table.double() - torch.outer(w, w)).abs())
        assert bool((gerr <= bound).all()), (i, float((gerr / bound).max()))


def test_restatement_reproduces_the_fp16_3d_and_2d_cases(golden):
    z = golden("f20_bp")
    for key, s, dtype in (("h", 4, torch.float16), ("d3", 3, torch.float32), ("d2", 2, torch.float32)):
        x, want = torch.from_numpy(z[f"{key}_x"]), torch.from_numpy(z[f"{key}_y"])
        y64 = R.forward(x, s)
        assert x.dtype == want.dtype == dtype
        assert y64.shape == want.shape == x.shape[:-2] + (x.shape[-2] // s, x.shape[-1] // s)
        tol = R.pin_bound(x, s, torch.from_numpy(z[f"table_s{s}"]))
        if dtype == torch.float16:
            tol = tol + 2.0 ** -11 * y64.abs()                        # the cast back to half
        assert bool(((y64 - want.double()).abs() <= tol).all()), key


def test_adjoint_is_the_adjoint_and_counts_every_copy():
    """<K x, g> = <x, K^T g> in fp64, and K^T 1 sums to (number of outputs) * (sum of taps)^2 = h w: no padded copy is
    lost or counted twice, also where one pixel lies under both mirrors (8 x 9, 6 x 7 at s = 4)."""
    gen = torch.Generator().manual_seed(3)
    for (H, W), s in (((8, 9), 4), ((6, 7), 4), ((26, 23), 4), ((15, 14), 3), ((4, 5), 3), ((3, 4), 2), ((10, 12), 2)):
        x = torch.rand((2, H, W), generator=gen, dtype=torch.float64)
        g = torch.randn((2, H // s, W // s), generator=gen, dtype=torch.float64)
        a, b = float((R.forward(x, s) * g).sum()), float((x * R.adjoint(g, s, H, W)).sum())
        assert abs(a - b) <= 1e-13 * max(abs(a), 1.0), (H, W, s)
        ones = R.adjoint(torch.ones((1, H // s, W // s), dtype=torch.float64), s, H, W)
        assert abs(float(ones.sum()) - (H // s) * (W // s)) <= 1e-12


def test_bp_symbols_are_exported():
    from ssl_amd import _lib
    import ssl_amd.losses as losses
    _lib.build()
    L = ctypes.CDLL(_lib.SO_PATH)
    hdr = open(_lib.HEADER).read()
    for name in BP_SYMBOLS:
        assert hasattr(L, name) and name in _lib.PROTOTYPES and f"{name}(" in hdr, name
    for name in ("imresize", "BackProjectionLoss"):
        assert callable(getattr(losses, name)), name
    m = losses.BackProjectionLoss()
    assert (m.loss_weight, m.reduction, m.scale) == (1.0, 'mean', 4)
    assert _lib.lib().ssg_abi_version() == 6
    # the training size: signs and partial sums -- nothing of input size
    nb = _lib.lib().ssg_bp_workspace_bytes(48, 192, 192, 4)
    assert 48 * 48 * 48 * 4 <= nb <= 2 * 48 * 48 * 48 * 4 + 65536
    for P, H, W, s in ((1, 6, 7, 4), (100000, 6, 6, 4), (3, 4, 5, 3), (7, 3, 4, 2), (5, 1000, 37, 2)):
        nb = _lib.lib().ssg_bp_workspace_bytes(P, H, W, s)
        assert 0 < nb <= 2 * P * (H // s) * (W // s) * 4 + 65536, (P, H, W, s)


def test_trip_shapes_cross_the_forward_workgroup_cap():
    """test_gpu_bp.TRIPS: the workspace behind the signs (one fp64 partial per forward workgroup) is the same for all
    four shapes -- the cap -- and larger than at 16 x 3 x 192 x 192, and each shape has more 16 x 8 output tiles than
    that.  Raising the cap fails here instead of sending the sweep back to one trip."""
    from ssl_amd import _lib
    from test_gpu_bp import TRIPS
    L = _lib.lib()

    def partials(s, shape):
        B, C, H, W = shape
        signs = -(-4 * B * C * (H // s) * (W // s) // 256) * 256
        return L.ssg_bp_workspace_bytes(B * C, H, W, s) - signs

    cap = {partials(s, shape) for s, shape in TRIPS}
    assert len(TRIPS) == 4 and len(cap) == 1
    cap = cap.pop()
    assert cap > partials(4, (16, 3, 192, 192)) == 864 * 8
    assert cap == partials(4, (100000, 3, 8, 8)) and cap % 8 == 0
    for s, (B, C, H, W) in TRIPS:
        tiles = B * C * -(-(H // s) // 8) * -(-(W // s) // 16)
        assert tiles > cap // 8, (s, B, C, H, W, tiles)


def test_bp_argument_checks_need_no_gpu():
    """SSG_E_BADARG (-1), SSG_E_TOOLARGE (-2), SSG_E_WORKSPACE (-3), SSG_E_IMAGESMALL (-4), SSG_E_ALIGN (-5): all
    decided before a launch (the pointers below are never dereferenced)."""
    from ssl_amd import _lib
    L = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)
    big = 1 << 40

    def down(x=one, P=3, H=24, W=20, s=4, y=one):
        return L.ssg_bp_downsample(x, P, H, W, s, y, None)

    def back(g=one, P=3, H=24, W=20, s=4, gx=one):
        return L.ssg_bp_downsample_backward(g, P, H, W, s, gx, None)

    def loss(x=one, lq=one, P=3, H=24, W=20, s=4, lw=1.0, out=one, ws=one, nb=big):
        return L.ssg_bp_loss(x, lq, P, H, W, s, lw, 1, out, None, None, ws, nb, None)

    for f in (down, back, loss):
        assert f(None) == -1 and f(P=0) == -1 and f(H=0) == -1 and f(W=-3) == -1
        assert f(s=1) == -1 and f(s=0) == -1 and f(s=-4) == -1
        assert f(s=5) == -2 and f(s=8) == -2 and f(P=1 << 15, H=1 << 8, W=1 << 8) == -2
        for s, p in ((2, 3), (3, 4), (4, 6)):
            assert f(s=s, H=p - 1) == -4 and f(s=s, W=p - 1) == -4, (s, p)
    assert down(y=None) == -1 and back(gx=None) == -1
    assert loss(lq=None) == -1 and loss(out=None) == -1 and loss(ws=None) == -1 and loss(lw=float('nan')) == -1
    # the order: a bad argument before the size, the size before the image, the image before the workspace
    assert loss(s=1, H=2) == -1 and loss(s=5, H=2) == -2 and loss(H=5, nb=0) == -4
    need = L.ssg_bp_workspace_bytes(3, 24, 20, 4)
    assert need > 0 and loss(nb=need - 1) == -3 and loss(nb=16) == -3 and loss(nb=0) == -3
    assert loss(ws=odd, nb=need) == -5 and loss(ws=odd, nb=need - 1) == -3
    for P, H, W, s in ((3, 5, 20, 4), (3, 24, 20, 5), (3, 24, 20, 1), (0, 24, 20, 4), (3, 3, 9, 3), (1, 2, 9, 2)):
        assert L.ssg_bp_workspace_bytes(P, H, W, s) == 0
    for P, H, W, s in ((3, 6, 6, 4), (3, 4, 4, 3), (1, 3, 3, 2)):
        assert L.ssg_bp_workspace_bytes(P, H, W, s) > 0


def test_imresize_outside_the_native_domain():
    from ssl_amd.losses import BackProjectionLoss, imresize
    x = torch.zeros(1, 3, 24, 24)
    with pytest.raises(ValueError, match="scale or sides"):
        imresize(x)
    with pytest.raises(ValueError, match="conflict"):
        imresize(x, scale=0.25, sides=(6, 6))
    for bad in (torch.zeros(24), torch.zeros(1, 1, 3, 24, 24)):
        with pytest.raises(ValueError, match="-dim Tensor"):
            imresize(bad, scale=0.25)
    for kw, word in ((dict(sides=(6, 6)), "sides"), (dict(scale=0.3), "scale"), (dict(scale=2.0), "scale"),
                     (dict(scale=1.0), "scale"), (dict(scale=1 / 5), "scale"), (dict(scale=1 / 8), "scale"),
                     (dict(scale=0.25, kernel='gaussian'), "kernel"),
                     (dict(scale=0.25, kernel=torch.ones(16, 16) / 256), "kernel"),
                     (dict(scale=0.25, antialiasing=False), "antialiasing"),
                     (dict(scale=0.25, padding_type='zero'), "padding_type")):
        with pytest.raises(NotImplementedError, match=word):
            imresize(x, **kw)
    with pytest.raises(NotImplementedError, match="dtype"):
        imresize(torch.zeros(1, 3, 24, 24, dtype=torch.uint8), scale=0.25)
    # inside the domain nothing above fires: the call reaches the engine, which has no CPU path
    for kw in (dict(scale=0.25), dict(scale=1 / 3, sigma=5, rotation_degree=30), dict(scale=0.5)):
        with pytest.raises(RuntimeError, match="GPU"):
            imresize(x, **kw)
    with pytest.raises(ValueError):
        BackProjectionLoss(reduction='none')
    for scale in (1, 5, 8, 2.5):
        with pytest.raises(NotImplementedError, match="scale"):
            BackProjectionLoss(scale=scale)
    assert BackProjectionLoss(0.37, 'sum', 2).scale == 2
