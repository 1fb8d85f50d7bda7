"""The multi-tensor criterion's kernels (ssl_amd/csrc/ssg_mcrit.hip behind engine.multi_pixel_loss and
ssl_amd.losses.PerceptualLoss) against the fp64 restatement tests/perceptual_reference.py, each result within the bound
derived there; the bit-for-bit promises (a pair's sum and gradient do not depend on the rest of the set, repeat calls,
ssg_pixel_grad's bits); every alignment and layout; the values that need care; the refusals; and the whole loss with
random VGG weights."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import perceptual_cases as C
import perceptual_reference as R

SENT = -123.25          # fills every gradient buffer and its guards before a call
GUARD = 8               # floats on either side of a gradient buffer (a multiple of 4: the view keeps its offset mod 16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda")


def _lib_():
    from ssl_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _geometry():
    L = _lib_()
    return L.ssg_mcrit_chunk(), L.ssg_mcrit_grid_cap()


def _kind_id(kind):
    from ssl_amd import _lib
    return _lib.CONSTANTS["SSG_PIX_" + kind.upper()]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _place(t, dev, offset=0):
    """t on the device as a flat view that starts `offset` floats behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[offset:offset + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4 * offset
    return v


def _grad_buffer(n, dev, offset=0):
    """(the whole buffer, the n-element view at `offset` floats behind a 16-byte boundary), all of it SENT"""
    buf = torch.full((GUARD + offset + n + GUARD,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _guards_intact(buf, offset, n):
    return bool((buf[:GUARD + offset] == SENT).all()) and bool((buf[GUARD + offset + n:] == SENT).all())


def _addresses(values):
    return np.asarray(values, dtype=np.uintp)


def _sums(xs, gs, ws, kind, eps=C.EPS):
    """ssg_mcrit_sums on flat device tensors: (status, the K + 1 doubles); the weights are taken as given"""
    L, K, dev = _lib_(), len(xs), xs[0].device
    px, pg = _addresses([t.data_ptr() for t in xs]), _addresses([t.data_ptr() for t in gs])
    counts, w = _addresses([t.numel() for t in xs]), np.asarray(ws, dtype=np.float64)
    nbytes = L.ssg_mcrit_workspace_bytes(K, counts.ctypes.data)
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    out = torch.full((K + 1,), 7.0, dtype=torch.float64, device=dev)
    rc = L.ssg_mcrit_sums(K, px.ctypes.data, pg.ctypes.data, counts.ctypes.data, w.ctypes.data, _kind_id(kind), eps,
                          work.data_ptr(), nbytes, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out


def _grads(xs, gs, outs, ws, kind, sums, coef, eps=C.EPS):
    """ssg_mcrit_grad into `outs` (None: a null address); returns the status"""
    L, K, dev = _lib_(), len(xs), xs[0].device
    px, pg = _addresses([t.data_ptr() for t in xs]), _addresses([t.data_ptr() for t in gs])
    po = _addresses([0 if t is None else t.data_ptr() for t in outs])
    counts, w = _addresses([t.numel() for t in xs]), np.asarray(ws, dtype=np.float64)
    c = torch.tensor([coef], dtype=torch.float64, device=dev)
    rc = L.ssg_mcrit_grad(K, px.ctypes.data, pg.ctypes.data, po.ctypes.data, counts.ctypes.data, w.ctypes.data,
                          _kind_id(kind), eps, sums.data_ptr(), c.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc


def _pixel_grad(x, g, kind, coef, eps=C.EPS):
    """ssg_pixel_grad on the pair, coef one double formed by the caller"""
    out = torch.empty_like(x)
    c = torch.tensor([coef], dtype=torch.float64, device=x.device)
    assert _lib_().ssg_pixel_grad(x.data_ptr(), g.data_ptr(), x.numel(), _kind_id(kind), eps, c.data_ptr(),
                                  out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return out


def _run_set(dev, xs, gs, ws, kind, coef, x_off=None, g_off=None, o_off=None, eps=C.EPS):
    """(sums, gradient views, whether every guard is intact) of one set placed at the given offsets"""
    K = len(xs)
    x_off, g_off, o_off = (v or [0] * K for v in (x_off, g_off, o_off))
    dx = [_place(t, dev, o) for t, o in zip(xs, x_off)]
    dg = [_place(t, dev, o) for t, o in zip(gs, g_off)]
    rc, sums = _sums(dx, dg, ws, kind, eps)
    assert rc == 0
    bufs = [_grad_buffer(t.numel(), dev, o) for t, o in zip(xs, o_off)]
    assert _grads(dx, dg, [v for _, v in bufs], ws, kind, sums, coef, eps) == 0
    intact = all(_guards_intact(b, o, t.numel()) for (b, _), o, t in zip(bufs, o_off, xs))
    return sums, [v for _, v in bufs], intact


def _check(kind, xs, gs, ws, coef, sums, grads, what, eps=C.EPS):
    """the kernel's S_k, total and gradients within the derived bound of the restatement; returns the shares"""
    want = R.criterion(xs, gs, ws, kind, eps, reduction="sum", upstream=coef)
    got = sums.cpu()
    s_share = max(R.share(got[k], want.S[k], want.S_bound[k]) for k in range(len(xs)))
    t_share = R.share(got[-1], want.total, want.total_bound)
    g_share = max(R.share(g, w.reshape(-1), b.reshape(-1)) for g, w, b in zip(grads, want.grads, want.grad_bound))
    print(f"{what} {kind}: share of the bound, S_k {s_share:.3e}, total {t_share:.3e}, gradients {g_share:.3e}")
    assert max(s_share, t_share, g_share) <= 1.0, (what, kind, s_share, t_share, g_share)
    return s_share, t_share, g_share


@pytest.mark.gpu
@pytest.mark.parametrize("kind", C.KINDS)
def test_sizes_around_the_chunk_within_the_bound(dev, kind):
    chunk, _ = _geometry()
    sizes = C.edge_sizes(chunk)
    xs, gs = C.pairs(sizes, 100)
    K = len(sizes)
    ws = [w / n for w, n in zip(C.weights(K), sizes)]
    sums, grads, intact = _run_set(dev, xs, gs, ws, kind, 0.75, x_off=[k % 4 for k in range(K)],
                                   g_off=[(k // 2) % 4 for k in range(K)], o_off=[(k + 1) % 4 for k in range(K)])
    assert intact
    _check(kind, xs, gs, ws, 0.75, sums, grads, "edge sizes")
    assert bool((grads[1] == 0).all())                               # (weight 0)
    assert L_workspace(sizes) == 8 * sum(-(-n // chunk) for n in sizes)


def L_workspace(sizes):
    counts = _addresses(sizes)
    return _lib_().ssg_mcrit_workspace_bytes(len(sizes), counts.ctypes.data)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", C.KINDS)
def test_multi_pixel_loss_on_vggs_size_ratios(dev, kind):
    """engine.multi_pixel_loss with autograd on five pairs of 32 : 16 : 8 : 4 : 1 elements: the loss, the gradient of
    every pred that wants one, none for the one that does not"""
    from ssl_amd import engine
    shapes = C.vgg_feature_shapes()
    xs, gs = C.pairs(shapes, 200)
    ws = list(C.KAIR_WEIGHTS)
    px = [t.to(dev).requires_grad_(k != 3) for k, t in enumerate(xs)]
    loss, sums = engine.multi_pixel_loss(px, [t.to(dev) for t in gs], ws, kind, C.EPS, "mean", return_sums=True)
    assert loss.dtype == torch.float32 and loss.shape == () and sums.shape == (6,)
    (loss * 0.75).backward()
    assert px[3].grad is None
    want = R.criterion(xs, gs, ws, kind, C.EPS, "mean", 0.75)
    shares = [R.share(loss, want.total, want.total_bound)]
    shares += [R.share(p.grad, w, b) for k, (p, w, b) in enumerate(zip(px, want.grads, want.grad_bound)) if k != 3]
    print(f"vgg ratios {kind}: share of the bound, loss {shares[0]:.3e}, gradients {max(shares[1:]):.3e}")
    assert max(shares) <= 1.0
    with torch.no_grad():
        again = engine.multi_pixel_loss(px, [t.to(dev) for t in gs], ws, kind, C.EPS)
    assert torch.equal(_bits(again), _bits(loss.detach()))
    with pytest.raises(ValueError, match="target"):
        engine.multi_pixel_loss(px[:1], [gs[0].to(dev).requires_grad_(True)], [1.0], kind)
    leaf = xs[4].to(dev).requires_grad_(True)
    up = torch.ones((), device=dev, requires_grad=True)
    g, = torch.autograd.grad(engine.multi_pixel_loss([leaf], [gs[4].to(dev)], [1.0], kind, C.EPS) * up, leaf,
                             create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5, 16, 17])
def test_a_pairs_bits_do_not_depend_on_the_set(dev, K):
    """S_k and grad_k alone and among K - 1 other pairs, twice, and against ssg_pixel_grad with coef w_k formed in fp64"""
    chunk, _ = _geometry()
    cycle = [5, chunk + 1, 3, 2 * chunk + 7, 1, chunk, 4, chunk - 1]
    sizes = [cycle[k % len(cycle)] + (k // len(cycle)) for k in range(K)]
    xs, gs = C.pairs(sizes, 300 + K)
    ws = [w / n for w, n in zip(C.weights(K, seed=K), sizes)]
    coef = -1.375
    for kind in ("l1", "charbonnier", "fro"):
        dx = [_place(t, dev, k % 4) for k, t in enumerate(xs)]
        dg = [_place(t, dev, (k + 2) % 4) for k, t in enumerate(gs)]
        rc, sums = _sums(dx, dg, ws, kind)
        rc2, sums2 = _sums(dx, dg, ws, kind)
        assert rc == 0 and rc2 == 0 and torch.equal(_bits(sums), _bits(sums2))
        outs = [torch.full_like(t, SENT) for t in dx]
        outs2 = [torch.full_like(t, SENT) for t in dx]
        assert _grads(dx, dg, outs, ws, kind, sums, coef) == 0 and _grads(dx, dg, outs2, ws, kind, sums, coef) == 0
        for k in range(K):
            rc, alone = _sums(dx[k:k + 1], dg[k:k + 1], ws[k:k + 1], kind)
            assert rc == 0 and torch.equal(_bits(alone[0]), _bits(sums[k])), (kind, k)
            one = torch.full_like(dx[k], SENT)
            assert _grads(dx[k:k + 1], dg[k:k + 1], [one], ws[k:k + 1], kind, alone, coef) == 0
            assert torch.equal(_bits(one), _bits(outs[k])) and torch.equal(_bits(outs2[k]), _bits(outs[k])), (kind, k)
            if kind != "fro":
                assert torch.equal(_bits(_pixel_grad(dx[k], dg[k], kind, coef * ws[k])), _bits(outs[k])), (kind, k)
        if K == 17:
            _check(kind, xs, gs, ws, coef, sums, outs, "17 pairs")


@pytest.mark.gpu
def test_a_grid_that_makes_a_second_trip(dev):
    chunk, cap = _geometry()
    sizes = C.second_trip_sizes(chunk, cap)
    assert sum(-(-n // chunk) for n in sizes) == cap + 2
    xs, gs = C.pairs(sizes, 400)
    ws = [1.0 / sizes[0], -2.0 / sizes[1], 0.5 / sizes[2]]
    dx, dg = [_place(t, dev, 1) for t in xs], [_place(t, dev, 1) for t in gs]
    rc, sums = _sums(dx, dg, ws, "mse")
    assert rc == 0
    outs = [torch.full_like(t, SENT) for t in dx]
    assert _grads(dx, dg, outs, ws, "mse", sums, 2.0) == 0
    _check("mse", xs, gs, ws, 2.0, sums, outs, "second trip")
    for k in range(3):
        rc, alone = _sums(dx[k:k + 1], dg[k:k + 1], ws[k:k + 1], "mse")
        assert rc == 0 and torch.equal(_bits(alone[0]), _bits(sums[k])), k
        assert torch.equal(_bits(_pixel_grad(dx[k], dg[k], "mse", 2.0 * ws[k])), _bits(outs[k])), k


@pytest.mark.gpu
def test_every_alignment_of_x_g_and_grad(dev):
    """the 64 offsets (x, g, grad) in 0 .. 3 of one pair of chunk + 7 elements, sixteen to a call: ssg_pixel_grad's bits
    every time, the guards on both sides of every gradient intact, and a sum that depends on x's offset alone"""
    chunk, _ = _geometry()
    n = chunk + 7
    x, g = C.pair(n, 500)
    w, coef, kind = 0.3 / n, 1.25, "charbonnier"
    want_grad = _pixel_grad(x.to(dev), g.to(dev), kind, coef * w)
    ref = R.criterion([x], [g], [w], kind, C.EPS, "sum", coef)
    by_x = {}
    combos = [(a, b, c) for a in range(4) for b in range(4) for c in range(4)]
    for at in range(0, 64, 16):
        part = combos[at:at + 16]
        sums, grads, intact = _run_set(dev, [x] * 16, [g] * 16, [w] * 16, kind, coef, [a for a, _, _ in part],
                                       [b for _, b, _ in part], [c for _, _, c in part])
        assert intact
        for (a, b, c), S, got in zip(part, sums[:16], grads):
            assert torch.equal(_bits(got), _bits(want_grad)), (a, b, c)
            assert R.share(S.cpu(), ref.S[0], ref.S_bound[0]) <= 1.0, (a, b, c)
            assert torch.equal(_bits(by_x.setdefault(a, S)), _bits(S)), (a, b, c)


@pytest.mark.gpu
def test_layouts_and_what_takes_the_torch_expression(dev):
    from ssl_amd import engine
    from ssl_amd.losses import perceptual, set_native_criteria
    shapes = [(2, 64, 8, 8), (2, 5, 3, 7)]
    xs, gs = C.pairs(shapes, 600)
    ws = [0.4, 1.5]
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)    # noqa: E731
    px = [cl(t).requires_grad_(True) for t in xs]
    loss = perceptual.multi_criterion(px, [cl(t) for t in gs], ws, "l1")
    assert type(loss.grad_fn).__name__.startswith("_MultiPixelFn")
    loss.backward()
    want = R.criterion(xs, gs, ws, "l1")
    assert R.share(loss, want.total, want.total_bound) <= 1.0
    for p, w, b in zip(px, want.grads, want.grad_bound):
        assert p.grad.stride() == p.stride() and R.share(p.grad, w, b) <= 1.0
    # mismatched strides, other dtypes, the switch: the reference's loop, bit for bit
    mixed = [xs[0].to(dev).requires_grad_(True), cl(xs[1]).requires_grad_(True)]
    mg = [cl(gs[0]), gs[1].to(dev)]
    assert not engine.multi_pair_is_native(mixed[0], mg[0])
    with pytest.raises(ValueError, match="dense strides"):
        engine.multi_pixel_loss(mixed, mg, ws, "l1")
    for kind in ("l1", "mse", "fro"):
        got = perceptual.multi_criterion(mixed, mg, ws, kind)
        assert "MultiPixel" not in type(got.grad_fn).__name__
        assert torch.equal(got, R.torch_loop(mixed, mg, ws, kind))
    for cast in (torch.float64, torch.float16, torch.bfloat16):
        a, b = [t.to(dev, cast) for t in xs], [t.to(dev, cast) for t in gs]
        assert torch.equal(perceptual.multi_criterion(a, b, ws, "l1"), R.torch_loop(a, b, ws, "l1"))
    empty = torch.empty(0, 3, device=dev)
    assert bool(torch.isnan(perceptual.multi_criterion([empty], [empty], [1.0], "l1")))
    a, b = [t.to(dev).requires_grad_(True) for t in xs], [t.to(dev) for t in gs]
    prev = set_native_criteria(False)
    try:
        off = perceptual.multi_criterion(a, b, ws, "fro")
        assert torch.equal(off, R.torch_loop(a, b, ws, "fro")) and "MultiPixel" not in type(off.grad_fn).__name__
    finally:
        set_native_criteria(prev)
    assert "MultiPixel" in type(perceptual.multi_criterion(a, b, ws, "fro").grad_fn).__name__


@pytest.mark.gpu
def test_values_that_need_care(dev):
    chunk, _ = _geometry()
    sizes = [chunk + 3, 70, 2 * chunk + 1]
    xs, gs = C.pairs(sizes, 700)
    ws = [1.0 / n for n in sizes]
    # equal elements: the L1 gradient is 0 there (either sign of zero), and exactly +-c elsewhere
    sums, grads, _ = _run_set(dev, xs, gs, ws, "l1", 2.0)
    for x, g, got, w in zip(xs, gs, grads, ws):
        same = (x == g).to(dev)
        assert int(same.sum()) > 0 and bool((got[same.reshape(-1)] == 0).all())
        assert bool((got[~same.reshape(-1)].abs() == np.float32(2.0 * w)).all())
    # a negative weight flips every bit's sign and nothing else
    _, neg, _ = _run_set(dev, xs, gs, [-w for w in ws], "mse", 2.0)
    _, pos, _ = _run_set(dev, xs, gs, ws, "mse", 2.0)
    for a, b in zip(neg, pos):
        assert torch.equal(_bits(a), _bits(-b))
    # a NaN element reaches its own tensor's sum and gradient element, and no other pair
    bad = [t.clone() for t in xs]
    bad[1][17] = float("nan")
    for kind in ("l1", "fro"):
        clean, clean_grads, _ = _run_set(dev, xs, gs, ws, kind, 1.0)
        sums, grads, _ = _run_set(dev, bad, gs, ws, kind, 1.0)
        assert bool(torch.isnan(sums[1])) and bool(torch.isnan(sums[3]))
        assert torch.equal(_bits(sums[[0, 2]]), _bits(clean[[0, 2]]))
        assert torch.equal(_bits(grads[0]), _bits(clean_grads[0])) and torch.equal(_bits(grads[2]), _bits(clean_grads[2]))
        nan = torch.isnan(grads[1])
        assert bool(nan[17]) and (int(nan.sum()) == 1 if kind == "l1" else bool(nan.all()))
    # S_k = 0 under fro: a zero gradient, no NaN; the other pairs as before
    zero = [xs[0], gs[1].clone(), xs[2]]
    sums, grads, _ = _run_set(dev, zero, gs, ws, "fro", 1.0)
    assert float(sums[1]) == 0.0 and bool((grads[1] == 0).all()) and bool(torch.isfinite(sums).all())
    assert torch.equal(_bits(grads[0]), _bits(clean_grads[0]))


@pytest.mark.gpu
def test_a_null_gradient_pointer_skips_its_pair(dev):
    chunk, _ = _geometry()
    sizes = [chunk + 2, 3 * chunk + 5, 9]
    xs, gs = C.pairs(sizes, 800)
    ws = [1.0, 0.5, 2.0]
    dx, dg = [t.to(dev) for t in xs], [t.to(dev) for t in gs]
    rc, sums = _sums(dx, dg, ws, "mse")
    bufs = [_grad_buffer(n, dev, 1) for n in sizes]
    full = [v for _, v in bufs]
    assert rc == 0 and _grads(dx, dg, [full[0], None, full[2]], ws, "mse", sums, 1.0) == 0
    assert bool((bufs[1][0] == SENT).all())                          # untouched
    assert all(_guards_intact(b, 1, n) for (b, _), n in zip(bufs, sizes))
    for k in (0, 2):
        assert torch.equal(_bits(full[k]), _bits(_pixel_grad(dx[k], dg[k], "mse", ws[k])))
    assert _grads(dx, dg, [None, None, None], ws, "mse", sums, 1.0) == 0


@pytest.mark.gpu
def test_every_status_code_with_the_outputs_untouched(dev):
    L = _lib_()
    chunk, _ = _geometry()
    n = chunk + 9
    x, g = torch.ones(n + 1, device=dev), torch.zeros(n + 1, device=dev)
    out = torch.full((n + 1,), SENT, device=dev)
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    coef = torch.ones(2, dtype=torch.float64, device=dev)
    work = torch.empty(64, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p
    A = _addresses
    ok = dict(K=1, x=A([x.data_ptr()]), g=A([g.data_ptr()]), o=A([out.data_ptr()]), n=A([n]), w=np.asarray([1.0]),
              kind=0, eps=0.0, work=work.data_ptr(), bytes=16, sums=sums.data_ptr(), coef=coef.data_ptr())

    def call_sums(**kw):
        a = dict(ok, **kw)
        ptr = lambda v: p(None) if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)   # noqa: E731
        return L.ssg_mcrit_sums(a["K"], ptr(a["x"]), ptr(a["g"]), ptr(a["n"]), ptr(a["w"]), a["kind"], a["eps"],
                                ptr(a["work"]), a["bytes"], ptr(a["sums"]), _stream())

    def call_grad(**kw):
        a = dict(ok, **kw)
        ptr = lambda v: p(None) if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)   # noqa: E731
        return L.ssg_mcrit_grad(a["K"], ptr(a["x"]), ptr(a["g"]), ptr(a["o"]), ptr(a["n"]), ptr(a["w"]), a["kind"],
                                a["eps"], ptr(a["sums"]), ptr(a["coef"]), _stream())

    bad = [dict(K=0), dict(x=None), dict(g=None), dict(n=None), dict(w=None), dict(x=A([0])), dict(g=A([0])),
           dict(n=A([0])), dict(kind=4), dict(kind=-1), dict(w=np.asarray([float("nan")])), dict(eps=-1.0),
           dict(eps=float("inf"))]
    for kw in bad:
        assert call_sums(**kw) == -1 and call_grad(**kw) == -1, kw
    assert call_sums(work=None) == -1 and call_sums(sums=None) == -1
    assert call_grad(o=None) == -1 and call_grad(sums=None) == -1 and call_grad(coef=None) == -1
    huge = A([(2 ** 31) * chunk])
    assert call_sums(n=huge) == -2 and call_grad(n=huge) == -2
    assert L.ssg_mcrit_workspace_bytes(1, huge.ctypes.data) == 0
    assert L.ssg_mcrit_workspace_bytes(1, ok["n"].ctypes.data) == 16
    assert call_sums(bytes=15) == -3 and call_sums(bytes=8) == -3
    assert call_sums(work=work.data_ptr() + 4) == -5 and call_sums(sums=sums.data_ptr() + 4) == -5
    assert call_sums(x=A([x.data_ptr() + 2])) == -5 and call_sums(g=A([g.data_ptr() + 1])) == -5
    assert call_grad(o=A([out.data_ptr() + 2])) == -5 and call_grad(coef=coef.data_ptr() + 4) == -5
    assert call_grad(sums=sums.data_ptr() + 4) == -5 and call_grad(x=A([x.data_ptr() + 2])) == -5
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((out == SENT).all())           # nothing was launched
    assert call_sums() == 0 and call_grad() == 0
    torch.cuda.synchronize()
    assert sums.tolist() == [float(n), float(n)] and bool((out[:n] == 1.0).all()) and float(out[n]) == SENT
    assert call_sums(x=A([x.data_ptr() + 4])) == 0                           # (a float's own alignment is enough)


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["l1", "l2", "fro"])
def test_the_whole_loss_with_random_vgg_weights(dev, criterion):
    """PerceptualLoss at 2 x 3 x 32 x 32 on the kernels against the torch formulation (the switch off) on the same GPU.
    Both terms of the loss are held to the kernel's derived bound of the fp64 restatement on the features.
    The gradient with respect to x passes through VGG's backward, for which no bound is derived here; it is held to the
    reference's own error instead: the torch formulation in fp32 against the same formulation in fp64 (network and
    criterion) differs by E in the largest element.  The two fp32 gradients differ in the rounding of the feature
    gradients alone (at most TORCH_GRAD_U + 1 roundings per element, below what the network's fp32 backward adds to
    either), so each lies within E of the fp64 one up to its own draw of rounding noise: 4 E between them."""
    from ssl_amd.losses import PerceptualLoss, kair, set_native_criteria
    state = C.vgg_state_dict("vgg19", seed=0)
    layer_weights = dict(zip(C.VGG19_TAPS, C.KAIR_WEIGHTS))
    crit = PerceptualLoss(layer_weights, perceptual_weight=0.8, style_weight=0.3, criterion=criterion,
                          vgg_weights=state).to(dev)
    x0, gt = (t.to(dev) for t in C.images())

    def run(module, x, gt, native=True):
        """(percep, style, d(percep + style)/dx, the features of x, the features of gt): the network runs once for each
        image, and the loss is formed on those very features (its `.vgg` replays them), with the kernels or without"""
        x = x.clone().requires_grad_(True)
        feats = module.vgg(x)
        with torch.no_grad():
            gfeats = module.vgg(gt)
        out = []
        for on in ((True, False) if native else (False,)):
            prev = set_native_criteria(on)
            module.vgg = _Replay(module.vgg, [feats, gfeats])
            try:
                percep, style = module(x, gt)
            finally:
                module.vgg = module.vgg.inner
                set_native_criteria(prev)
            gx, = torch.autograd.grad(percep + style, x, retain_graph=True)
            out.append((percep.detach(), style.detach(), gx))
        return out, list(feats.values()), list(gfeats.values())

    ((percep, style, gx), (t_percep, t_style, t_gx)), fx, fg = run(crit, x0, gt)
    crit64 = PerceptualLoss(layer_weights, perceptual_weight=0.8, style_weight=0.3, criterion=criterion,
                            vgg_weights=state).to(dev).double()
    ((_, _, gx64),), _, _ = run(crit64, x0.double(), gt.double(), native=False)
    kind = {"l1": "l1", "l2": "mse", "fro": "fro"}[criterion]
    fx = [v.detach() for v in fx]
    ws = [w * 0.8 for w in C.KAIR_WEIGHTS]
    want = R.criterion(fx, fg, ws, kind)
    assert R.share(percep, want.total, want.total_bound) <= 1.0
    assert R.share(t_percep, want.total, want.torch_total_bound) <= 1.0
    gram = [crit._gram_mat(v) for v in fx], [crit._gram_mat(v) for v in fg]
    want_style = R.criterion(gram[0], gram[1], [w * 0.3 for w in C.KAIR_WEIGHTS], kind)
    assert R.share(style, want_style.total, want_style.total_bound) <= 1.0
    E = float((t_gx.double() - gx64).abs().max())
    diff = float((gx - t_gx).abs().max())
    print(f"whole loss {criterion}: |grad_x native - torch| {diff:.3e}, the torch formulation's own error E {E:.3e}, "
          f"max |grad_x| {float(gx64.abs().max()):.3e}")
    assert float(gx.abs().max()) > 0 and diff <= 4 * E
    if criterion != "fro":
        other = kair.PerceptualLoss(list(C.VGG19_TAP_INDICES), list(C.KAIR_WEIGHTS), criterion, vgg_weights=state).to(dev)
        other.vgg = _Replay(other.vgg, [fx, fg])
        loss = other(x0, gt)
        assert "MultiPixel" not in type(loss.grad_fn).__name__ and loss.dtype == torch.float32    # (nothing wants a gradient)
        want = R.criterion(fx, fg, C.KAIR_WEIGHTS, kind)
        assert R.share(loss, want.total, want.total_bound) <= 1.0


class _Replay(torch.nn.Module):
    """stands in for a loss's `.vgg` for one forward: returns, call by call, the features already computed (so that the
    restatement sees the very tensors the loss saw, whatever convolution algorithm the library picks from call to call)"""

    def __init__(self, inner, outputs):
        super().__init__()
        self.inner, self.outputs, self.calls = inner, outputs, 0

    def forward(self, x):
        self.calls += 1
        return self.outputs[self.calls - 1]


def poison_cases():
    """The outputs the LDS-poison test compares bit for bit (test_gpu_perceptual_poison.py): every kind over the sizes
    around the chunk, seventeen pairs (two launches that carry the total on), and the grid's second trip."""
    dev = torch.device("cuda")
    chunk, cap = _geometry()
    out = []
    sizes = C.edge_sizes(chunk)
    xs, gs = C.pairs(sizes, 100)
    ws = [w / n for w, n in zip(C.weights(len(sizes)), sizes)]
    for kind in C.KINDS:
        sums, grads, _ = _run_set(dev, xs, gs, ws, kind, 0.75, x_off=[k % 4 for k in range(len(sizes))])
        out += [sums] + grads
    sizes = [5 + 3 * k for k in range(17)]
    xs, gs = C.pairs(sizes, 317)
    sums, grads, _ = _run_set(dev, xs, gs, [1.0 / n for n in sizes], "fro", 1.0)
    out += [sums] + grads
    sizes = C.second_trip_sizes(chunk, cap)
    xs, gs = C.pairs(sizes, 400)
    sums, grads, _ = _run_set(dev, xs, gs, [1.0 / n for n in sizes], "l1", 1.0)
    out += [sums, grads[1]]
    return out
