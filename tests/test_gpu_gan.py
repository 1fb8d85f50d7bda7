"""The GAN criteria's kernels (ssl_amd/csrc/ssg_gan.hip behind ssl_amd.losses.GANLoss / MultiScaleGANLoss and the
relativistic helpers) against the fp64 restatement tests/gan_reference.py, each result within the bound derived there
(the one the reference's own fp32 results are held to in test_cpu_gan.py), evaluated at the same fp32 d: the loss, and the
gradient element by element, for every kind, sign and label over the shapes, alignments and contents of
tests/gan_cases.py; NaN propagation, the multi-scale and relativistic forms, routing and the bit-for-bit promises."""
import ctypes
import functools

import pytest
import torch

import gan_cases as C
import gan_reference as R


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _cap():
    from ssl_amd import _lib
    return _lib.lib().ssg_gan_grid_cap()


def _crit(gan_type, labels=(1.0, 0.0), weight=C.WEIGHT, multi=False):
    from ssl_amd.losses import GANLoss, MultiScaleGANLoss
    return (MultiScaleGANLoss if multi else GANLoss)(gan_type, labels[0], labels[1], loss_weight=weight)


def _to_device(x, dev, offset):
    """x on the device as a leaf; offset: as a view that starts that many floats (True: one) into its buffer (not 16-byte
    aligned)."""
    if not offset:
        return x.to(dev)
    k = int(offset)
    buf = torch.empty(x.numel() + k, dtype=x.dtype, device=dev)
    v = buf[k:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 * k and v.is_contiguous()
    return v


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _within(got, want, bound, what):
    got, want = got.double().cpu(), torch.as_tensor(want, dtype=torch.float64)
    d = (got - want).abs()
    share = R.share(got, want, bound)
    print(f"{what}: max |diff| {float(d.max()):.3e}, share of the bound {share:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert bool((d <= torch.as_tensor(bound, dtype=torch.float64)).all()), (what, share)
    return share


def _plain(dev, x, config, offset=False, weight=C.WEIGHT):
    """One module call and its backward on the GPU: (loss, grad) on the CPU and the loss's grad_fn name."""
    gan_type, labels, real, disc, upstream = config
    a = _to_device(x, dev, offset).requires_grad_(True)
    loss = _crit(gan_type, labels, weight)(a, real, disc)
    (loss * upstream).backward()
    return loss.detach().cpu(), a.grad.cpu(), type(loss.grad_fn).__name__


@pytest.mark.gpu
@pytest.mark.parametrize("content", C.CONTENTS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_plain_loss_and_gradient_within_the_bound(dev, shape, content):
    x = C.content(content, C.shape_of(shape, _cap()))
    d = R.delta(x)
    for config in C.CONFIGS:
        gan_type, labels, real, disc, upstream = config
        w = 1.0 if disc else C.WEIGHT                         # loss_weight is the generator's alone
        sp = R.spec(gan_type, real, disc, *labels)
        want_l, want_g = R.plain(x, sp, w, upstream)
        loss, grad, node = _plain(dev, x, config, offset=shape == "view67")
        assert "PlainCriterion" in node and loss.shape == () and loss.dtype == torch.float32 and grad.shape == x.shape
        what = f"{shape} {content} {gan_type} labels={labels} real={real} disc={disc} upstream={upstream}"
        _within(loss, want_l, R.loss_bound(d, sp, w), what + " loss")
        _within(grad, want_g, R.grad_bound(d, sp, upstream * w / d.numel()), what + " grad")


@pytest.mark.gpu
def test_hinge_derivative_is_zero_at_its_corner_and_nothing_overflows(dev):
    x = C.content("special", C.shape_of("2x1x7x5", _cap()))
    flat = x.view(-1)
    for real, corner in ((True, 1.0), (False, -1.0)):
        _, grad, _ = _plain(dev, x, ("hinge", (1.0, 0.0), real, True, 1.0))
        at = flat == corner
        assert int(at.sum()) == 3 and not bool(grad.view(-1)[at].any())
        assert bool((grad.view(-1)[flat == corner * (1 - 2.0 ** -24)] != 0).all())      # one ulp inside: the slope
    for gan_type in ("vanilla", "wgan_softplus"):
        for real in (True, False):
            loss, grad, _ = _plain(dev, x, (gan_type, (1.0, 0.0), real, True, 1.0))
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    # d = +-100 gives 100 or 0
    big = torch.tensor([100.0, -100.0])
    for real, want in ((True, (0.0, 100.0)), (False, (100.0, 0.0))):
        for k in range(2):
            loss, _, _ = _plain(dev, big[k:k + 1].reshape(1, 1), ("vanilla", (1.0, 0.0), real, True, 1.0))
            assert abs(float(loss) - want[k]) <= 1e-5 * want[k] + 1e-30


@pytest.mark.gpu
@pytest.mark.parametrize("where", ("first", "last"))
def test_a_nan_reaches_the_sum_and_its_own_gradient_alone(dev, where):
    from ssl_amd.losses import set_native_criteria
    x = C.content("normal", (67,)).clone()
    at = 0 if where == "first" else 66
    x[at] = float("nan")
    for config in C.CONFIGS:
        loss, grad, node = _plain(dev, x, config, offset=True)
        assert "PlainCriterion" in node and bool(torch.isnan(loss)), config
        prev = set_native_criteria(False)
        try:
            _, want, _ = _plain(dev, x, config, offset=True)
        finally:
            set_native_criteria(prev)
        assert torch.equal(torch.isnan(grad), torch.isnan(want)), config       # (l' = s of wgan and hinge is no NaN)
        kind = R.spec(config[0], config[2], config[3])[0]
        if kind in (R.BCE, R.LS, R.SOFTPLUS):
            assert bool(torch.isnan(grad[at])) and int(torch.isnan(grad).sum()) == 1, config
    # relativistic: the NaN belongs to `other`, the shift is NaN and every element of pred's gradient with it
    pred = C.content("normal", (2, 1, 7, 5)).to(dev).requires_grad_(True)
    for gan_type in ("vanilla", "lsgan", "wgan_softplus"):
        loss = _crit(gan_type).relativistic_term(pred, _to_device(x, dev, True), True, is_disc=True)
        pred.grad = None
        loss.backward()
        assert "RelativisticTerm" in type(loss.grad_fn).__name__
        assert bool(torch.isnan(loss)) and bool(torch.isnan(pred.grad).all()), gan_type


@pytest.mark.gpu
def test_loss_weight_is_not_applied_to_a_discriminator(dev):
    x = C.content("normal", (2, 1, 7, 5))
    for gan_type in R.BASICSR_TYPES:
        base = (gan_type, (1.0, 0.0), True)
        d_w, gd_w, _ = _plain(dev, x, base + (True, 1.0), weight=0.3)
        d_1, gd_1, _ = _plain(dev, x, base + (True, 1.0), weight=1.0)
        assert torch.equal(_bits(d_w), _bits(d_1)) and torch.equal(_bits(gd_w), _bits(gd_1))
        g_w, _, _ = _plain(dev, x, base + (False, 1.0), weight=0.3)
        g_1, _, _ = _plain(dev, x, base + (False, 1.0), weight=1.0)
        assert abs(float(g_w) - 0.3 * float(g_1)) <= 4 * R.U * abs(float(g_1))


@pytest.mark.gpu
def test_discriminator_pair_graph_and_multiscale(dev):
    """(cri(real, True) + cri(fake, False)) / 2, the upstream 0.5 reaching both nodes through the graph; then
    MultiScaleGANLoss on three tensors of different sizes and on a list of lists."""
    real, fake = C.rel_inputs("sizes_differ", _cap())
    for gan_type, labels in C.REL_TYPES:
        crit = _crit(gan_type, labels)
        a, b = real.to(dev).requires_grad_(True), fake.to(dev).requires_grad_(True)
        loss = (crit(a, True, is_disc=True) + crit(b, False, is_disc=True)) / 2
        loss.backward()
        total, bound = 0.0, 0.0
        for x, leaf, is_real in ((real, a, True), (fake, b, False)):
            sp = R.spec(gan_type, is_real, True, *labels)
            l, g = R.plain(x, sp, 1.0, 0.5)
            total, bound = total + float(l) / 2, bound + R.loss_bound(R.delta(x), sp) / 2
            _within(leaf.grad, g, R.grad_bound(R.delta(x), sp, 0.5 / x.numel()), f"pair {gan_type} grad")
        _within(loss.detach(), total, bound + 2 * R.U * abs(total), f"pair {gan_type} loss")
    scales = [C.content("normal", s, seed=k) for k, s in enumerate(((2, 1, 9, 9), (2, 1, 5, 4), (2, 1, 2, 1)))]
    for gan_type, real_t, disc in (("vanilla", True, False), ("hinge", False, True), ("lsgan", False, False)):
        crit = _crit(gan_type, multi=True)
        w, sp = (1.0 if disc else C.WEIGHT), R.spec(gan_type, real_t, disc)
        L, grads = R.multiscale(scales, sp, w)
        bound = sum(R.loss_bound(R.delta(t), sp, w) for t in scales) / 3 + 4 * R.U * abs(float(L))
        for nested in (False, True):
            leaves = [t.to(dev).requires_grad_(True) for t in scales]
            feature = torch.zeros(2, 3, 4, 4, device=dev)
            arg = [[feature, leaves[0]], [feature, feature, leaves[1]], [leaves[2]]] if nested else leaves
            loss = crit(arg, real_t, disc)
            loss.backward()
            _within(loss.detach(), L, bound, f"multiscale {gan_type} nested={nested} loss")
            for leaf, g, t in zip(leaves, grads, scales):
                _within(leaf.grad, g, R.grad_bound(R.delta(t), sp, w / (3 * t.numel())), f"multiscale {gan_type} grad")
        assert "PlainCriterion" in type(crit(leaves[0], real_t, disc).grad_fn).__name__        # a tensor: GANLoss itself


def _relativistic(dev, crit, form, real, fake, offset=False, upstream=1.0):
    need = C.rel_needs(form)
    a = _to_device(real, dev, offset).requires_grad_(need[0])
    b = _to_device(fake, dev, offset).requires_grad_(need[1])
    if form == "gen_real":
        loss = crit.relativistic_generator(a, b)
    else:
        loss = R.rel_form(form, a, b, crit.relativistic_term, crit.relativistic_generator)
    (loss * upstream).backward()
    node = loss.grad_fn                                       # (a discriminator's line multiplies its term by 0.5)
    node = node.next_functions[0][0] if type(node).__name__.startswith("MulBackward") else node
    return (loss.detach().cpu(), None if a.grad is None else a.grad.cpu(), None if b.grad is None else b.grad.cpu(),
            type(node).__name__)


def _relativistic_restated(gan_type, labels, form, real, fake, upstream):
    """(L, dL/dreal, dL/dfake, their three bounds) at the restatement's shift, the fp64 mean rounded to fp32."""
    if form.startswith("gen"):
        sa, sb = R.spec(gan_type, False, False, *labels), R.spec(gan_type, True, False, *labels)
        L, gr, gf = R.relativistic_generator(real, fake, sa, sb, C.WEIGHT, upstream)
        return (L, gr, gf) + R.generator_bounds(real, fake, sa, sb, C.WEIGHT, upstream)
    pred, other, is_real = (real, fake, True) if form == "disc_real" else (fake, real, False)
    sp = R.spec(gan_type, is_real, True, *labels)
    L, gp, _, _ = R.relativistic_term(pred, other, sp, 1.0, 0.5 * upstream)
    bl, bp, _ = R.term_bounds(pred, other, sp, 1.0, 0.5 * upstream)
    out = (L * 0.5, gp, None, bl * 0.5 + R.U * abs(float(L)), bp, None)
    return out if form == "disc_real" else (out[0], None, out[1], out[3], None, out[4])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [p[0] for p in C.REL_PAIRS])
def test_relativistic_term_and_generator_within_the_bound(dev, pair):
    real, fake = C.rel_inputs(pair, _cap())
    # (past the grid cap the fp64 yardstick of a million elements takes a moment: two criteria, three forms)
    types, forms = (C.REL_TYPES, C.REL_FORMS) if pair != "trip" else (C.REL_TYPES[::4], C.REL_FORMS[1:4])
    for gan_type, labels in types:
        crit = _crit(gan_type, labels)
        for k, form in enumerate(forms):
            upstream = (1.0, 0.5)[k % 2]
            loss, gr, gf, node = _relativistic(dev, crit, form, real, fake, offset=pair == "views", upstream=upstream)
            need = C.rel_needs(form)
            assert ("RelativisticPair" if form.startswith("gen") else "RelativisticTerm") in node
            assert (gr is not None, gf is not None) == need
            L, wr, wf, bl, br, bf = _relativistic_restated(gan_type, labels, form, real, fake, upstream)
            what = f"relativistic {pair} {gan_type} {form}"
            _within(loss, L, bl, what + " loss")
            if need[0]:
                _within(gr, wr, br, what + " grad_real")
            if need[1]:
                _within(gf, wf, bf, what + " grad_fake")
    # the gradient of a term reaches `other` through the mean alone: a constant
    crit = _crit("vanilla")
    a, b = real.to(dev).requires_grad_(True), fake.to(dev).requires_grad_(True)
    crit.relativistic_term(a, b, True).backward()
    sp = R.spec("vanilla", True)
    _, gp, go, _ = R.relativistic_term(real, fake, sp, C.WEIGHT)
    _, bp, bo = R.term_bounds(real, fake, sp, C.WEIGHT)
    _within(a.grad, gp, bp, f"term {pair} grad_pred")
    _within(b.grad, go, bo, f"term {pair} grad_other")


@pytest.mark.gpu
def test_two_identical_calls_give_identical_bits(dev):
    for shape in ("2x1x7x5", "view67", "trip"):
        x = C.content("normal", C.shape_of(shape, _cap()))
        for config in (C.CONFIGS[2], C.CONFIGS[11], C.CONFIGS[12]):
            one = _plain(dev, x, config, offset=shape == "view67")
            two = _plain(dev, x, config, offset=shape == "view67")
            assert torch.equal(_bits(one[0]), _bits(two[0])) and torch.equal(_bits(one[1]), _bits(two[1]))
    real, fake = C.rel_inputs("trip", _cap())
    one = _relativistic(dev, _crit("vanilla"), "gen_both", real, fake)
    two = _relativistic(dev, _crit("vanilla"), "gen_both", real, fake)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(one[:3], two[:3]))


@pytest.mark.gpu
def test_offset_gradient_takes_the_wide_stores_to_the_same_bits(dev):
    """The module's gradient buffer is aligned, so an offset input stores one by one; through the C ABI a gradient
    buffer with the input's own misalignment takes the 16-byte stores behind a scalar head: the same bits."""
    from ssl_amd import _lib
    L = _lib.lib()
    x = C.content("special", (67,))
    a = _to_device(x, dev, True)
    coef = torch.tensor([0.25, -0.125], dtype=torch.float64, device=dev)
    shift = torch.tensor([0.375], dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for kind in range(5):
        outs = []
        for off in (0, 1, 2):
            buf = torch.zeros(67 + 4, dtype=torch.float32, device=dev)
            g = buf[off:off + 67]
            _lib.check(L.ssg_gan_grad(a.data_ptr(), 67, kind, -1.0, 0.9, shift.data_ptr(), coef.data_ptr(), g.data_ptr(),
                                      stream))
            assert not bool(buf[:off].any()) and not bool(buf[off + 67:].any())      # nothing outside the 67
            outs.append(g.clone())
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
        d = R.delta(x, 0.375)
        want = 0.25 * R.dell(d, kind, -1.0, R.fl32(0.9)) - 0.125
        _within(outs[0], want, R.grad_bound(d, (kind, -1.0, R.fl32(0.9)), 0.25) + R.U * want.abs(), f"C ABI kind {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("offset", (0, 1, 2, 3))
def test_heads_and_tails_of_one_two_and_three(dev, offset):
    """Eleven elements 0, 1, 2 and 3 floats behind a 16-byte boundary: a scalar head of 0, 3, 2 and 1, two float4, a tail
    of 3, 0, 1 and 2.  The sums and the gradient through the module (its gradient buffer is aligned), then the gradient
    through the C ABI into a buffer with the input's own alignment (16-byte stores) and into one a float further (stored
    one by one): the same bits."""
    from ssl_amd import _lib
    L = _lib.lib()
    x = C.content("special", (11,))
    d = R.delta(x)
    for config in C.CONFIGS:
        gan_type, labels, real, disc, upstream = config
        w = 1.0 if disc else C.WEIGHT
        sp = R.spec(gan_type, real, disc, *labels)
        want_l, want_g = R.plain(x, sp, w, upstream)
        loss, grad, node = _plain(dev, x, config, offset=offset)
        assert "PlainCriterion" in node
        what = f"offset {offset} {gan_type} labels={labels} real={real} disc={disc}"
        _within(loss, want_l, R.loss_bound(d, sp, w), what + " loss")
        _within(grad, want_g, R.grad_bound(d, sp, upstream * w / d.numel()), what + " grad")
    a = _to_device(x, dev, offset)
    coef = torch.tensor([0.25, -0.125], dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for kind in range(5):
        outs = []
        for off in (offset, (offset + 1) % 4):
            buf = torch.zeros(11 + 8, dtype=torch.float32, device=dev)
            g = buf[off:off + 11]
            _lib.check(L.ssg_gan_grad(a.data_ptr(), 11, kind, 1.0, 0.9, None, coef.data_ptr(), g.data_ptr(), stream))
            assert not bool(buf[:off].any()) and not bool(buf[off + 11:].any())      # nothing outside the 11
            outs.append(g.clone())
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
        want = 0.25 * R.dell(d, kind, 1.0, R.fl32(0.9)) - 0.125
        _within(outs[0], want, R.grad_bound(d, (kind, 1.0, R.fl32(0.9)), 0.25) + R.U * want.abs(), f"C ABI kind {kind}")


@pytest.mark.gpu
def test_routing_native_node_torch_path_and_the_switch(dev):
    from ssl_amd.losses import set_native_criteria
    x = C.content("normal", (2, 1, 7, 5))
    crit = _crit("vanilla", (0.9, 0.1))
    for dtype in (torch.float64, torch.bfloat16):
        a = x.to(dev, dtype).requires_grad_(True)
        loss = crit(a, True)
        loss.backward()
        assert "Criterion" not in type(loss.grad_fn).__name__ and loss.dtype == dtype
        b = x.to(dev, dtype).requires_grad_(True)
        want = crit._torch(b, True, False)
        want.backward()
        assert torch.equal(loss.detach(), want.detach()) and torch.equal(a.grad, b.grad)
    a = x.to(dev).t().contiguous().t() if x.dim() == 2 else x.to(dev).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not a.is_contiguous()
    a.requires_grad_(True)
    loss = crit(a, False, is_disc=True)
    loss.backward()
    want_l, want_g, node = _plain(dev, x, ("vanilla", (0.9, 0.1), False, True, 1.0))
    assert "PlainCriterion" in type(loss.grad_fn).__name__ == node
    assert torch.equal(loss.detach().cpu(), want_l) and torch.equal(a.grad.cpu(), want_g)       # made contiguous
    prev = set_native_criteria(False)
    try:
        b = x.to(dev).requires_grad_(True)
        off = crit(b, False, is_disc=True)
        assert "Criterion" not in type(off.grad_fn).__name__
        g, = torch.autograd.grad(off, b, create_graph=True)
        g.square().sum().backward()                           # a second derivative through the criterion
        assert b.grad is not None
        assert "Relativistic" not in type(crit.relativistic_generator(b, b * 0.5).grad_fn).__name__
    finally:
        set_native_criteria(prev)
    assert abs(float(off) - float(want_l)) <= 2 * R.loss_bound(R.delta(x), R.spec("vanilla", False, True, 0.9, 0.1))
    assert "PlainCriterion" in type(crit(x.to(dev).requires_grad_(True), True).grad_fn).__name__
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                             # on the current stream of the tensor's device
        c = x.to(dev).requires_grad_(True)
        l2 = crit(c, False, is_disc=True)
        l2.backward()
    side.synchronize()
    assert torch.equal(l2.detach().cpu(), want_l) and torch.equal(c.grad.cpu(), want_g)


@pytest.mark.gpu
def test_refusals_on_the_device(dev):
    from ssl_amd import _lib
    L = _lib.lib()
    x = torch.ones(70, device=dev)
    work = torch.empty(L.ssg_gan_workspace_bytes(), dtype=torch.uint8, device=dev)
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    coef = torch.ones(2, dtype=torch.float64, device=dev)
    grad = torch.full((70,), 7.0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = ctypes.c_void_p
    bad = [(None, 70, 0, 1.0), (x.data_ptr(), 0, 0, 1.0), (x.data_ptr(), 70, 5, 1.0), (x.data_ptr(), 70, -1, 1.0),
           (x.data_ptr(), 70, 2, 0.0), (x.data_ptr(), 70, 3, 2.0), (x.data_ptr(), 70, 4, float("nan"))]
    for ptr, n, kind, sign in bad:
        assert L.ssg_gan_sums(p(ptr), n, kind, sign, 1.0, None, work.data_ptr(), sums.data_ptr(), stream) == -1
        assert L.ssg_gan_grad(p(ptr), n, kind, sign, 1.0, None, coef.data_ptr(), grad.data_ptr(), stream) == -1
    assert L.ssg_gan_sums(x.data_ptr(), 70, 0, 1.0, 1.0, None, None, sums.data_ptr(), stream) == -1
    assert L.ssg_gan_sums(x.data_ptr(), 70, 0, 1.0, 1.0, None, work.data_ptr(), None, stream) == -1
    assert L.ssg_gan_grad(x.data_ptr(), 70, 0, 1.0, 1.0, None, None, grad.data_ptr(), stream) == -1
    assert L.ssg_gan_grad(x.data_ptr(), 70, 0, 1.0, 1.0, None, coef.data_ptr(), None, stream) == -1
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((grad == 7.0).all())          # nothing was launched
    assert L.ssg_gan_sums(x.data_ptr(), 70, 2, 1.0, 0.0, None, work.data_ptr(), sums.data_ptr(), stream) == 0
    assert sums.tolist() == [70.0, 70.0]                                     # LINEAR, s = 1: the plain sum, and n
    with pytest.raises(NotImplementedError):
        _crit("dcgan")
    once = _crit("vanilla")(x.clone().requires_grad_(True), True)
    w = torch.ones((), device=dev, requires_grad=True)
    leaf = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(_crit("vanilla")(leaf, True) * w, leaf, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    assert once.dtype == torch.float32


def poison_cases():
    """The outputs the LDS-poison test compares bit for bit (test_gpu_gan_poison.py): every kind of both kernels, the
    single-workgroup form, the fold past one workgroup and past the grid cap, an offset view, the relativistic forms."""
    dev = torch.device("cuda")
    out = []
    for shape in ("16x1", "view67", "trip"):
        x = C.content("normal", C.shape_of(shape, _cap()))
        for config in (C.CONFIGS[2], C.CONFIGS[5], C.CONFIGS[8], C.CONFIGS[11], C.CONFIGS[13]):
            out += list(_plain(dev, x, config, offset=shape == "view67")[:2])
    x = C.content("normal", (5000,))                          # five workgroups: the fold below the cap
    out += list(_plain(dev, x, C.CONFIGS[0])[:2])
    for pair in ("sizes_differ", "trip"):
        real, fake = C.rel_inputs(pair, _cap())
        out += list(_relativistic(dev, _crit("vanilla", (0.9, 0.1)), "gen_both", real, fake)[:3])
        out += [t for t in _relativistic(dev, _crit("hinge"), "disc_fake", real, fake)[:3] if t is not None]
    return out
