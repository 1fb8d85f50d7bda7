"""The one-launch Adam / AdamW kernel (ssl_amd/csrc/ssg_multi.hip behind ssl_amd.optim) against tests/adam_reference.py's
float32 restatement of its contract: int32 bit patterns, no tolerance; at NaN positions both must be NaN.  Sets of many
tensors carved from buffers with guards between them, every alignment of p against g / m / v, the second grid trip,
special values, thirty chained steps, and the classes: launches per group, rebuilds, layouts, the fallbacks' bits, no
host synchronisation.  The step is NOT captured into a graph anywhere: its bias corrections are host scalars of step t."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import adam_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EADBEEF                                  # the guards' word (as a float: about 6.2e18)
MODES = ((0.0, False), (0.01, False), (0.01, True))    # weight decay: none, Adam's L2, AdamW's decoupled


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _chunk():
    from ssl_amd import _lib
    return _lib.lib().ssg_multi_chunk()


class Carved:
    """Tensors of `sizes` elements carved from one flat buffer, `gaps[i]` sentinel words in front of tensor i (and a run
    behind the last): values on the CPU (numpy), then the same layout on the device."""

    def __init__(self, sizes, gaps, values):
        self.sizes, self.starts, pos = list(sizes), [], 0
        for n, g in zip(sizes, gaps):
            pos += g
            self.starts.append(pos)
            pos += n
        self.total = pos + 7
        flat = np.full(self.total, SENTINEL, dtype=np.int32)
        self.index = np.concatenate([np.arange(s, s + n) for s, n in zip(self.starts, sizes)] + [np.zeros(0, np.int64)])
        flat[self.index] = np.asarray(values, dtype=np.float32).view(np.int32)
        self.cpu = flat.view(np.float32)

    def on(self, dev, shift=0):
        """The buffer on the device, its first word `shift` floats behind a 16-byte boundary."""
        buf = torch.empty(self.total + 4, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        flat = buf[shift:shift + self.total]
        flat.copy_(torch.from_numpy(self.cpu))
        return flat

    def pointers(self, flat):
        return [flat.data_ptr() + 4 * s for s in self.starts]


def _values(rng, n, kind):
    if kind == "g":
        return R.gradients(rng, n)
    if kind == "v":
        return (R.gradients(rng, n).astype(np.float64) ** 2).astype(np.float32)
    return (rng.standard_normal(n) * (0.05 if kind == "p" else 1e-3)).astype(np.float32)


def _launch(dev, bufs, sets, s):
    """One ssg_adam_apply on the carved sets (p, g, m, v) living in the device buffers `bufs`."""
    from ssl_amd import _lib, optim
    built = optim.build_tables(*(c.pointers(b) for c, b in zip(sets, bufs)), sets[0].sizes, dev)
    assert built is not None
    table, grads, n_chunks, _ = built
    sc = optim.Scalars(*(s[k] for k, _ in optim.Scalars._fields_))
    _lib.check(_lib.lib().ssg_adam_apply(table.data_ptr(), grads.data_ptr(), n_chunks, ctypes.addressof(sc),
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return n_chunks


def _check_sets(dev, sets, s, shifts=(0, 0, 0, 0), what=""):
    """One step on the carved sets: the whole p, m and v buffers, guards included, equal the restatement's on the CPU
    copies, and the g buffer is unchanged."""
    bufs = [c.on(dev, sh) for c, sh in zip(sets, shifts)]
    P, G, M, V = sets
    new = R.restate(P.cpu[P.index], G.cpu[G.index], M.cpu[M.index], V.cpu[V.index], s)
    _launch(dev, bufs, sets, s)
    for c, b, name, vals in ((P, bufs[0], "p", new[0]), (M, bufs[2], "m", new[1]), (V, bufs[3], "v", new[2])):
        want = c.cpu.copy()
        want[c.index] = vals
        got = b.cpu().numpy()
        guard = np.ones(c.total, dtype=bool)
        guard[c.index] = False
        assert np.array_equal(R.bits(got)[guard], R.bits(c.cpu)[guard]), (what, name, "a guard changed")
        assert R.same_bits(got, want), (what, name, int((R.bits(got) != R.bits(want)).sum()))
    assert np.array_equal(R.bits(bufs[1].cpu().numpy()), R.bits(G.cpu)), (what, "g changed")
    return new


def _scalars(wd=0.0, decoupled=False, step=3.0, lr=2e-4, betas=(0.9, 0.99), eps=1e-8):
    return R.host_scalars(lr, betas[0], betas[1], eps, wd, decoupled, float(step))


# ---- the kernel through the C ABI ----
@pytest.mark.parametrize("wd,decoupled", MODES)
def test_mixed_set_with_guards(dev, wd, decoupled):
    """1,510 tensors from 0 to 2 chunk + 7 elements, 1,500 of them in the bias regime, carved with 1- to 7-element gaps
    of a sentinel, different for p, g, m and v, so every residue mod 16 occurs in every combination."""
    c = _chunk()
    rng = np.random.default_rng(5)
    sizes = [1, 3, 4, 5, 1023, c - 1, c, c + 1, 2 * c + 7, 0] + rng.integers(1, 65, 1500).tolist()
    n = sum(sizes)
    sets = [Carved(sizes, rng.integers(1, 8, len(sizes)).tolist(), _values(rng, n, k)) for k in "pgmv"]
    residues = {tuple(s.starts[i] % 4 for s in sets) for i in range(len(sizes))}
    assert len(residues) > 200                                    # of the 256 combinations
    _check_sets(dev, sets, _scalars(wd, decoupled), what="mixed")


@pytest.mark.parametrize("shifts", [(a, b, b, b) for a in range(4) for b in range(4)] + [(0, 1, 2, 3)])
def test_alignment_of_p_against_g_m_v(dev, shifts):
    """Every tensor starts on a 16-byte boundary of its buffer; the buffers are views offset by 0, 4, 8 or 12 bytes: all
    4 x 4 residues of p against a shared residue of g, m and v, and one case where the three differ from each other."""
    c = _chunk()
    sizes = [1, 3, 4, 5, 7, 8, 1023, c - 1, c, c + 1, 2 * c + 7]
    gaps, pos = [], 0
    for n in sizes:
        g = 4 + (-pos) % 4
        gaps.append(g)
        pos += g + n
    rng = np.random.default_rng(13)
    sets = [Carved(sizes, gaps, _values(rng, sum(sizes), k)) for k in "pgmv"]
    assert all(s % 4 == 0 for s in sets[0].starts)
    _check_sets(dev, sets, _scalars(0.01, False), shifts=shifts, what=f"shifts {shifts}")


def test_second_grid_trip(dev):
    """One tensor of (grid cap + 1) chunk + 5 elements: the first two workgroups take a second chunk."""
    from ssl_amd import _lib
    L = _lib.lib()
    c, cap = L.ssg_multi_chunk(), L.ssg_multi_grid_cap()
    sizes = [(cap + 1) * c + 5]
    assert L.ssg_multi_chunks(1, np.ascontiguousarray(sizes, dtype=np.uintp).ctypes.data) == cap + 2
    rng = np.random.default_rng(17)
    sets = [Carved(sizes, [g], _values(rng, sizes[0], k)) for k, g in zip("pgmv", (1, 2, 3, 5))]
    _check_sets(dev, sets, _scalars(), what="second trip")


def test_special_values(dev):
    """g = 0, +-1e-30 (g^2 underflows), +-1e20 (v infinite, the update 0), +-inf, NaN; a subnormal v; eps dominating;
    lr = 0; weight decay of both forms; steps 1 and 10^6.  Nothing is special-cased, on either side."""
    inf, nan = float("inf"), float("nan")
    g = np.array([0.0, -0.0, 1e-30, -1e-30, 1e20, -1e20, inf, -inf, nan, 0.3, -7e-5], dtype=np.float32)
    v = np.array([0.0, 1e-40, 3e-45, 1e-12, 1.0, 3e38], dtype=np.float32)
    m = np.array([0.0, 0.1, -1e-30, 1e-42], dtype=np.float32)
    p = np.array([0.5, -2.0, 0.0, 1e-39], dtype=np.float32)
    G, V, M, P = (x.ravel() for x in np.meshgrid(g, v, m, p, indexing="ij"))
    with np.errstate(all="ignore"):
        assert np.float32(1e-30) ** 2 == 0 and np.isinf(np.float32(1e20) * np.float32(1e20)) and 0 < v[1] < 2.0 ** -126
    sizes = [len(G), 37, len(G)]
    rng = np.random.default_rng(19)
    pick = rng.integers(0, len(G), 37)
    cat = lambda x: np.concatenate([x, x[pick], x[::-1]])       # noqa: E731
    sets = [Carved(sizes, gaps, cat(x)) for x, gaps in ((P, (3, 1, 2)), (G, (3, 5, 2)), (M, (1, 1, 6)), (V, (2, 7, 3)))]
    seen_inf_v = seen_zero_update = False
    for wd, decoupled in MODES:
        for step in (1, 10 ** 6):
            for lr in (0.0, 1e-3):
                for eps in (1e-8, 1.0):                              # eps = 1 dominates every finite sqrt(v) here but one
                    s = _scalars(wd, decoupled, step, lr=lr, eps=eps, betas=(0.9, 0.999))
                    new = _check_sets(dev, sets, s, what=f"special wd={wd} decoupled={decoupled} t={step} lr={lr} eps={eps}")
                    big = np.abs(sets[1].cpu[sets[1].index]) == np.float32(1e20)
                    seen_inf_v |= bool(np.isinf(new[2][big]).all())
                    if lr and not wd:
                        seen_zero_update |= bool((new[0][big] == sets[0].cpu[sets[0].index][big]).all())
    assert seen_inf_v and seen_zero_update


def test_thirty_chained_steps(dev):
    """Thirty steps chained on the device, a new gradient each, against thirty chained steps of the restatement."""
    from ssl_amd import _lib, optim
    c = _chunk()
    sizes = [5, 64, 577, c + 9]
    rng = np.random.default_rng(23)
    n = sum(sizes)
    sets = [Carved(sizes, gaps, vals) for gaps, vals in (((1, 2, 3, 1), _values(rng, n, "p")), ((2, 2, 2, 2), np.zeros(n)),
                                                         ((3, 1, 4, 1), np.zeros(n)), ((4, 4, 1, 3), np.zeros(n)))]
    bufs = [s.on(dev) for s in sets]
    table, grads, n_chunks, _ = optim.build_tables(*(s.pointers(b) for s, b in zip(sets, bufs)), sizes, dev)
    P, G, M, V = sets
    state = (P.cpu[P.index], M.cpu[M.index], V.cpu[V.index])
    stream = torch.cuda.current_stream().cuda_stream
    gcpu = G.cpu.copy()
    for t in range(1, 31):
        g = R.gradients(rng, n)
        gcpu[G.index] = g
        bufs[1].copy_(torch.from_numpy(gcpu))
        s = R.host_scalars(2e-4, 0.9, 0.99, 1e-8, 0.01 if t % 2 else 0.0, False, float(t))
        sc = optim.Scalars(*(s[k] for k, _ in optim.Scalars._fields_))
        _lib.check(_lib.lib().ssg_adam_apply(table.data_ptr(), grads.data_ptr(), n_chunks, ctypes.addressof(sc), stream))
        state = R.restate(state[0], g, state[1], state[2], s)
    torch.cuda.synchronize()
    for c_, b, want in ((P, bufs[0], state[0]), (M, bufs[2], state[1]), (V, bufs[3], state[2])):
        assert R.same_bits(b.cpu().numpy()[c_.index], want)
    assert not R.same_bits(state[0], P.cpu[P.index])


# ---- the classes ----
def _conv_net(dev, dtype=torch.float32, fmt=torch.contiguous_format, seed=29):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Conv2d(3, 6, 3), nn.PReLU(), nn.Conv2d(6, 5, 3, bias=False), nn.Conv2d(5, 3, 1))
    return net.to(dev, dtype).to(memory_format=fmt)


def _backward(nets, gen, dev, fresh=True):
    """The same new gradients on every net, as a training iteration leaves them: zero_grad(set_to_none) then new tensors."""
    for ps in zip(*(n.parameters() for n in nets)):
        g = torch.randn(ps[0].shape, generator=gen).to(dev, ps[0].dtype)
        for p in ps:
            if fresh or p.grad is None:
                p.grad = torch.empty_like(p).copy_(g)
            else:
                p.grad.copy_(g)


def _strided_numpy(t):
    """The tensor's memory in storage order (the step walks the storage: channels_last included)."""
    t = t.detach()
    order = sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))
    return t.permute(order).contiguous().cpu().numpy().ravel()


def _restated_twin(net, opt):
    return {k: (_strided_numpy(p), np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32))
            for k, p in net.named_parameters()}


@pytest.mark.parametrize("name,wd,fmt", [("Adam", 0.0, torch.contiguous_format), ("Adam", 0.01, torch.contiguous_format),
                                         ("AdamW", 0.01, torch.channels_last)])
def test_classes_equal_the_restatement_and_torch_meets_the_bound(dev, name, wd, fmt):
    """Four steps of the class on a small network: p, exp_avg and exp_avg_sq equal the chained restatement bit for bit (a
    channels_last network is native: the group is one launch over the storage).  Beside it torch's own GPU Adam from the
    same state each step: its share of the fp64 bound is printed (an observation)."""
    from ssl_amd import optim
    net, ref_net = _conv_net(dev, fmt=fmt), _conv_net(dev, fmt=fmt)
    if fmt == torch.channels_last:
        assert not net[0].weight.is_contiguous()
    opt = getattr(optim, name)(net.parameters(), 2e-4, betas=(0.9, 0.99), weight_decay=wd)
    ref = getattr(torch.optim, name)(ref_net.parameters(), 2e-4, betas=(0.9, 0.99), weight_decay=wd)
    twin = _restated_twin(net, opt)
    gen = torch.Generator().manual_seed(31)
    worst = [0.0, 0.0, 0.0]
    for t in range(1, 5):
        _backward((net, ref_net), gen, dev)
        for (k, p), q in zip(net.named_parameters(), ref_net.parameters()):   # torch's GPU step from OUR state
            q.data.copy_(p.data)
            if t > 1:
                ref.state[q]["exp_avg"].copy_(opt.state[p]["exp_avg"])
                ref.state[q]["exp_avg_sq"].copy_(opt.state[p]["exp_avg_sq"])
        opt.step()
        ref.step()
        s = R.host_scalars(2e-4, 0.9, 0.99, 1e-8, wd, name == "AdamW", float(t))
        for (k, p), q in zip(net.named_parameters(), ref_net.parameters()):
            before = twin[k]
            g = _strided_numpy(p.grad)
            twin[k] = R.restate(before[0], g, before[1], before[2], s)
            want, bound = R.exact_and_bound(before[0], g, before[1], before[2], s, sqrt_ulps=1.0)
            theirs = (q, ref.state[q]["exp_avg"], ref.state[q]["exp_avg_sq"])
            for i in range(3):
                worst[i] = max(worst[i], R.share(_strided_numpy(theirs[i]), want[i], bound[i]))
    torch.cuda.synchronize()
    print(f"{name} wd={wd}: torch's GPU result, largest share of the bound used: p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    for k, p in net.named_parameters():
        st = opt.state[p]
        assert R.same_bits(_strided_numpy(p), twin[k][0]), k
        assert R.same_bits(_strided_numpy(st["exp_avg"]), twin[k][1]) and R.same_bits(_strided_numpy(st["exp_avg_sq"]), twin[k][2]), k
        assert float(st["step"]) == 4.0 and not st["step"].is_cuda
    plan = opt._plans[(0, 0)]
    assert plan.native and plan.rebuilds == 1 and len(opt._plans) == 1


class _Counting:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def ssg_adam_apply(self, *args):
        self.calls.append(args[2])
        return self.real.ssg_adam_apply(*args)


def _module(n_tensors, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    m = nn.Module()
    for i in range(n_tensors):
        shape = (1 + i % 64,) if i % 3 else (2, 1 + i % 7, 3)
        m.register_parameter(f"p{i}", nn.Parameter(torch.randn(shape, generator=gen).to(dev)))
    return m


def test_one_apply_per_group_rebuilds_and_equal_bits_from_equal_state(dev, monkeypatch):
    from ssl_amd import optim
    lib = _Counting(optim._lib.lib())
    monkeypatch.setattr(optim, "_library", lambda: lib)
    results = []
    for _ in range(2):
        net = _module(300, 37, dev)
        params = list(net.parameters())
        opt = optim.Adam([dict(params=params[:100]), dict(params=params[100:], lr=1e-4)], 2e-4, betas=(0.9, 0.99))
        gen = torch.Generator().manual_seed(41)
        lib.calls.clear()
        _backward((net,), gen, dev)
        opt.step()
        assert len(lib.calls) == 2                                 # one apply per group, 100 and 200 tensors
        _backward((net,), gen, dev, fresh=False)                   # the same gradient tensors: nothing is uploaded
        opt.step()
        plans = [opt._plans[(0, 0)], opt._plans[(1, 0)]]
        assert len(lib.calls) == 4 and [(p.rebuilds, p.grad_uploads) for p in plans] == [(1, 0), (1, 0)]
        held = [p.grad for p in params]                            # (alive, so that every new gradient lies elsewhere)
        opt.zero_grad(set_to_none=True)
        _backward((net,), gen, dev)                                # the gradients moved: the address array alone
        assert all(p.grad.data_ptr() != h.data_ptr() for p, h in zip(params, held))
        opt.step()
        assert len(lib.calls) == 6 and [(p.rebuilds, p.grad_uploads) for p in plans] == [(1, 1), (1, 1)]
        p0 = params[3]
        old = p0.data_ptr()
        p0.data = p0.data.clone()                                  # new storage: the table is rebuilt, the old one kept till then
        assert p0.data_ptr() != old and old in [t.data_ptr() for t in plans[0].keep[0]]
        _backward((net,), gen, dev, fresh=False)
        opt.step()
        assert len(lib.calls) == 8 and [p.rebuilds for p in plans] == [2, 1]
        assert old not in [t.data_ptr() for t in plans[0].keep[0]]
        torch.cuda.synchronize()
        del held
        results.append(torch.cat([p.detach().flatten().view(torch.int32) for p in params]
                                 + [opt.state[p][k].flatten().view(torch.int32) for p in params for k in ("exp_avg", "exp_avg_sq")]))
    assert torch.equal(results[0], results[1])


def _run_pair(dev, make_ours, make_theirs, dtype=torch.float32, steps=3):
    a, b = _conv_net(dev, dtype), _conv_net(dev, dtype)
    ours, theirs = make_ours(a.parameters()), make_theirs(b.parameters())
    gen = torch.Generator().manual_seed(43)
    for _ in range(steps):
        _backward((a, b), gen, dev)
        ours.step()
        theirs.step()
    torch.cuda.synchronize()
    same = all(torch.equal(p.detach().view(torch.uint8), q.detach().view(torch.uint8)) for p, q in zip(a.parameters(), b.parameters()))
    return ours, same


@pytest.mark.parametrize("case", ["fp64", "half", "amsgrad", "maximize", "tensor_lr", "switch_off"])
def test_outside_the_native_domain_gives_torchs_own_gpu_bits(dev, case):
    from ssl_amd import optim
    from ssl_amd.losses import set_native_criteria
    kwargs, dtype = dict(betas=(0.9, 0.99)), torch.float32
    if case == "fp64":
        dtype = torch.float64
    elif case == "half":
        dtype = torch.float16
    elif case == "amsgrad":
        kwargs["amsgrad"] = True
    elif case == "maximize":
        kwargs["maximize"] = True
    lr = (lambda: torch.tensor(2e-4)) if case == "tensor_lr" else (lambda: 2e-4)
    if case == "tensor_lr":
        kwargs["foreach"] = False
    prev = set_native_criteria(False) if case == "switch_off" else None
    try:
        ours, same = _run_pair(dev, lambda ps: optim.Adam(ps, lr(), **kwargs), lambda ps: torch.optim.Adam(ps, lr(), **kwargs), dtype)
    finally:
        if prev is not None:
            set_native_criteria(prev)
    assert same
    plans = ours.__dict__.get("_plans", {})
    assert all(not p.native for p in plans.values())               # no table was built for any of them
    if case == "switch_off":                                       # the switch is seen by the next call
        net = _conv_net(dev)
        opt = optim.Adam(net.parameters(), 2e-4)
        _backward((net,), torch.Generator().manual_seed(1), dev)
        opt.step()
        assert opt._plans[(0, 0)].native


def test_step_makes_no_host_synchronisation(dev):
    from ssl_amd import optim
    net = _conv_net(dev)
    opt = optim.Adam(net.parameters(), 2e-4, betas=(0.9, 0.99))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.5)
    gen = torch.Generator().manual_seed(47)
    _backward((net,), gen, dev)
    opt.step()                                                     # builds and uploads the tables
    torch.cuda.synchronize()
    assert hasattr(torch.cuda, "set_sync_debug_mode")
    for fresh in (False, True, True):                              # a plain step, then steps after the gradients moved
        held = [p.grad for p in net.parameters()]                  # (alive, so that a new gradient lies elsewhere)
        if fresh:
            opt.zero_grad(set_to_none=True)
        _backward((net,), gen, dev, fresh=fresh)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
            sched.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    plan = opt._plans[(0, 0)]
    assert plan.native and plan.rebuilds == 1 and plan.grad_uploads == 2 and len(held) == 6
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())


def test_state_dict_crosses_between_the_classes_on_the_gpu(dev):
    """A checkpoint of torch.optim.Adam loads into ssl_amd.optim.Adam and the other way round; each goes on natively or
    as torch does, within a rounding of the other."""
    from ssl_amd import optim
    a, b = _conv_net(dev), _conv_net(dev)
    ours, theirs = optim.Adam(a.parameters(), 2e-4), torch.optim.Adam(b.parameters(), 2e-4)
    gen = torch.Generator().manual_seed(53)
    for _ in range(2):
        _backward((a, b), gen, dev)
        ours.step()
        theirs.step()
    c, d = copy.deepcopy(b), copy.deepcopy(a)
    into_ours, into_theirs = optim.Adam(c.parameters(), 2e-4), torch.optim.Adam(d.parameters(), 2e-4)
    into_ours.load_state_dict(copy.deepcopy(theirs.state_dict()))
    into_theirs.load_state_dict(copy.deepcopy(ours.state_dict()))
    _backward((a, b, c, d), gen, dev)
    for o in (ours, theirs, into_ours, into_theirs):
        o.step()
    torch.cuda.synchronize()
    assert into_ours._plans[(0, 0)].native
    for p, q, r, s in zip(a.parameters(), b.parameters(), c.parameters(), d.parameters()):
        assert float(into_ours.state[r]["step"]) == float(into_theirs.state[s]["step"]) == 3.0
        assert torch.allclose(p, s, rtol=1e-5, atol=1e-7) and torch.allclose(q, r, rtol=1e-5, atol=1e-7)
