"""The spectral-normalisation kernels (ssl_amd/csrc/ssg_specnorm.hip behind ssl_amd.spectral) against the fp64
restatement and its derived bounds (tests/specnorm_reference.py) on the cases of tests/specnorm_cases.py: v, u, sigma32,
W_sn and dW of every layer; carved buffers with guards at every 4-byte offset of W, u, v, the output and G; bit-for-bit
repeat calls, a layer alone against among others, eval mode, a HIP-graph replay, the second grid trip; the fused module
under autograd with two forwards before one backward, the rebuild after new storage, the fallback of a half-precision
layer, and UNetDiscriminatorSN end to end against fp64."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn.utils import spectral_norm

import specnorm_cases as C
import specnorm_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EADBEEF


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _carve(dev, arrays, shift):
    """The arrays in one flat device buffer, each on a 16-byte boundary plus `shift` floats, sentinel words between and
    around them: (the flat buffer, the views, the guard mask)."""
    starts, pos = [], 4
    for a in arrays:
        starts.append(pos)
        pos += a.size + 4 + (-a.size) % 4
    host = np.full(pos, SENTINEL, dtype=np.uint32)
    guard = np.ones(pos, dtype=bool)
    for s, a in zip(starts, arrays):
        host[s:s + a.size] = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)
        guard[s:s + a.size] = False
    buf = torch.empty(pos + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    flat = buf[shift:shift + pos]
    flat.copy_(torch.from_numpy(host.view(np.float32)))
    return flat, [flat[s:s + a.size].view(a.shape) for s, a in zip(starts, arrays)], guard


def _guards_intact(flat, guard):
    words = flat.cpu().numpy().view(np.uint32)
    return bool((words[guard] == SENTINEL).all())


class Run:
    """One layer set on the device (carved, with the given shifts), its plan, and the calls on blocks of this test's
    own, filled with the sentinel first."""

    def __init__(self, dev, layers, shifts=(0, 0, 0, 0, 0)):
        from ssl_amd import spectral
        self.dev, self.layers, self.shifts = dev, layers, shifts
        self.Wf, self.W, self.Wg = _carve(dev, [l[0] for l in layers], shifts[0])
        self.uf, self.u, self.ug = _carve(dev, [l[1] for l in layers], shifts[1])
        self.vf, self.v, self.vg = _carve(dev, [l[2] for l in layers], shifts[2])
        self.W0 = self.Wf.cpu()
        self.plan = spectral.Plan(list(zip(self.W, self.u, self.v)), dev)

    def _block(self, shift):
        n = self.plan.out_bytes // 4
        buf = torch.empty(n + 12, dtype=torch.float32, device=self.dev)
        buf.view(torch.int32).fill_(np.int32(np.uint32(SENTINEL)).item())
        return buf, buf[4 + shift:4 + shift + n]

    def _block_guards(self, buf, shift):
        words = buf.cpu().numpy().view(np.uint32)
        mask = np.ones(len(words), dtype=bool)
        for o, r, c in zip(self.plan.out_off, self.plan.rows, self.plan.cols):
            mask[4 + shift + o:4 + shift + o + r * c] = False
        return bool((words[mask] == SENTINEL).all())

    def forward(self, training=True):
        buf, block = self._block(self.shifts[3])
        outs, saved = self.plan.forward(training, out=block)
        torch.cuda.synchronize()
        assert self._block_guards(buf, self.shifts[3]), "the output block's guards changed"
        assert _guards_intact(self.uf, self.ug) and _guards_intact(self.vf, self.vg), "a guard of u or v changed"
        assert torch.equal(self.Wf.cpu().view(torch.int32), self.W0.view(torch.int32)), "W changed"
        return [o.cpu().numpy() for o in outs], saved

    def saved_parts(self, saved):
        s = saved.cpu().numpy()
        return [(s[o:o + r], s[o + r:o + r + c], s[o + r + c]) for o, r, c in
                zip(self.plan.saved_off, self.plan.rows, self.plan.cols)]

    def backward(self, saved, grads):
        gf, gviews, gg = _carve(self.dev, [g for g in grads if g is not None], self.shifts[4])
        it = iter(gviews)
        gs = [None if g is None else next(it) for g in grads]
        buf, block = self._block(self.shifts[3])
        dW = self.plan.backward(saved, gs, block=block)
        torch.cuda.synchronize()
        assert self._block_guards(buf, self.shifts[3]), "the gradient block's guards changed"
        assert _guards_intact(gf, gg)
        return [None if d is None else d.cpu().numpy() for d in dW]


def _hold(name, run, training, outs, saved, grads=None, dWs=None, shares=None):
    """Every output of one call against the restatement, layer by layer, from the layers' values BEFORE the call."""
    parts = run.saved_parts(saved)
    for i, ((W, u0, v0), out, (su, sv, ssig)) in enumerate(zip(run.layers, outs, parts)):
        f = R.forward(W, u0, v0, training)
        G = None if grads is None else grads[i]
        b = None if G is None else R.backward(W, f, G)
        bd = R.bounds(W, u0, f, training, G, b)
        tag = f"{name}[{i}] {W.shape}"
        got = dict(v=sv, u=su, sigma32=np.float32(ssig).reshape(1), out=out)
        want = dict(v=f["v"], u=f["u"], sigma32=np.float32(f["sigma32"]).reshape(1), out=f["out"])
        bound = dict(v=bd["dv"], u=bd["du"], sigma32=bd["dsig32"], out=bd["dout"])
        if G is not None:
            got["dW"], want["dW"], bound["dW"] = dWs[i], b["dW"], bd["ddW"]
        for k in got:
            share = R.check(f"{tag} {k}", got[k], want[k], bound[k])
            if shares is not None:
                shares[k] = max(shares.get(k, 0.0), share)
        if training:      # in place: the buffers hold what the saved block holds
            assert np.array_equal(R.bits(run.u[i].cpu().numpy()), R.bits(su)), tag
            assert np.array_equal(R.bits(run.v[i].cpu().numpy()), R.bits(sv)), tag
        else:
            assert np.array_equal(R.bits(su), R.bits(u0)) and np.array_equal(R.bits(sv), R.bits(v0)), tag
            assert np.array_equal(R.bits(run.u[i].cpu().numpy()), R.bits(u0)), tag
            assert np.array_equal(R.bits(run.v[i].cpu().numpy()), R.bits(v0)), tag


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_cases_against_the_restatement(dev, name):
    """Training forward and backward, then an eval forward on the updated vectors (which must leave them alone)."""
    shapes, content, nan_layer = C.CASES[name]
    layers = C.layer_set(shapes, content, seed=3, nan_layer=nan_layer)
    grads = C.gradients(shapes)
    run = Run(dev, layers)
    shares = {}
    outs, saved = run.forward(True)
    dWs = run.backward(saved, grads)
    _hold(name, run, True, outs, saved, grads, dWs, shares)
    if content == "zero":
        assert all(np.isnan(o).all() for o in outs) and all((p[0] == 0).all() and (p[1] == 0).all()
                                                            for p in run.saved_parts(saved))
    if nan_layer is not None:
        for i, o in enumerate(outs):
            assert np.isnan(o).all() == (i == nan_layer) and np.isnan(o).any() == (i == nan_layer), i
    after = [(W, u.cpu().numpy(), v.cpu().numpy()) for (W, _, _), u, v in zip(layers, run.u, run.v)]
    run.layers = after
    outs2, saved2 = run.forward(False)
    dW2 = run.backward(saved2, grads)
    _hold(name + " eval", run, False, outs2, saved2, grads, dW2, shares)
    print(name, "largest shares of the bounds:", {k: f"{v:.2e}" for k, v in shares.items()})


def test_rank_one_layer_finds_its_singular_pair(dev):
    """W = 3 a b^T: one power iteration from any u lands on (a, b) up to sign, sigma = 3, W_sn = a b^T."""
    layers = C.layer_set([(33, 65)], "rank1", seed=5)
    run = Run(dev, layers)
    outs, saved = run.forward(True)
    (u, v, sig), W = run.saved_parts(saved)[0], layers[0][0].astype(np.float64)
    assert abs(float(sig) - 3.0) < 1e-5
    assert np.abs(np.outer(u, v) * 3.0 - W).max() < 1e-5 and np.abs(outs[0] - W / 3.0).max() < 1e-6


@pytest.mark.parametrize("role,shift", [(r, s) for r in range(5) for s in (1, 2, 3)])
def test_every_offset_of_every_tensor_gives_the_aligned_bits(dev, role, shift):
    """W, u, v, the output block or G moved by 4, 8 or 12 bytes: the guards stay and every output is the aligned run's,
    bit for bit (sums are ordered by index, not by address)."""
    shapes = C.SMALLEST + C.EDGES + C.MIXED_8[:3]
    layers, grads = C.layer_set(shapes, seed=7), C.gradients(shapes)
    results = []
    for shifts in ((0, 0, 0, 0, 0), tuple(shift if k == role else 0 for k in range(5))):
        run = Run(dev, layers, shifts)
        outs, saved = run.forward(True)
        dWs = run.backward(saved, grads)
        results.append(outs + dWs + [saved.cpu().numpy()])
    for a, b in zip(*results):
        assert np.array_equal(R.bits(a), R.bits(b))


def test_repeat_alone_and_among_others_give_the_same_bits(dev):
    shapes = C.MIXED_17
    layers, grads = C.layer_set(shapes, seed=9), C.gradients(shapes)

    def once(idx):
        run = Run(dev, [layers[i] for i in idx])
        outs, saved = run.forward(True)
        dWs = run.backward(saved, [grads[i] for i in idx])
        return [(o, d, p) for o, d, p in zip(outs, dWs, run.saved_parts(saved))]

    a, b = once(range(17)), once(range(17))
    for i in (0, 5, 11, 16):
        alone = once([i])[0]
        for x, y, z in zip(a[i][:2] + a[i][2], b[i][:2] + b[i][2], alone[:2] + alone[2]):
            assert np.array_equal(R.bits(x), R.bits(y)) and np.array_equal(R.bits(x), R.bits(z)), i


def test_a_layer_without_a_gradient_is_skipped(dev):
    shapes = C.MIXED_8[:4]
    layers, grads = C.layer_set(shapes, seed=11), C.gradients(shapes)
    run = Run(dev, layers)
    outs, saved = run.forward(True)
    full = run.backward(saved, grads)
    part = run.backward(saved, [grads[0], None, grads[2], None])
    assert part[1] is None and part[3] is None
    assert np.array_equal(R.bits(part[0]), R.bits(full[0])) and np.array_equal(R.bits(part[2]), R.bits(full[2]))


def test_second_grid_trip_gives_the_product_builds_bits(dev):
    """The profiling build with the grid cap lowered to 2 (the chunk size kept): every workgroup of every launch walks
    several units, and every output equals the product build's bit for bit."""
    from ssl_amd import _lib
    shapes = C.TALL + C.MIXED_8
    layers, grads = C.layer_set(shapes, seed=13), C.gradients(shapes)

    def once():
        run = Run(dev, layers)
        outs, saved = run.forward(True)
        return outs + run.backward(saved, grads) + [saved.cpu().numpy()]

    want = once()
    with _lib.profile_build() as P:
        tune = P.ssg_prof_sn_tuning
        tune.restype, tune.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
        chunk, cap = P.ssg_sn_chunk(), P.ssg_sn_grid_cap()
        assert tune(chunk, 2) == 0 and P.ssg_sn_grid_cap() == 2
        try:
            got = once()
        finally:
            torch.cuda.synchronize()
            tune(chunk, cap)
    for a, b in zip(got, want):
        assert np.array_equal(R.bits(a), R.bits(b))


# ---- the fused module ----
def _net(dev, dtype=torch.float32, seed=0, widths=(3, 6, 12, 6)):
    torch.manual_seed(seed)
    convs = [spectral_norm(nn.Conv2d(a, b, 3, 1, 1, bias=False)) for a, b in zip(widths[:-1], widths[1:])]
    return nn.Sequential(*convs).to(dev, dtype)


def _state(net):
    """[(W, u, v)] numpy of the net's normalised layers."""
    return [tuple(getattr(m, k).detach().cpu().numpy().copy() for k in ("weight_orig", "weight_u", "weight_v"))
            for m in net if hasattr(m, "weight_orig")]


def test_two_forwards_then_one_backward_see_their_own_vectors(dev):
    """L = sum_l <W_sn,l (first forward), C_l> + <W_sn,l (second forward), D_l>, one backward: the gradient is the sum of
    both calls' restated gradients, each from ITS call's u, v, sigma (u moves between the forwards)."""
    from ssl_amd import spectral
    net = _net(dev)
    handle = spectral.fuse_spectral_norm(net)
    x = torch.zeros(1, 3, 4, 4, device=dev)
    gen = torch.Generator().manual_seed(3)
    Cs = [[torch.randn(m.weight_orig.shape, generator=gen) for m in net] for _ in range(2)]
    states, loss = [], 0.0
    for k in range(2):
        states.append(_state(net))
        net(x)
        loss = loss + sum((m.weight * c.to(dev)).sum() for m, c in zip(net, Cs[k]))
    loss.backward()
    torch.cuda.synchronize()
    assert handle.rebuilds == 1
    for i, m in enumerate(net):
        want, bound = 0.0, 0.0
        for k in range(2):
            W, u0, v0 = states[k][i]
            f = R.forward(W, u0, v0, True)
            b = R.backward(W, f, Cs[k][i].numpy())
            want = want + b["dW"].astype(np.float64)
            bound = bound + R.bounds(W, u0, f, True, Cs[k][i].numpy(), b)["ddW"]
        bound = bound + 2 * R.E32 * np.abs(want)              # the fp32 accumulation of the two gradients
        R.check(f"layer {i}", m.weight_orig.grad.cpu().numpy(), want.astype(np.float32), bound)
        assert not np.array_equal(states[0][i][1], states[1][i][1])
    handle.unfuse()


def test_vectors_move_without_grad_and_rest_in_eval(dev):
    from ssl_amd import spectral
    net = _net(dev)
    spectral.fuse_spectral_norm(net)
    x = torch.zeros(1, 3, 4, 4, device=dev)
    before = _state(net)
    with torch.no_grad():
        net(x)
    mid = _state(net)
    assert all(not np.array_equal(a[1], b[1]) for a, b in zip(before, mid))
    for p in net.parameters():
        p.requires_grad_(False)
    net(x)
    after = _state(net)
    assert all(not np.array_equal(a[1], b[1]) for a, b in zip(mid, after))
    net.eval()
    net(x)
    net(x)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(after, _state(net)) for k in (1, 2))
    for (W, u, v), m in zip(after, net):
        f = R.forward(W, u, v, False)
        R.check("eval", m.weight.cpu().numpy(), f["out"], R.bounds(W, u, f, False)["dout"])


def test_rebuild_after_new_storage(dev):
    from ssl_amd import spectral
    net = _net(dev)
    handle = spectral.fuse_spectral_norm(net)
    x = torch.zeros(1, 3, 4, 4, device=dev)
    net(x)
    net(x)
    assert handle.rebuilds == 1
    p = net[1].weight_orig
    p.data = p.data.clone().mul_(3.0)
    state = _state(net)
    net(x)
    torch.cuda.synchronize()
    assert handle.rebuilds == 2
    W, u, v = state[1]
    f = R.forward(W, u, v, True)
    R.check("rebuilt", net[1].weight.detach().cpu().numpy(), f["out"], R.bounds(W, u, f, True)["dout"])


def test_half_layer_inside_a_fused_set_takes_torchs_hook(dev):
    """The middle layer in half precision: the set's call takes the two fp32 layers, the half layer's own hook runs
    torch's lines and gives torch's bits; with set_native_criteria(False) every layer does."""
    from ssl_amd import spectral
    from ssl_amd.losses import set_native_criteria
    net, twin = _net(dev, seed=5), _net(dev, seed=5)
    net[1].half(), twin[1].half()
    handle = spectral.fuse_spectral_norm(net)
    handle.refresh()                  # (what the net's forward does first; the net itself cannot run on mixed dtypes)
    for a, b in zip(net, twin):
        inp = torch.ones(1, a.in_channels, 4, 4, device=dev, dtype=a.weight_orig.dtype)
        a(inp), b(inp)
    handle.release()
    assert len(handle._plans) == 1 and handle._plans[0][0] == [0, 2]
    assert torch.equal(net[1].weight, twin[1].weight) and torch.equal(net[1].weight_u, twin[1].weight_u)
    for i in (0, 2):
        assert torch.allclose(net[i].weight, twin[i].weight, rtol=1e-4, atol=1e-6)
    prev = set_native_criteria(False)
    try:
        fused_off, torchs = _net(dev, seed=7), _net(dev, seed=7)
        off = spectral.fuse_spectral_norm(fused_off)
        y = torch.ones(1, 3, 4, 4, device=dev)
        assert torch.equal(fused_off(y), torchs(y)) and off._plans == []
        assert all(torch.equal(a.weight, b.weight) and torch.equal(a.weight_u, b.weight_u)
                   for a, b in zip(fused_off, torchs))
    finally:
        set_native_criteria(prev)


def test_forward_replays_as_hip_graph(dev):
    """A captured training forward: three replays equal three eager forwards bit for bit, u and v included."""
    from ssl_amd import spectral
    eager, rec = _net(dev, seed=9), _net(dev, seed=9)
    he, hr = spectral.fuse_spectral_norm(eager), spectral.fuse_spectral_norm(rec)
    start = [t.clone() for t in rec.buffers()]
    with torch.no_grad():
        hr.refresh()                                       # builds the table outside the capture
        torch.cuda.synchronize()
        for t, s in zip(rec.buffers(), start):
            t.copy_(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            hr.refresh()                                   # (the set's call alone: no convolution enters the capture)
        weights = [m.weight for m in rec]                  # the capture's output views
        for t, s in zip(rec.buffers(), start):
            t.copy_(s)
        for _ in range(3):
            he.refresh()
            graph.replay()
            torch.cuda.synchronize()
            for a, w, b in zip(eager, weights, rec):
                assert torch.equal(a.weight.view(torch.int32), w.view(torch.int32))
                assert torch.equal(a.weight_u.view(torch.int32), b.weight_u.view(torch.int32))
                assert torch.equal(a.weight_v.view(torch.int32), b.weight_v.view(torch.int32))


def test_unet_discriminator_end_to_end_against_fp64(dev):
    """UNetDiscriminatorSN at 2 x 3 x 32 x 32, fused on the GPU, against the same module in fp64 on the CPU; the
    yardstick is the error of torch's own unfused fp32 module (on the CPU) against that fp64 run: at most 4 x it."""
    from ssl_amd import archs
    torch.manual_seed(21)
    ref32 = archs.UNetDiscriminatorSN(3, 16, fused=False)
    ref64 = archs.UNetDiscriminatorSN(3, 16, fused=False).double()
    ref64.load_state_dict(ref32.state_dict())
    fused = archs.UNetDiscriminatorSN(3, 16).to(dev)
    fused.load_state_dict(ref32.state_dict())
    x = torch.randn(2, 3, 32, 32)
    want = ref64(x.double())
    want.sum().backward()
    y32 = ref32(x)
    y32.sum().backward()
    got = fused(x.to(dev))
    got.sum().backward()
    assert fused.spectral.rebuilds == 1 and len(fused.spectral._plans) == 1

    def err(a, b):
        return float((a.detach().double().cpu() - b.detach()).abs().max())

    yard, mine = err(y32, want), err(got, want)
    print(f"output: torch fp32 against fp64 {yard:.3e}, fused against fp64 {mine:.3e}")
    assert mine <= 4 * yard
    for (k, p), q, r in zip(ref64.named_parameters(), ref32.parameters(), fused.parameters()):
        yard, mine = err(q.grad, p.grad), err(r.grad, p.grad)
        print(f"grad {k}: torch fp32 against fp64 {yard:.3e}, fused against fp64 {mine:.3e}")
        assert mine <= 4 * yard, k
