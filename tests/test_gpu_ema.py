"""The multi-tensor EMA / copy kernel (ssl_amd/csrc/ssg_multi.hip behind ssl_amd.ema) against tests/ema_reference.py,
torch's own expressions on the CPU copies of the same tensors: int32 bit patterns, no tolerance; at NaN positions both
must be NaN.  Sets of many tensors with every alignment, guards between the tensors, the second grid trip, special
values, layouts, the rebuild after new storage, LitEma on the fixture's model, and the replay as a HIP graph."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import ema_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f34_ema.npz")
SENTINEL = 0x5EADBEEF                                  # the guards' word (as a float: about 6.2e18)
DECAYS = (0.0, 0.5, 0.999, 0.9999, 1.0)
KINDS = (R.EMA, R.LIT, R.COPY)


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
    """Tensors of `sizes` elements carved from one flat buffer, `gaps[i]` sentinel words in front of tensor i (and one
    run behind the last): values on the CPU, then the same layout on the device."""

    def __init__(self, sizes, gaps, values):
        self.sizes, self.starts, pos = list(sizes), [], 0
        for n, g in zip(sizes, gaps):
            pos += g
            self.starts.append(pos)
            pos += n
        self.total = pos + 7
        flat = torch.full((self.total,), SENTINEL, dtype=torch.int32)
        self.guard = torch.ones(self.total, dtype=torch.bool)
        for s, n, v in zip(self.starts, sizes, values):
            flat[s:s + n] = v.contiguous().view(torch.int32)
            self.guard[s:s + n] = False
        self.cpu = flat.view(torch.float32)

    def views(self, flat):
        return [flat[s:s + n] for s, n in zip(self.starts, self.sizes)]

    def on(self, dev, shift=0):
        """The buffer on the device, its first word `shift` floats behind a 16-byte boundary."""
        buf = torch.empty(self.total + 4, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        flat = buf[shift:shift + self.total]
        flat.copy_(self.cpu)
        return flat


def _random_values(sizes, gen):
    return [torch.randn(n, generator=gen) for n in sizes]


def _apply_native(dev, kind, e_views, p_views, decay, w_dev):
    from ssl_amd import _lib, ema
    table, n_chunks, _ = ema.build_table([t.data_ptr() for t in e_views], [t.data_ptr() for t in p_views],
                                         [t.numel() for t in e_views], dev)
    d, a = (float(decay), 1 - float(decay)) if kind == R.EMA else (0.0, 0.0)
    _lib.check(_lib.lib().ssg_multi_apply(table.data_ptr(), n_chunks, kind, d, a,
                                          None if w_dev is None else w_dev.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return n_chunks


def _weight(decay):
    """LitEma's one_minus_decay for a decay buffer: a 0-d fp32 tensor."""
    return 1.0 - torch.tensor(decay, dtype=torch.float32)


def _check_set(dev, E, P, kinds=KINDS, decays=DECAYS, shift_e=0, shift_p=0, what=""):
    """Every kind and decay on the carved sets E (dst) and P (src), each from the same start: the whole dst buffer, guards
    included, equals the reference's on the CPU copy, and src is unchanged."""
    e_dev, p_dev = E.on(dev, shift_e), P.on(dev, shift_p)
    for kind in kinds:
        for decay in (decays if kind != R.COPY else decays[:1]):
            e_dev.copy_(E.cpu)
            want = E.cpu.clone()
            w = _weight(decay)
            for e, p in zip(E.views(want), P.views(P.cpu)):
                R.apply(kind, e, p, decay=decay, w=w)
            _apply_native(dev, kind, E.views(e_dev), P.views(p_dev), decay, w.to(dev).reshape(1))
            got = e_dev.cpu()
            assert torch.equal(R.bits(got)[E.guard], R.bits(E.cpu)[E.guard]), (what, kind, decay, "a guard changed")
            assert R.same_bits(got, want), (what, kind, decay)
            assert torch.equal(R.bits(p_dev.cpu()), R.bits(P.cpu)), (what, kind, decay, "src changed")


def _mixed_sizes():
    c = _chunk()
    gen = torch.Generator().manual_seed(5)
    return [1, 3, 4, 5, 1023, c - 1, c, c + 1, 2 * c + 5, 0] + torch.randint(1, 65, (1500,), generator=gen).tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_set_with_guards(dev, kind):
    """1,510 tensors from 0 to 2 chunk + 5 elements, 1,500 of them in the bias regime, carved with 1- to 7-element gaps
    of a sentinel (so every residue mod 16 occurs on either side, equal and unequal): results and guards."""
    sizes = _mixed_sizes()
    gen = torch.Generator().manual_seed(11)
    ge = torch.randint(1, 8, (len(sizes),), generator=gen).tolist()
    gp = torch.randint(1, 8, (len(sizes),), generator=gen).tolist()
    E, P = Carved(sizes, ge, _random_values(sizes, gen)), Carved(sizes, gp, _random_values(sizes, gen))
    residues = {(s % 4, t % 4) for s, t in zip(E.starts, P.starts)}
    assert len(residues) == 16
    _check_set(dev, E, P, kinds=(kind,), what="mixed")


@pytest.mark.parametrize("shift_e,shift_p", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 2), (3, 3)])
def test_alignment_of_dst_src_and_both(dev, shift_e, shift_p):
    """Every tensor of the set starts on a 16-byte boundary of its buffer (gaps pad to multiples of four elements); the
    buffers themselves are views offset by 4, 8 or 12 bytes: dst only, src only, both."""
    c = _chunk()
    sizes = [1, 3, 4, 5, 7, 8, 1023, c - 1, c, c + 1, 2 * c + 5]
    gaps, pos = [], 0
    for n in sizes:
        g = 4 + (-pos) % 4
        gaps.append(g)
        pos += g + n
    gen = torch.Generator().manual_seed(13)
    E, P = Carved(sizes, gaps, _random_values(sizes, gen)), Carved(sizes, gaps, _random_values(sizes, gen))
    assert all(s % 4 == 0 for s in E.starts)
    _check_set(dev, E, P, decays=(0.999,), shift_e=shift_e, shift_p=shift_p, what=f"shift {shift_e},{shift_p}")


def test_second_grid_trip(dev):
    """cap + 3 chunks, one large tensor plus tails: the first three workgroups take a second chunk."""
    from ssl_amd import _lib
    L = _lib.lib()
    c, cap = L.ssg_multi_chunk(), L.ssg_multi_grid_cap()
    sizes = [cap * c - 7, 5, c, 1]
    gen = torch.Generator().manual_seed(17)
    E, P = Carved(sizes, [1, 2, 3, 5], _random_values(sizes, gen)), Carved(sizes, [1, 2, 3, 5], _random_values(sizes, gen))
    counts = np.ascontiguousarray(sizes, dtype=np.uintp)
    assert L.ssg_multi_chunks(len(sizes), counts.ctypes.data) == cap + 3
    _check_set(dev, E, P, decays=(0.999,), what="second trip")


def test_special_values(dev):
    """+-0, subnormals, +-inf and NaN in e, in p and in both (every pairing), under every kind and decay: decay = 0 with
    an infinite e is 0 * inf = NaN, as the reference's product gives it."""
    s = torch.tensor([0.0, -0.0, 1e-40, -1e-40, float("inf"), -float("inf"), float("nan"), 1.5, -3.0e38])
    e_vals, p_vals = s.repeat_interleave(len(s)), s.repeat(len(s))
    gen = torch.Generator().manual_seed(19)
    sizes = [len(e_vals), 37, len(e_vals)]
    ev = [e_vals, torch.randn(37, generator=gen), e_vals.flip(0)]
    pv = [p_vals, s[torch.randint(0, len(s), (37,), generator=gen)], p_vals]
    E, P = Carved(sizes, [3, 1, 2], ev), Carved(sizes, [3, 5, 2], pv)
    want = torch.tensor([float("inf")]).mul_(0.0).add_(torch.tensor([1.0]), alpha=1.0)
    assert bool(torch.isnan(want).all())
    _check_set(dev, E, P, what="special values")


def _conv_nets(dev, dtype=torch.float32, fmt_net=torch.contiguous_format, fmt_ema=torch.contiguous_format, seed=23):
    torch.manual_seed(seed)
    make = lambda: nn.Sequential(nn.Conv2d(3, 6, 3), nn.PReLU(), nn.Conv2d(6, 5, 3, bias=False))  # noqa: E731
    net, avg = make().to(dev, dtype).to(memory_format=fmt_net), make().to(dev, dtype).to(memory_format=fmt_ema)
    return net, avg


def _cpu_twin(module, device="cpu"):
    """name -> a copy of each parameter WITH ITS STRIDES, on the CPU (or on `device`)."""
    out = {}
    for k, p in module.named_parameters():
        c = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=device)
        c.copy_(p.detach())
        out[k] = c
    return out


def _check_model_ema(net, avg, decay, steps=2, native=None, twin_on="cpu"):
    from ssl_amd import ema
    m = ema.ModelEma(net, avg)
    want, src = _cpu_twin(avg, twin_on), _cpu_twin(net, twin_on)
    for _ in range(steps):
        m.update(decay)
        for k in want:
            R.ema_update(want[k], src[k], decay)
    torch.cuda.synchronize()
    for k, p in avg.named_parameters():
        print(k, "elements that differ from the CPU's expression:", int((R.bits(p) != R.bits(want[k])).sum()))
    for k, p in avg.named_parameters():
        assert R.same_bits(p, want[k]), k
    if native is not None:
        assert (m._ema._fallback == []) == native and bool(m._ema._tables) == native
    return m


def test_model_ema_function_forms_and_copy(dev):
    from ssl_amd import ema
    net, avg = _conv_nets(dev)
    want, src = _cpu_twin(avg), _cpu_twin(net)
    ema.model_ema(net, avg, 0.999)
    ema.update_E(net, avg)
    for k in want:
        R.ema_update(R.ema_update(want[k], src[k], 0.999), src[k], 0.999)
    for k, p in avg.named_parameters():
        assert R.same_bits(p, want[k]), k
    m = _check_model_ema(net, avg, 0.9999, native=True)
    m.copy()
    for k, p in avg.named_parameters():
        assert R.same_bits(p, src[k]), k


def test_channels_last_pair_is_native(dev):
    net, avg = _conv_nets(dev, fmt_net=torch.channels_last, fmt_ema=torch.channels_last)
    assert not net[0].weight.is_contiguous() and net[0].weight.stride() == avg[0].weight.stride()
    _check_model_ema(net, avg, 0.999, native=True)


def test_pairs_outside_the_native_domain_take_the_expression(dev):
    """Different strides, fp16, and everything after set_native_criteria(False): the reference's expression per pair.

    The fp32 pairs are held to the expression on the CPU copies like everything else in this file.  The fp16 pair is held
    to the same expression (ema_reference.ema_update) on copies ON THE DEVICE: the fallback is torch's own kernels on
    those tensors, what the reference's loop would run there, and torch's fp16 mul_ / add_ on the GPU and on the CPU are
    not the same bits (measured: 1 of 162 elements of the first weight differs after two updates, 2 after three; the
    count against the CPU copies is printed)."""
    from ssl_amd import ema
    from ssl_amd.losses import set_native_criteria
    net, avg = _conv_nets(dev, fmt_net=torch.channels_last)
    m = _check_model_ema(net, avg, 0.999)
    assert len(m._ema._fallback) == 2 and len(m._ema._tables) == 1        # the two 4-d weights; PReLU and the bias native
    net, avg = _conv_nets(dev, dtype=torch.float16)
    _check_model_ema(net, avg, 0.999, native=False, twin_on=dev)
    cpu, src = _cpu_twin(avg), _cpu_twin(net)
    for k, p in avg.named_parameters():                  # (the observation: one more update on either side)
        R.ema_update(cpu[k], src[k], 0.999)
    ema.ModelEma(net, avg).update(0.999)
    for k, p in avg.named_parameters():
        print(k, "fp16 elements that differ from the CPU's expression:", int((R.bits(p) != R.bits(cpu[k])).sum()))
    net, avg = _conv_nets(dev)
    prev = set_native_criteria(False)
    try:
        m = _check_model_ema(net, avg, 0.999, native=False)
    finally:
        set_native_criteria(prev)
    want, src = _cpu_twin(avg), _cpu_twin(net)
    m.update(0.5)                                                          # the switch is seen by the next call
    assert m._ema._fallback == [] and m._ema.rebuilds == 2
    for k, p in avg.named_parameters():
        assert R.same_bits(p, R.ema_update(want[k], src[k], 0.5)), k
    assert isinstance(ema.EMA, int)


def test_rebuild_after_new_storage(dev):
    from ssl_amd import ema
    net, avg = _conv_nets(dev)
    m = ema.ModelEma(net, avg)
    m.update(0.9)
    p = net[2].weight
    old = p.data_ptr()
    p.data = p.data.clone()
    p.data.mul_(3.0)
    assert p.data_ptr() != old
    kept = [t.data_ptr() for pair in m._ema._keep for t in pair]
    assert old in kept                                   # the cache still holds the old storage: nothing can reuse it
    want, src = _cpu_twin(avg), _cpu_twin(net)
    m.update(0.9)
    torch.cuda.synchronize()
    assert m._ema.rebuilds == 2 and old not in [t.data_ptr() for pair in m._ema._keep for t in pair]
    for k, q in avg.named_parameters():
        assert R.same_bits(q, R.ema_update(want[k], src[k], 0.9)), k
    m.update(0.9)
    assert m._ema.rebuilds == 2


def test_repeat_gives_the_same_bits_and_update_is_one_apply(dev, monkeypatch):
    from ssl_amd import ema
    real, calls = ema._lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            return getattr(real, name)

        def ssg_multi_apply(self, *args):
            calls.append(args[2])
            return real.ssg_multi_apply(*args)

    monkeypatch.setattr(ema, "_library", lambda: Counting())
    results = []
    for _ in range(2):
        net, avg = nn.Module(), nn.Module()
        g = torch.Generator().manual_seed(31)
        for i in range(300):
            shape = (1 + i % 64,) if i % 3 else (2, 1 + i % 7, 3)
            net.register_parameter(f"p{i}", nn.Parameter(torch.randn(shape, generator=g).to(dev)))
            avg.register_parameter(f"p{i}", nn.Parameter(torch.randn(shape, generator=g).to(dev)))
        calls.clear()
        m = ema.ModelEma(net, avg)
        m.update(0.999)
        assert calls == [R.EMA]
        m.update(0.999)
        assert calls == [R.EMA, R.EMA] and m._ema.rebuilds == 1
        results.append(torch.cat([R.bits(p).flatten() for p in avg.parameters()]))
    assert torch.equal(results[0], results[1])


def test_lit_ema_on_the_fixtures_model_without_a_host_read(dev):
    from ssl_amd import ema
    with np.load(GOLDEN) as z:
        fixture = {k: np.asarray(z[k]) for k in z.files}
    net = R.fixture_model({k[5:]: v for k, v in fixture.items() if k.startswith("init_")}).to(dev)
    pert = {k[5:]: torch.from_numpy(v).to(dev) for k, v in fixture.items() if k.startswith("pert_")}
    lit = ema.LitEma(net, decay=R.FIXTURE_DECAY).to(dev)
    shadows = {s: [] for s in lit.m_name2s_name.values()}
    has_mode = hasattr(torch.cuda, "set_sync_debug_mode")
    assert has_mode, "this torch has no sync debug mode: count device-to-host copies with the profiler instead"
    for t in range(R.FIXTURE_STEPS):
        R.perturb(net, pert, t)
        if t == 0:
            lit(net)                                      # builds and uploads the table
            torch.cuda.synchronize()
        else:
            torch.cuda.set_sync_debug_mode("error")
            try:
                lit(net)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        for s in shadows:
            shadows[s].append(dict(lit.named_buffers())[s].clone())
    torch.cuda.synchronize()
    assert lit._forward.rebuilds == 1 and lit._forward._fallback == []
    for s, steps in shadows.items():
        for t, got in enumerate(steps):
            assert R.same_bits(got, torch.from_numpy(fixture["shadow_" + s][t])), (s, t)
    assert int(lit.num_updates) == R.FIXTURE_STEPS
    live = {n: p.detach().clone() for n, p in net.named_parameters()}
    lit.store(net.parameters())
    lit.copy_to(net)
    for n, p in net.named_parameters():
        want = torch.from_numpy(fixture["shadow_" + n.replace(".", "")][-1]) if p.requires_grad else live[n]
        assert R.same_bits(p, want), n
    lit.restore(net.parameters())
    for n, p in net.named_parameters():
        assert R.same_bits(p, live[n]), n


def test_replays_as_hip_graph(dev):
    """One linear capture on one stream: three replays equal three eager updates bit for bit."""
    from ssl_amd import ema
    net, avg = _conv_nets(dev)
    _, twin = _conv_nets(dev)
    for a, b in zip(twin.parameters(), avg.parameters()):
        a.data.copy_(b.data)
    eager, rec = ema.ModelEma(net, twin), ema.ModelEma(net, avg)
    start = [p.detach().clone() for p in avg.parameters()]
    rec.update(0.999)                                     # builds the table outside the capture
    torch.cuda.synchronize()
    for p, s in zip(avg.parameters(), start):
        p.data.copy_(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec.update(0.999)
    for p, s in zip(avg.parameters(), start):             # (a capture does not run)
        p.data.copy_(s)
    gen = torch.Generator().manual_seed(37)
    for _ in range(3):
        for p in net.parameters():
            p.data.copy_(torch.randn(p.shape, generator=gen))
        eager.update(0.999)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(twin.parameters(), avg.parameters()):
            assert torch.equal(R.bits(a), R.bits(b))
    assert rec._ema.rebuilds == 1
    want = _cpu_twin(twin)
    assert any(not torch.equal(w, s.cpu()) for w, s in zip(want.values(), start))

