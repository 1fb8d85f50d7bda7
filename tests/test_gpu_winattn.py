"""The window-attention kernels on the GPU: the bare C ABI against the fp64 restatement within its derived bound on every
case, every 4-byte offset of every buffer between guards, bit-for-bit repeats and batch independence, NaN containment,
ssl_amd.winattn under autograd against the torch route, a HIP-graph replay, and SwinIR end to end."""
import os

import numpy as np
import pytest
import torch

import winattn_cases as C
import winattn_reference as R

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f38_swinir.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Buf:
    """n floats at float offset `off` behind a 16-byte boundary, between guard words; an output starts as NaNs (an
    element that nobody writes shows)."""

    def __init__(self, dev, data=None, n=None, off=0):
        self.n, self.lo = (data.size if data is not None else n), 4 + off
        self.holder = torch.full((self.n + 12,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.holder[self.lo:self.lo + self.n]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).ravel()))
        else:
            self.view.fill_(float("nan"))
        assert self.view.data_ptr() % 16 == 4 * (off % 4)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        h = self.holder
        return bool((h[:self.lo] == SENTINEL).all()) and bool((h[self.lo + self.n:] == SENTINEL).all())

    def numpy(self, shape):
        return self.view.cpu().numpy().reshape(shape)


def run(dev, case, arrays=None, offs=(0, 0, 0, 0, 0), want_table=True, backward=True):
    """(out, dqkv, dtable) of one forward and one backward call of the bare C ABI, guards checked; offs: the float
    offsets of qkv, out, dout, dqkv and the two tables."""
    from ssl_amd import _lib
    L = _lib.lib()
    qkv, table, dout, scale = arrays if arrays is not None else C.make(case)
    B, H, W = qkv.shape[:3]
    heads, d, shift = case["heads"], case["d"], case["shift"]
    st = torch.cuda.current_stream().cuda_stream
    b_qkv, b_tab, b_dout = Buf(dev, qkv, off=offs[0]), Buf(dev, table, off=offs[4]), Buf(dev, dout, off=offs[2])
    b_out, b_dqkv = Buf(dev, n=dout.size, off=offs[1]), Buf(dev, n=qkv.size, off=offs[3])
    b_dtab = Buf(dev, n=table.size, off=offs[4])
    _lib.check(L.ssg_winattn_forward(b_qkv.ptr, b_tab.ptr, b_out.ptr, B, H, W, heads, d, shift, scale, st))
    res = [b_out.numpy(dout.shape), None, None]
    if backward:
        nbytes = L.ssg_winattn_workspace_bytes(B, H, W, heads, d)
        assert nbytes > 0
        ws = torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)   # (no zero-fill is relied on)
        _lib.check(L.ssg_winattn_backward(b_qkv.ptr, b_tab.ptr, b_dout.ptr, b_dqkv.ptr, b_dtab.ptr if want_table else None,
                                          ws.data_ptr() if want_table else None, nbytes if want_table else 0, B, H, W,
                                          heads, d, shift, scale, st))
        res[1] = b_dqkv.numpy(qkv.shape)
        res[2] = b_dtab.numpy(table.shape) if want_table else None
        assert bool(torch.isnan(ws[-1]))
    torch.cuda.synchronize()
    for b in (b_qkv, b_tab, b_dout, b_out, b_dqkv, b_dtab):
        assert b.intact()
    assert np.array_equal(b_qkv.numpy(qkv.shape).view(np.int32), qkv.view(np.int32))      # inputs are only read
    return res


def bits(a):
    return a.view(np.int32)


@pytest.mark.parametrize("case", C.ALL, ids=lambda c: c["name"])
def test_abi_against_the_restatement_within_the_bound(dev, case):
    want = C.reference(case)
    out, dqkv, dtable = run(dev, case)
    shares = (R.share(out, want.out, want.out_bound), R.share(dqkv, want.dqkv, want.dqkv_bound),
              R.share(dtable, want.dtable, want.dtable_bound))
    print(case["name"], "kernel shares of the bound: out %.3f dqkv %.3f dtable %.3f" % shares)
    assert max(shares) <= 1.0, shares


def test_uniform_rows_zero_input_and_one_window_gradient(dev):
    """What the special contents promise, exactly: identical keys give equal weights; all-zero qkv gives a zero output;
    a dout inside one window gives a dqkv that is zero outside it."""
    case = C.by_name("same_keys")
    qkv, table, dout, scale = C.make(case)
    out, _, _ = run(dev, case)
    v = qkv.reshape(1, 16, 24, 3, 2, 30)[:, :, :, 2].astype(np.float64)
    mean = v.reshape(2, 8, 3, 8, 2, 30).mean(axis=(1, 3))                             # (wy, wx, heads, d)
    want = np.broadcast_to(mean[:, None, :, None], (2, 8, 3, 8, 2, 30)).reshape(1, 16, 24, 60)
    assert np.abs(out - want).max() <= 66 * R.U * np.abs(v).max()
    out, _, _ = run(dev, C.by_name("zeros_s4"))
    assert not out.any()
    case = C.by_name("one_window_dout")
    _, _, dout, _ = C.make(case)
    _, dqkv, _ = run(dev, case)
    outside = ~dout.any(axis=-1)
    assert outside.sum() == 16 * 24 - 64 and not dqkv[outside].any() and dqkv[~outside].all()


@pytest.mark.parametrize("name", ["labels_s4", "batch_d31"])
def test_every_offset_of_every_buffer_between_guards(dev, name):
    case = C.by_name(name)
    want = run(dev, case)
    for which in range(5):
        for off in (1, 2, 3):
            offs = [0] * 5
            offs[which] = off
            got = run(dev, case, offs=offs)
            for a, b in zip(got, want):
                assert np.array_equal(bits(a), bits(b)), (which, off)


def test_repeat_and_batch_independence_bit_for_bit(dev):
    case = C.by_name("batch_d10")
    arrays = C.make(case)
    want = run(dev, case, arrays)
    again = run(dev, case, arrays)
    for a, b in zip(again, want):
        assert np.array_equal(bits(a), bits(b))
    qkv, table, dout, scale = arrays
    for b in range(case["B"]):
        out, dqkv, _ = run(dev, case, (qkv[b:b + 1], table, dout[b:b + 1], scale))
        assert np.array_equal(bits(out[0]), bits(want[0][b])) and np.array_equal(bits(dqkv[0]), bits(want[1][b]))
    no_table = run(dev, case, arrays, want_table=False)
    assert np.array_equal(bits(no_table[1]), bits(want[1])) and no_table[2] is None


def test_second_grid_trip_equals_its_images_alone(dev):
    """1,152 units on 1,020 workgroups: a unit taken on a workgroup's second trip gives the bits it gives on a first."""
    from ssl_amd import _lib
    case = C.SECOND_TRIP
    assert _lib.lib().ssg_winattn_workspace_bytes(3, 64, 64, 6, 10) // (8 * 225) == 1020 < 3 * 64 * 6
    qkv, table, dout, scale = arrays = C.make(case)
    want = run(dev, case, arrays)
    for b in range(case["B"]):
        out, dqkv, _ = run(dev, case, (qkv[b:b + 1], table, dout[b:b + 1], scale))
        assert np.array_equal(bits(out[0]), bits(want[0][b])) and np.array_equal(bits(dqkv[0]), bits(want[1][b]))


def test_a_nan_token_stays_inside_its_window(dev):
    case = C.by_name("nan_s4")
    clean = dict(case, content="random")
    out, dqkv, _ = run(dev, case)
    out0, dqkv0, _ = run(dev, clean)
    b, y, x = C.NAN_TOKEN
    src, _ = R.geometry(case["H"], case["W"], case["shift"])
    inside = np.zeros(case["H"] * case["W"], dtype=bool)
    inside[src[np.argwhere(src == y * case["W"] + x)[0, 0]]] = True
    inside = inside.reshape(case["H"], case["W"])
    for a, a0 in ((out, out0), (dqkv, dqkv0)):
        assert np.isnan(a[b][inside]).all()
        assert np.array_equal(bits(a[b][~inside]), bits(a0[b][~inside]))


class Counting:
    """The library behind ssl_amd.winattn's seam, counting the launching calls."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name in ("ssg_winattn_forward", "ssg_winattn_backward"):
            def counted(*args):
                self.calls.append(name)
                return fn(*args)
            return counted
        return fn


@pytest.fixture
def counted(monkeypatch):
    from ssl_amd import _lib, winattn
    c = Counting(_lib.lib())
    monkeypatch.setattr(winattn, "_library", lambda: c)
    return c


def _autograd(fn, qkv, table, dout):
    q, t = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
    out = fn(q, t)
    out.backward(dout)
    return out.detach(), q.grad, t.grad


@pytest.mark.parametrize("name", ["labels_s4", "batch_d32", "big_s4"])
def test_window_attention_under_autograd_against_the_torch_route(dev, counted, name):
    from ssl_amd import winattn
    case = C.by_name(name)
    want = C.reference(case)
    qkv, table, dout, scale = (torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in C.make(case))
    heads, shift = case["heads"], case["shift"]
    native = _autograd(lambda q, t: winattn.window_attention(q, t, heads, 8, shift), qkv, table, dout)
    assert counted.calls == ["ssg_winattn_forward", "ssg_winattn_backward"]
    torchs = _autograd(lambda q, t: winattn.torch_route(q, t, heads, 8, shift), qkv, table, dout)
    assert len(counted.calls) == 2
    # the sum of both bounds: torch's lines meet the kernels' for out and dqkv and the fp32-sum one for the table
    both = (2 * want.out_bound, 2 * want.dqkv_bound, want.dtable_bound + want.dtable_bound_fp32)
    for a, b, bound in zip(native, torchs, both):
        assert (np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy()) <= bound).all()
    # the native results are the bare ABI's
    bare = run(dev, case)
    for a, b in zip(native, bare):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


def test_fallbacks_really_take_the_torch_route(dev, counted):
    from ssl_amd import losses, winattn
    case = C.by_name("labels_s4")
    qkv, table, dout, scale = (torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in C.make(case))
    want = winattn.torch_route(qkv, table, 2, 8, 4)
    calls = [lambda: winattn.window_attention(qkv.double(), table.double(), 2, 8, 4),
             lambda: winattn.window_attention(qkv.half(), table.half(), 2, 8, 4),
             lambda: winattn.window_attention(qkv.cpu(), table.cpu(), 2, 8, 4),
             lambda: winattn.window_attention(qkv[:, :14, :21].contiguous(), table[:169].contiguous(), 2, 7, 3),
             lambda: winattn.window_attention(qkv, table[:, :1].contiguous(), 1, 8, 4)]          # head_dim 60
    for call in calls:
        call()
    prev = losses.set_native_criteria(False)
    try:
        off = winattn.window_attention(qkv, table, 2, 8, 4)
    finally:
        losses.set_native_criteria(prev)
    assert counted.calls == [] and torch.equal(off, want)
    winattn.window_attention(qkv, table, 2, 8, 4)
    assert counted.calls == ["ssg_winattn_forward"]


def test_forward_replays_from_a_hip_graph(dev):
    from ssl_amd import winattn
    case = C.by_name("batch_d10")
    qkv, table, _, _ = (torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in C.make(case))
    other = torch.flip(qkv, dims=(0,)).contiguous()
    eager = [winattn.window_attention(x, table, 6, 8, 3).clone() for x in (qkv, other)]
    static = qkv.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        winattn.window_attention(static, table, 6, 8, 3)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = winattn.window_attention(static, table, 6, 8, 3)
    for x, want in ((other, eager[1]), (qkv, eager[0])):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def _fixture_state():
    z = np.load(GOLDEN)
    return {str(k): torch.from_numpy(z[f"sd_{i}"]) for i, k in enumerate(z["keys"])}


def _random_state(cfg):
    from ssl_amd import archs
    torch.manual_seed(30)
    net = archs.SwinIR(fused=False, **cfg)
    gen = torch.Generator().manual_seed(3030)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(torch.randn(p.shape, generator=gen))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            elif name.endswith("qkv.weight"):
                p.copy_(0.5 * torch.randn(p.shape, generator=gen))
    return net.state_dict()


NETS = {"fixture": (dict(img_size=16, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=8, upscale=2,
                         upsampler="pixelshuffle"), _fixture_state),
        "head_dim_30": (dict(img_size=16, embed_dim=60, depths=[2, 2], num_heads=[2, 2], window_size=8, upscale=2,
                             upsampler="pixelshuffle"), None)}


@pytest.mark.parametrize("which", list(NETS))
def test_swinir_end_to_end_fused_against_torch_against_fp64(dev, counted, which):
    """Forward and backward of the same weights three ways.  The native module's largest deviation from the fp64 module is
    at most 4 x that of torch's fp32 module, for the output and for every parameter gradient: both are fp32 evaluations
    that differ in the order of their roundings, not in their number."""
    from ssl_amd import archs
    cfg, state = NETS[which]
    state = state() if state else _random_state(cfg)
    gen = torch.Generator().manual_seed(77)
    x = torch.rand((2, 3, 16, 24), generator=gen)
    results = {}
    for tag, fused, dtype in (("native", True, torch.float32), ("torch", False, torch.float32), ("fp64", False, torch.float64)):
        net = archs.SwinIR(fused=fused, **cfg).eval()
        net.load_state_dict(state, strict=True)
        net = net.to(dev, dtype)
        del counted.calls[:]
        y = net(x.to(dev, dtype))
        weight = torch.rand(y.shape, generator=torch.Generator().manual_seed(78)).to(dev, dtype)
        (y * weight).sum().backward()
        results[tag] = (y.detach().double().cpu(), {n: p.grad.double().cpu() for n, p in net.named_parameters()})
        assert counted.calls == (["ssg_winattn_forward"] * 4 + ["ssg_winattn_backward"] * 4 if tag == "native" else [])
    ref_y, ref_g = results["fp64"]
    worst = (0.0, None)
    rows = []
    for name in ["output"] + list(ref_g):
        ref = ref_y if name == "output" else ref_g[name]
        native, torchs = ((results[t][0] if name == "output" else results[t][1][name]) for t in ("native", "torch"))
        dn, dt = float((native - ref).abs().max()), float((torchs - ref).abs().max())
        rows.append((name, dn, dt))
        ratio = dn / dt if dt > 0 else (0.0 if dn == 0 else float("inf"))
        worst = max(worst, (ratio, name))
    print(which, "largest deviation from fp64, native / torch fp32: output %.3e / %.3e; worst ratio %.2f (%s)"
          % (rows[0][1], rows[0][2], worst[0], worst[1]))
    for name, dn, dt in rows:
        assert dn <= 4 * dt, (name, dn, dt)
