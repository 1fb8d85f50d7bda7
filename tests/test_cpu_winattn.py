"""The window attention without a GPU: the fp64 restatement against torch's autograd, the label rule against the
constructed mask, the bound against eight wrong restatements and against torch's own fp32 lines, the restated SwinIR
against a fixture recorded from the reference's class, the symbols and every refusal of the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import winattn_cases as C
import winattn_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f38_swinir.npz")
SMALL_NET = dict(img_size=16, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=8, upscale=2,
                 upsampler="pixelshuffle")
NAMES = ("ssg_winattn_grid_cap", "ssg_winattn_workspace_bytes", "ssg_winattn_forward", "ssg_winattn_backward")


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


def _torch_lines(case, dtype):
    """out, dqkv, dtable of the package's torch route (the reference's operations) with autograd, as numpy"""
    from ssl_amd import winattn
    qkv, table, dout, scale = C.make(case)
    scale = float(np.float32(scale))        # the fp32 value that the kernels and torch's fp32 product take
    q = torch.from_numpy(qkv).to(dtype).requires_grad_(True)
    t = torch.from_numpy(table).to(dtype).requires_grad_(True)
    out = winattn.window_attention(q, t, case["heads"], 8, case["shift"], scale)
    out.backward(torch.from_numpy(dout).to(dtype))
    return out.detach().numpy(), q.grad.numpy(), t.grad.numpy()


# ---- the restatement is the reference's formula ----
@pytest.mark.parametrize("case", C.SMALL, ids=lambda c: c["name"])
def test_restatement_against_fp64_autograd_of_the_reference_formula(case):
    want = C.reference(case)
    out, dqkv, dtable = _torch_lines(case, torch.float64)
    for name, got, ref in (("out", out, want.out), ("dqkv", dqkv, want.dqkv), ("dtable", dtable, want.dtable)):
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), name
        if nan.all():
            continue
        size = np.abs(ref[~nan]).max()
        assert np.abs(got[~nan] - ref[~nan]).max() <= 1e-12 * max(size, 1.0), name


def test_nan_case_fills_exactly_one_window():
    case = C.by_name("nan_s4")
    want = C.reference(case)
    b, y, x = C.NAN_TOKEN
    src, _ = R.geometry(case["H"], case["W"], case["shift"])
    window = src[np.argwhere(src == y * case["W"] + x)[0, 0]]
    inside = np.zeros(case["H"] * case["W"], dtype=bool)
    inside[window] = True
    for a in (want.out, want.dqkv):
        nan = np.isnan(a).reshape(case["B"], case["H"] * case["W"], -1)
        assert nan[b, inside].all() and not nan[b, ~inside].any()


@pytest.mark.parametrize("shift", [1, 4, 7])
@pytest.mark.parametrize("H", [8, 16, 24, 32, 40])
@pytest.mark.parametrize("W", [8, 16, 24, 32, 40])
def test_label_rule_is_the_constructed_mask(H, W, shift):
    from ssl_amd import winattn
    want = winattn.shift_mask(H, W, 8, shift).numpy()
    got = R.label_mask(H, W, shift).astype(np.float32)
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_index_buffer_is_the_bias_rule():
    from ssl_amd import archs, winattn
    assert np.array_equal(winattn.relative_position_index(8).numpy(), R.bias_index())
    assert np.array_equal(archs.WindowAttention(12, (8, 8), 2).relative_position_index.numpy(), R.bias_index())


# ---- the bound is not vacuous, and torch's fp32 lines meet it ----
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_wrong_restatement_leaves_the_bound(mutant):
    worst = 0.0
    for case in C.SHAPES + [C.by_name("big_s4")]:
        want = C.reference(case)
        qkv, table, dout, scale = C.make(case)
        got = R.evaluate(qkv, table, case["heads"], case["shift"], scale, dout, mutant=mutant)
        worst = max(worst, R.share(got.out, want.out, want.out_bound), R.share(got.dqkv, want.dqkv, want.dqkv_bound))
    assert worst > 1.0, (mutant, worst)


@pytest.mark.parametrize("case", C.SMALL, ids=lambda c: c["name"])
def test_torchs_fp32_lines_meet_the_bounds_on_the_cpu(case):
    """out and dqkv: the kernels' bound (it holds for any order of summation); dtable: the wider fp32-sum bound."""
    want = C.reference(case)
    out, dqkv, dtable = _torch_lines(case, torch.float32)
    shares = (R.share(out, want.out, want.out_bound), R.share(dqkv, want.dqkv, want.dqkv_bound),
              R.share(dtable, want.dtable, want.dtable_bound_fp32))
    print(case["name"], "torch fp32 shares of the bound: out %.3f dqkv %.3f dtable %.3f" % shares)
    assert max(shares) <= 1.0, shares


# ---- the network ----
def _golden_net(fused):
    from ssl_amd import archs
    z = np.load(GOLDEN)
    keys = [str(k) for k in z["keys"]]
    net = archs.SwinIR(fused=fused, **SMALL_NET).eval()
    state = {k: torch.from_numpy(z[f"sd_{i}"]) for i, k in enumerate(keys)}
    return net, z, keys, state


@pytest.mark.parametrize("fused", [False, True])
def test_swinir_torch_route_gives_the_reference_bits(fused):
    """(fused=True on CPU tensors takes the torch route as well)"""
    from ssl_amd import archs
    net, z, keys, state = _golden_net(fused)
    assert list(net.state_dict().keys()) == keys and len(keys) == 76
    net.load_state_dict(state, strict=True)
    taps = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: taps.append(out.detach().numpy()))
             for m in net.modules() if isinstance(m, archs.WindowAttention)]
    for tag in "ab":
        del taps[:]
        with torch.no_grad():
            y = net(torch.from_numpy(z[f"x_{tag}"])).numpy()
        assert np.array_equal(y.view(np.int32), z[f"y_{tag}"].view(np.int32)), tag
        assert len(taps) == 4
        for k, tap in enumerate(taps):
            assert np.array_equal(tap.view(np.int32), z[f"attn_{tag}_{k}"].view(np.int32)), (tag, k)
    for h in hooks:
        h.remove()


def test_swinir_buffers_and_state_dict_round_trip():
    """The buffers are registered with the reference's values, so a state dict saved here holds what the reference's
    strict load asks for: every key of the fixture with its shape and dtype, buffers bit for bit."""
    net, z, keys, state = _golden_net(True)
    fresh = net.state_dict()
    for i, k in enumerate(keys):
        assert tuple(fresh[k].shape) == z[f"sd_{i}"].shape and fresh[k].numpy().dtype == z[f"sd_{i}"].dtype, k
        if k.endswith(("relative_position_index", "attn_mask")):
            assert np.array_equal(fresh[k].numpy(), z[f"sd_{i}"]), k
    assert sum(k.endswith("attn_mask") for k in keys) == 2 and sum(k.endswith("relative_position_index") for k in keys) == 4
    net.load_state_dict(state, strict=True)
    back = net.state_dict()
    assert all(np.array_equal(back[k].numpy(), z[f"sd_{i}"]) for i, k in enumerate(keys))


def test_swinir_other_constructions_run_on_the_cpu():
    from ssl_amd import archs
    x = torch.rand(1, 3, 10, 13)
    for kwargs, scale in ((dict(upsampler="pixelshuffledirect", upscale=3), 3), (dict(upsampler="nearest+conv", upscale=4), 4),
                          (dict(upsampler="", upscale=1, resi_connection="3conv", ape=True, img_size=16), 1)):
        net = archs.SwinIR(**dict(dict(img_size=16, embed_dim=8, depths=[2], num_heads=[2], window_size=8), **kwargs))
        assert net.train()(x).shape == (1, 3, 10 * scale, 13 * scale)
    net = archs.SwinIR(img_size=16, embed_dim=8, depths=[2], num_heads=[2], window_size=8, use_checkpoint=True)
    net(torch.rand(1, 3, 16, 16, requires_grad=True)).sum().backward()


def test_fallbacks_are_the_torch_route():
    from ssl_amd import winattn
    case = C.by_name("labels_s4")
    qkv, table, _, _ = C.make(case)
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        assert not winattn.is_native(torch.from_numpy(qkv).to(dtype), torch.from_numpy(table).to(dtype), 2, 8, 4)
    out = winattn.window_attention(torch.from_numpy(qkv[:, :14, :21]).contiguous(), torch.zeros(169, 2), 2, 7, 3)
    assert out.shape == (1, 14, 21, 60)


# ---- the C ABI ----
def test_symbols_are_exported_declared_and_bound(L):
    from ssl_amd import _lib
    size_t, ptr, i, f = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {"ssg_winattn_grid_cap": (i, []),
            "ssg_winattn_workspace_bytes": (size_t, [i, i, i, i, i]),
            "ssg_winattn_forward": (i, [ptr, ptr, ptr, i, i, i, i, i, i, f, ptr]),
            "ssg_winattn_backward": (i, [ptr, ptr, ptr, ptr, ptr, ptr, size_t, i, i, i, i, i, i, f, ptr])}
    assert set(want) == set(NAMES)
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert getattr(L, name).argtypes == proto[1]
        assert hasattr(ctypes.CDLL(_lib.PROF_SO_PATH), name)
    assert L.ssg_abi_version() == 6
    assert L.ssg_winattn_grid_cap() == 1024
    # one partial of 225 doubles per workgroup; the grid is the unit count under the cap rounded down to the heads
    assert L.ssg_winattn_workspace_bytes(1, 16, 24, 2, 30) == 8 * 225 * 12
    assert L.ssg_winattn_workspace_bytes(3, 64, 64, 6, 10) == 8 * 225 * 1020
    assert L.ssg_winattn_workspace_bytes(1, 8, 8, 2000, 1) == 8 * 225 * 2000


def test_every_refusal_is_decided_before_any_launch(L):
    """(no GPU here: a call that got as far as a launch would return a HIP status, which is positive)"""
    from ssl_amd import _lib
    K = _lib.CONSTANTS
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    good = dict(qkv=p, table=p, out=p, dout=p, dqkv=p, dtable=p, ws=p, ws_bytes=8 * 225 * 12, B=1, H=16, W=24, heads=2,
                d=30, shift=4)

    def fwd(**kw):
        a = dict(good, **kw)
        return L.ssg_winattn_forward(a["qkv"], a["table"], a["out"], a["B"], a["H"], a["W"], a["heads"], a["d"],
                                     a["shift"], 0.5, None)

    def bwd(**kw):
        a = dict(good, **kw)
        return L.ssg_winattn_backward(a["qkv"], a["table"], a["dout"], a["dqkv"], a["dtable"], a["ws"], a["ws_bytes"],
                                      a["B"], a["H"], a["W"], a["heads"], a["d"], a["shift"], 0.5, None)

    shapes = [dict(B=0), dict(H=0), dict(W=-8), dict(H=12), dict(W=20), dict(shift=-1), dict(shift=8), dict(d=0),
              dict(d=33), dict(heads=0)]
    for kw in shapes:
        assert fwd(**kw) == K["SSG_E_BADARG"], kw
        assert bwd(**kw) == K["SSG_E_BADARG"], kw
        a = dict(good, **kw)
        if "shift" not in kw:               # (the size does not depend on the shift)
            assert L.ssg_winattn_workspace_bytes(a["B"], a["H"], a["W"], a["heads"], a["d"]) == 0, kw
    for name in ("qkv", "table", "out"):
        assert fwd(**{name: None}) == K["SSG_E_BADARG"], name
        assert fwd(**{name: p + 2}) == K["SSG_E_ALIGN"], name
    for name in ("qkv", "table", "dout", "dqkv", "ws"):
        assert bwd(**{name: None}) == K["SSG_E_BADARG"], name
    for name in ("qkv", "table", "dout", "dqkv", "dtable"):
        assert bwd(**{name: p + 2}) == K["SSG_E_ALIGN"], name
    assert bwd(ws=p + 4) == K["SSG_E_ALIGN"]
    assert bwd(ws_bytes=8 * 225 * 12 - 1) == K["SSG_E_WORKSPACE"]
    assert bwd(ws_bytes=0) == K["SSG_E_WORKSPACE"]
    assert fwd(B=2 ** 31 - 1, H=2 ** 16, W=2 ** 16) == K["SSG_E_TOOLARGE"]
    assert fwd(B=2 ** 30, heads=64, d=1) == K["SSG_E_TOOLARGE"]
    assert not buf.any()
