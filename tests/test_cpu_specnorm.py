"""What of the fused spectral normalisation (ssl_amd/csrc/ssg_specnorm.hip, ssl_amd/spectral.py, ssl_amd/archs.py) can
be checked without a device: the restatement tests/specnorm_reference.py against torch's own hook on the CPU (forward and
gradient, within the wider fp32 bound) and against a full fp64 module, every case of tests/specnorm_cases.py inside
the restatement's own bounds, the C ABI's symbols, table and refusals, and the Python layer on CPU modules, where it
must give torch's bits."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn.utils import remove_spectral_norm, spectral_norm
from torch.nn.utils.spectral_norm import SpectralNorm

import specnorm_cases as C
import specnorm_reference as R

WORD = 8


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


def _arr(values):
    return np.ascontiguousarray(values, dtype=np.uintp)


def _torch_layer(W, u, v, dtype=torch.float32):
    """torch's spectral_norm on a bias-free Linear holding W (R x K), its vectors set to u, v."""
    R_, K = C.rows_cols(W.shape)
    m = spectral_norm(nn.Linear(K, R_, bias=False)).to(dtype)
    with torch.no_grad():
        m.weight_orig.copy_(torch.from_numpy(W.reshape(R_, K)))
        m.weight_u.copy_(torch.from_numpy(u))
        m.weight_v.copy_(torch.from_numpy(v))
    return m


def _hook(m):
    return next(h for h in m._forward_pre_hooks.values() if isinstance(h, SpectralNorm))


# ---- the restatement is torch's function ----
@pytest.mark.parametrize("shape", [(6, 72), (1, 5), (5, 1), (33, 65), (12, 3, 4, 4)])
@pytest.mark.parametrize("training", [True, False])
def test_restatement_against_torchs_hook_on_the_cpu(shape, training):
    """torch's fp32 lines within the bound for sums of unit roundoff 2^-24 and eight roundings behind the last cast."""
    (W, u, v), = C.layer_set([shape], seed=2)
    G, = C.gradients([shape])
    m = _torch_layer(W, u, v).train(training)
    weight = _hook(m).compute_weight(m, do_power_iteration=training)
    (weight * torch.from_numpy(G.reshape(weight.shape))).sum().backward()
    f = R.forward(W, u, v, training)
    b = R.backward(W, f, G)
    bd = R.bounds(W, u, f, training, G, b, E=R.E32, rounds=8)
    flat = (shape[0], -1)
    shares = [R.check("v", m.weight_v.numpy(), f["v"], bd["dv"]), R.check("u", m.weight_u.numpy(), f["u"], bd["du"]),
              R.check("out", weight.detach().numpy(), f["out"].reshape(flat), bd["dout"].reshape(flat)),
              R.check("dW", m.weight_orig.grad.numpy(), b["dW"].reshape(flat), bd["ddW"].reshape(flat))]
    print(shape, training, "shares of the fp32 bound used by torch's lines (v, u, out, dW):", shares)
    assert max(shares) > 0 or not training


@pytest.mark.parametrize("shape", [(6, 72), (33, 65)])
def test_restatement_against_a_full_fp64_module(shape):
    """torch's lines in fp64 throughout differ from the restatement by its fp32 casts of v, u and sigma alone: inside
    the kernels' bound, which allows one cast on either side."""
    (W, u, v), = C.layer_set([shape], seed=4)
    G, = C.gradients([shape])
    m = _torch_layer(W, u, v, torch.float64).train()
    weight = _hook(m).compute_weight(m, do_power_iteration=True)
    (weight * torch.from_numpy(G).double()).sum().backward()
    f = R.forward(W, u, v, True)
    b = R.backward(W, f, G)
    bd = R.bounds(W, u, f, True, G, b)
    assert np.abs(m.weight_v.numpy() - f["v"]).max() <= bd["dv"].max()
    assert (np.abs(m.weight_u.numpy() - f["u"]) <= bd["du"]).all()
    assert (np.abs(weight.detach().numpy() - f["out"]) <= bd["dout"]).all()
    assert (np.abs(m.weight_orig.grad.numpy() - b["dW"]) <= bd["ddW"]).all()


def _forward_long(W, u, v, training):
    """The contract again with every sum in long double and in the REVERSE order of the rows and columns."""
    LD = np.longdouble
    W2 = W.reshape(W.shape[0], -1).astype(LD)[::-1, ::-1]
    u, v = u.astype(np.float32)[::-1], v.astype(np.float32)[::-1]
    with np.errstate(all="ignore"):
        if training:
            t = (W2 * u.astype(LD)[:, None]).sum(axis=0)
            n = np.sqrt((t * t).sum())
            v = (t / (LD(R.EPS) if n < R.EPS else n)).astype(np.float32)
        s = (W2 * v.astype(LD)[None, :]).sum(axis=1)
        if training:
            n = np.sqrt((s * s).sum())
            u = (s / (LD(R.EPS) if n < R.EPS else n)).astype(np.float32)
        sigma32 = np.float32((u.astype(LD) * s).sum())
        out = (W2.astype(np.float32) / sigma32).astype(np.float32)
    return dict(v=v[::-1], u=u[::-1], sigma32=sigma32, out=out[::-1, ::-1].reshape(W.shape))


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_every_case_stays_inside_its_own_bounds(name):
    """Each case of the GPU test through the restatement twice -- numpy's fp64 sums, and long-double sums in reverse
    order -- : the two differ by less than the derived bounds, which therefore are no tighter than fp64 allows, and the
    special contents do what the cases say (NaN for the zero layer, eps branch, exact zero for the orthogonal u)."""
    shapes, content, nan_layer = C.CASES[name]
    layers = C.layer_set(shapes, content, seed=3, nan_layer=nan_layer)
    for i, (W, u, v) in enumerate(layers):
        for training in (True, False):
            f, g = R.forward(W, u, v, training), _forward_long(W, u, v, training)
            bd = R.bounds(W, u, f, training)
            for k, bound in (("v", "dv"), ("u", "du"), ("out", "dout")):
                R.check(f"{name}[{i}] {k}", g[k], f[k], bd[bound])
            R.check(f"{name}[{i}] sigma32", np.float32(g["sigma32"]).reshape(1), np.float32(f["sigma32"]).reshape(1),
                    bd["dsig32"])
        f = R.forward(W, u, v, True)
        if content == "zero":
            assert not f["v"].any() and not f["u"].any() and np.isnan(f["out"]).all()
        if content == "tiny":
            assert np.sqrt((f["t"] ** 2).sum()) < R.EPS and np.sqrt((f["s"] ** 2).sum()) < R.EPS
        if content == "orthogonal" and W.shape[0] >= 2:
            assert not f["t"].any() and f["sigma32"] == 0
        if content == "rank1":
            assert abs(float(f["sigma32"]) - 3.0) < 1e-5
        if nan_layer is not None:
            assert np.isnan(f["out"]).all() == (i == nan_layer)


def test_case_shapes_sit_on_the_kernels_unit_sizes(L):
    assert (L.ssg_sn_strip(), L.ssg_sn_rows_a(), L.ssg_sn_rows_b(), L.ssg_sn_chunk()) == (C.STRIP, C.ROWS_A, C.ROWS_B,
                                                                                        C.CHUNK)
    dims = [C.rows_cols(s) for s in C.EDGES]
    for unit, values in ((C.STRIP, [k for _, k in dims]), (C.ROWS_A, [r for r, _ in dims]),
                         (C.ROWS_B, [r for r, _ in dims]), (C.CHUNK, [r * k for r, k in dims])):
        assert {unit - 1, unit, unit + 1} <= set(values), unit
    assert C.rows_cols(C.TALL[0])[0] > 2 * C.ROWS_A and len(C.MIXED_8) == 8 and len(C.MIXED_17) == 17


# ---- the C ABI ----
NAMES = ("ssg_sn_chunk", "ssg_sn_grid_cap", "ssg_sn_strip", "ssg_sn_rows_a", "ssg_sn_rows_b", "ssg_sn_table_bytes",
         "ssg_sn_output_bytes", "ssg_sn_workspace_bytes", "ssg_sn_saved_bytes", "ssg_sn_table_fill", "ssg_sn_forward",
         "ssg_sn_backward")


def test_symbols_are_exported_declared_and_bound(L):
    from ssl_amd import _lib
    size_t, ptr, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    want = {n: (i, []) for n in NAMES[:5]}
    want.update({n: (size_t, [size_t, ptr, ptr]) for n in NAMES[5:9]})
    want["ssg_sn_table_fill"] = (i, [size_t, ptr, ptr, ptr, ptr, ptr, ptr, size_t])
    want["ssg_sn_forward"] = (i, [ptr, ptr, i, ptr, size_t, ptr, size_t, ptr, size_t, ptr])
    want["ssg_sn_backward"] = (i, [ptr, ptr, ptr, ptr, size_t, ptr, size_t, ptr, size_t, ptr])
    assert set(want) == set(NAMES)
    for name, proto in want.items():
        assert _lib.PROTOTYPES[name] == proto, name
        assert getattr(L, name).argtypes == proto[1]
    assert L.ssg_abi_version() == 6
    assert not hasattr(L, "ssg_prof_sn_tuning") and hasattr(ctypes.CDLL(_lib.PROF_SO_PATH), "ssg_prof_sn_tuning")
    assert L.ssg_sn_chunk() % 4 == 0 and L.ssg_sn_grid_cap() >= 1


def _fill(L, w, u, v, rows, cols, slack=0):
    a = [_arr(x) for x in (w, u, v, rows, cols)]
    n = len(rows)
    nbytes = L.ssg_sn_table_bytes(n, a[3].ctypes.data, a[4].ctypes.data)
    table = np.zeros(max(nbytes // WORD, 1) + 1, dtype=np.uint64)
    rc = L.ssg_sn_table_fill(n, *(x.ctypes.data for x in a), table.ctypes.data, nbytes + slack)
    return rc, table[:nbytes // WORD]


def _addresses(rows, cols, base=0x10000000):
    """Non-overlapping W, u, v ranges for the shapes, W only 4-byte aligned."""
    w, u, v, pos = [], [], [], base + 4
    for r, k in zip(rows, cols):
        w.append(pos), u.append(pos + 4 * r * k), v.append(pos + 4 * r * k + 4 * r)
        pos += 4 * (r * k + r + k) + 4
    return w, u, v


def test_table_lists_every_unit_once_and_lays_the_blocks_out(L):
    rows, cols = [1, 5, 130, 64, 100], [1, 1, 300, 64, 8192]
    w, u, v = _addresses(rows, cols)
    rc, t = _fill(L, w, u, v, rows, cols)
    assert rc == 0
    n = len(rows)
    up = lambda a, b: -(-a // b)      # noqa: E731
    ua = [up(r, C.ROWS_A) * up(k, C.STRIP) for r, k in zip(rows, cols)]
    ub = [up(r, C.ROWS_B) for r in rows]
    ch = [up(r * k, C.CHUNK) for r, k in zip(rows, cols)]
    out = [up(r * k, 64) * 64 for r, k in zip(rows, cols)]
    ws = [up(r, C.ROWS_A) * k + r + c for r, k, c in zip(rows, cols, ch)]
    sv = [r + k + 1 for r, k in zip(rows, cols)]
    assert t[:8].tolist() == [n, sum(ua), sum(ub), sum(ch), C.CHUNK, sum(out), sum(ws), sum(sv)]
    rec = t[8:8 + 8 * n].reshape(n, 8)
    assert rec[:, 0].tolist() == w and rec[:, 1].tolist() == u and rec[:, 2].tolist() == v
    assert rec[:, 3].tolist() == rows and rec[:, 4].tolist() == cols
    starts = lambda x: np.concatenate([[0], np.cumsum(x)]).tolist()      # noqa: E731
    assert rec[:, 5].tolist() == starts(out)[:-1] and rec[:, 6].tolist() == starts(ws)[:-1]
    assert rec[:, 7].tolist() == starts(sv)[:-1]
    tail = t[8 + 8 * n:]
    assert tail.tolist() == starts(ua) + starts(ub) + starts(ch)
    r, k = _arr(rows), _arr(cols)
    assert L.ssg_sn_output_bytes(n, r.ctypes.data, k.ctypes.data) == 4 * sum(out)
    assert L.ssg_sn_workspace_bytes(n, r.ctypes.data, k.ctypes.data) == 8 * sum(ws)
    assert L.ssg_sn_saved_bytes(n, r.ctypes.data, k.ctypes.data) == 4 * sum(sv)
    assert L.ssg_sn_table_bytes(n, r.ctypes.data, k.ctypes.data) == 8 * (8 + 8 * n + 3 * (n + 1))


def test_the_fill_refuses_overlapping_and_impossible_records(L):
    from ssl_amd import _lib
    K = _lib.CONSTANTS
    rows, cols = [4, 6], [10, 3]
    w, u, v = _addresses(rows, cols)
    assert _fill(L, w, u, v, rows, cols)[0] == 0
    for which, layer, address in ((1, 0, w[0] + 4 * 39), (2, 1, u[1] + 4 * 5), (0, 1, w[0]), (1, 1, u[0]),
                                  (2, 0, w[1] - 4)):
        lists = [list(w), list(u), list(v)]
        lists[which][layer] = address                      # one range laid over another
        rc, t = _fill(L, *lists, rows, cols)
        assert rc == K["SSG_E_BADARG"] and not t.any(), (which, layer)
    lists = [list(w), list(u), list(v)]
    lists[2][1] = 0
    assert _fill(L, *lists, rows, cols)[0] == K["SSG_E_BADARG"]
    lists[2][1] = v[1] + 2
    assert _fill(L, *lists, rows, cols)[0] == K["SSG_E_ALIGN"]
    lists[2][1] = 2 ** 64 - 8                                # a range that wraps the address space
    assert _fill(L, *lists, rows, cols)[0] == K["SSG_E_BADARG"]
    assert _fill(L, w, u, v, [4, 0], cols)[0] == K["SSG_E_BADARG"]
    assert _fill(L, w, u, v, rows, [0, 3])[0] == K["SSG_E_BADARG"]
    big = _arr([2 ** 16, 6]), _arr([2 ** 15, 3])           # 2^31 elements
    assert L.ssg_sn_table_bytes(2, big[0].ctypes.data, big[1].ctypes.data) == 0
    assert L.ssg_sn_output_bytes(2, big[0].ctypes.data, big[1].ctypes.data) == 0
    table = np.zeros(64, dtype=np.uint64)
    a = [_arr(x) for x in (w, u, v)]
    assert L.ssg_sn_table_fill(2, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, big[0].ctypes.data,
                               big[1].ctypes.data, table.ctypes.data, 512) == K["SSG_E_TOOLARGE"]
    assert _fill(L, w, u, v, rows, cols, slack=-8)[0] == K["SSG_E_WORKSPACE"]
    r, k = _arr(rows), _arr(cols)
    assert L.ssg_sn_table_fill(2, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, r.ctypes.data, k.ctypes.data,
                               table.ctypes.data + 4, 512) == K["SSG_E_ALIGN"]
    assert L.ssg_sn_table_fill(2, None, a[1].ctypes.data, a[2].ctypes.data, r.ctypes.data, k.ctypes.data,
                               table.ctypes.data, 512) == K["SSG_E_BADARG"]
    assert not table.any()


def test_every_refusal_of_the_calls_is_decided_before_any_launch(L):
    """No device here: a call that reached a launch would fail otherwise (or fault); every refusal returns its own status,
    with addresses that are never dereferenced on the device."""
    from ssl_amd import _lib
    K = _lib.CONSTANTS
    rows, cols = [4, 6], [10, 3]
    w, u, v = _addresses(rows, cols)
    rc, image = _fill(L, w, u, v, rows, cols)
    assert rc == 0
    out_b, ws_b, sv_b = (int(image[5]) * 4, int(image[6]) * 8, int(image[7]) * 4)
    dev = 0x20000000                                        # stands for device memory
    good = dict(table=dev, image=image.ctypes.data, training=1, out=dev + 0x1000, out_bytes=out_b, ws=dev + 0x2000,
                ws_bytes=ws_b, saved=dev + 0x3000, saved_bytes=sv_b)

    def fwd(**kw):
        a = dict(good, **kw)
        return L.ssg_sn_forward(a["table"], a["image"], a["training"], a["out"], a["out_bytes"], a["ws"], a["ws_bytes"],
                                a["saved"], a["saved_bytes"], None)

    def bwd(grads=dev + 0x4000, **kw):
        a = dict(good, **kw)
        return L.ssg_sn_backward(a["table"], a["image"], grads, a["saved"], a["saved_bytes"], a["out"], a["out_bytes"],
                                 a["ws"], a["ws_bytes"], None)

    for call in (fwd, bwd):
        for name in ("table", "image", "out", "ws", "saved"):
            assert call(**{name: None}) == K["SSG_E_BADARG"], name
        for name, off in (("table", 4), ("image", 4), ("ws", 4), ("out", 2), ("saved", 1)):
            assert call(**{name: good[name] + off}) == K["SSG_E_ALIGN"], name
        for name in ("out_bytes", "ws_bytes", "saved_bytes"):
            assert call(**{name: good[name] - 1}) == K["SSG_E_WORKSPACE"], name
        huge = image.copy()
        huge[3] = 2 ** 31
        assert call(image=huge.ctypes.data) == K["SSG_E_TOOLARGE"]
    assert fwd(training=2) == K["SSG_E_BADARG"] and fwd(training=-1) == K["SSG_E_BADARG"]
    assert bwd(grads=None) == K["SSG_E_BADARG"] and bwd(grads=dev + 0x4004) == K["SSG_E_ALIGN"]
    rc, empty = _fill(L, [], [], [], [], [])
    assert rc == 0 and empty.tolist() == [0, 0, 0, 0, C.CHUNK, 0, 0, 0, 0, 0, 0]
    assert fwd(image=empty.ctypes.data) == 0 and bwd(image=empty.ctypes.data) == 0      # nothing to launch


# ---- the Python layer on CPU modules: torch's bits ----
def _net(seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    return nn.Sequential(spectral_norm(nn.Conv2d(3, 6, 3, 1, 1, bias=False)), nn.LeakyReLU(0.2),
                         spectral_norm(nn.Conv2d(6, 4, 3, 1, 1)), spectral_norm(nn.ConvTranspose2d(4, 4, 3, 1, 1)),
                         spectral_norm(nn.Conv2d(4, 2, 1), n_power_iterations=2)).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fused_cpu_modules_give_torchs_bits_and_keep_the_keys(dtype):
    from ssl_amd import spectral
    fused, plain = _net(3, dtype), _net(3, dtype)
    keys = list(plain.state_dict().keys())
    handle = spectral.fuse_spectral_norm(fused)
    assert [type(m) for m, _ in handle.layers] == [nn.Conv2d, nn.Conv2d]        # dim 1 and two iterations stay torch's
    assert list(fused.state_dict().keys()) == keys
    x = torch.randn(2, 3, 8, 8, dtype=dtype)
    for mode in (True, True, False):
        fused.train(mode), plain.train(mode)
        a, b = fused(x), plain(x)
        assert torch.equal(a, b)
        a.square().sum().backward(), b.square().sum().backward()
    for (k, p), q in zip(fused.named_parameters(), plain.parameters()):
        assert torch.equal(p.grad, q.grad), k
    for (k, p), q in zip(fused.state_dict().items(), plain.state_dict().values()):
        assert torch.equal(p, q), k
    assert handle._plans == [] and handle.rebuilds >= 1
    plain.load_state_dict(fused.state_dict())
    fused.load_state_dict(plain.state_dict())


def test_unfuse_restores_the_hooks_and_remove_spectral_norm_still_works():
    from ssl_amd import spectral
    net = _net(5)
    hooks = [h for m in net for h in m._forward_pre_hooks.values()]
    before = [(id(h), type(h)) for h in hooks]
    n_net_hooks = len(net._forward_pre_hooks), len(net._forward_hooks)
    handle = spectral.fuse_spectral_norm(net)
    assert [id(h) for m in net for h in m._forward_pre_hooks.values()] == [i for i, _ in before]
    assert all(isinstance(h, SpectralNorm) for h in hooks) and type(hooks[0]) is not SpectralNorm
    with pytest.raises(RuntimeError):
        spectral.fuse_spectral_norm(net)
    handle.unfuse()
    assert [(id(h), type(h)) for m in net for h in m._forward_pre_hooks.values()] == before
    assert (len(net._forward_pre_hooks), len(net._forward_hooks)) == n_net_hooks
    handle = spectral.fuse_spectral_norm(net)              # and again, then torch's removal on a fused layer
    x = torch.randn(1, 3, 8, 8)
    net(x)
    remove_spectral_norm(net[0])
    assert isinstance(net[0].weight, nn.Parameter) and not hasattr(net[0], "weight_orig")


def test_a_fused_layer_called_on_its_own_runs_torchs_hook():
    from ssl_amd import spectral
    fused, plain = _net(7), _net(7)
    spectral.fuse_spectral_norm(fused)
    x = torch.randn(1, 3, 8, 8)
    assert torch.equal(fused(x), plain(x))
    assert torch.equal(fused[0](x), plain[0](x)) and torch.equal(fused[0].weight_u, plain[0].weight_u)


def test_unet_discriminator_state_dict_round_trip_with_torchs_layers():
    """The restated UNetDiscriminatorSN and a module built from torch's layers in the same order under the reference's
    attribute names: the same keys and shapes, either loads the other's state, and on the CPU the same output bits."""
    from ssl_amd import archs

    class Plain(nn.Module):
        def __init__(self, cin, nf):
            super().__init__()
            sn = spectral_norm
            self.conv0 = nn.Conv2d(cin, nf, 3, 1, 1)
            self.conv1 = sn(nn.Conv2d(nf, nf * 2, 4, 2, 1, bias=False))
            self.conv2 = sn(nn.Conv2d(nf * 2, nf * 4, 4, 2, 1, bias=False))
            self.conv3 = sn(nn.Conv2d(nf * 4, nf * 8, 4, 2, 1, bias=False))
            self.conv4 = sn(nn.Conv2d(nf * 8, nf * 4, 3, 1, 1, bias=False))
            self.conv5 = sn(nn.Conv2d(nf * 4, nf * 2, 3, 1, 1, bias=False))
            self.conv6 = sn(nn.Conv2d(nf * 2, nf, 3, 1, 1, bias=False))
            self.conv7 = sn(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
            self.conv8 = sn(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
            self.conv9 = nn.Conv2d(nf, 1, 3, 1, 1)

    torch.manual_seed(9)
    plain, mine, kair = Plain(3, 8), archs.UNetDiscriminatorSN(3, num_feat=8), archs.Discriminator_UNet(3, 8)
    assert len(mine.spectral.layers) == 8 and isinstance(kair, archs.UNetDiscriminatorSN)
    want = {k: v.shape for k, v in plain.state_dict().items()}
    assert {k: v.shape for k, v in mine.state_dict().items()} == want
    assert list(mine.state_dict().keys()) == list(plain.state_dict().keys()) == list(kair.state_dict().keys())
    mine.load_state_dict(plain.state_dict())
    twin = archs.UNetDiscriminatorSN(3, 8, fused=False)
    twin.load_state_dict(mine.state_dict())
    plain.load_state_dict(twin.state_dict())
    x = torch.randn(2, 3, 16, 16)
    y = mine(x)
    assert torch.equal(y, twin(x)) and y.shape == (2, 1, 16, 16)
    assert all(torch.equal(a, b) for a, b in zip(mine.state_dict().values(), twin.state_dict().values()))
    assert sum(p.numel() for k, p in archs.UNetDiscriminatorSN(3).named_parameters() if "orig" in k) == 4374528
    noskip = archs.UNetDiscriminatorSN(3, 8, skip_connection=False)
    assert noskip(x).shape == (2, 1, 16, 16) and not torch.equal(noskip(x), y)
