"""The LPIPS and DISTS criteria's kernels (ssl_amd/csrc/ssg_featmetric.hip, include/ssg_hip.h section (V)) on synthetic
feature sets against the fp64 restatement of tests/featmetric_reference.py within its kernel bound; their
reproducibility, every refusal, the workspace's tail; and the modules end to end, native against the packages' torch
lines within the wider bound."""
import numpy as np
import pytest
import torch

import featmetric_cases as C
import featmetric_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _L():
    from ssl_amd import _lib
    return _lib.lib()


def _geometry():
    L = _L()
    return L.ssg_featmetric_unit(), L.ssg_featmetric_chunk(), L.ssg_featmetric_grid_cap()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _to(ts, dev):
    return [t.to(dev) for t in ts]


_sets = {}


def lpips_set(name, dev):
    """(cpu maps, device maps, restatement) of one case, computed once and left unchanged"""
    if ("l", name) not in _sets:
        unit, _, cap = _geometry()
        _, N, layers, content = next(c for c in C.lpips_cases(unit, cap) if c[0] == name)
        f0, f1, w = C.lpips_maps(N, layers, content)
        _sets["l", name] = ((f0, f1, w), (_to(f0, dev), _to(f1, dev), _to(w, dev)), R.lpips(f0, f1, w))
    return _sets["l", name]


def dists_set(name, dev):
    if ("d", name) not in _sets:
        _, N, layers, content = next(c for c in C.dists_cases(_geometry()[1]) if c[0] == name)
        x, y, a, b = C.dists_maps(N, layers, content)
        _sets["d", name] = ((x, y, a, b), (_to(x, dev), _to(y, dev), a.to(dev), b.to(dev)), R.dists(x, y, a, b))
    return _sets["d", name]


LPIPS_NAMES = [c[0] for c in C.lpips_cases(256, 1024)]
DISTS_NAMES = [c[0] for c in C.dists_cases(8192)]


# ------------------------------------------------------------------------------------------------------- LPIPS ---
@pytest.mark.parametrize("name", LPIPS_NAMES)
def test_lpips_layers_against_the_restatement(dev, name):
    from ssl_amd import metrics_feat as MF
    _, (f0, f1, w), ref = lpips_set(name, dev)
    out = MF.lpips_layers(f0, f1, w).cpu().numpy()
    K = len(f0)
    assert out.shape == (f0[0].shape[0], K + 1)
    ls, vs = R.share(out[:, :K], ref.layers, ref.layers_bound), R.share(out[:, K], ref.value, ref.value_bound)
    print(f"lpips {name}: layer share {ls:.3g} value share {vs:.3g} max bound/value "
          f"{float(np.max(ref.value_bound / np.maximum(np.abs(ref.value), 1e-300))):.3g}")
    assert ls <= 1.0 and vs <= 1.0
    assert (out[:, K] == np.cumsum(out[:, :K], axis=1)[:, -1]).all()      # the sum in layer order
    if "identical" in name:
        assert (out == 0.0).all()                                          # exactly
    if "near" in name:
        # the case an fp32 expansion fails: its error, 2^-24 of the expansion's terms, is far outside the bound
        assert float(np.max(ref.layers_bound / ref.layers)) < 1e-3
    if "second_trip" in name:
        unit, _, cap = _geometry()
        assert f0[0].shape[2] * f0[0].shape[3] > (cap + 1) * unit


def test_lpips_zero_vectors_give_the_package_value(dev):
    from ssl_amd import metrics_feat as MF
    f0 = torch.relu(torch.randn(2, 5, 3, 4, generator=torch.Generator().manual_seed(1)))
    f1 = f0.clone()
    f0[0, :, 0, 0] = 0            # one side
    f1[0, :, 0, 0] = 1
    f0[1, :, 2, 3] = 0
    f1[1, :, 2, 3] = 0            # both sides
    w = [torch.rand(5, generator=torch.Generator().manual_seed(2))]
    ref = R.lpips([f0], [f1], w)
    out = MF.lpips_layers([f0.to(dev)], [f1.to(dev)], _to(w, dev)).cpu().numpy()
    assert np.isfinite(out).all() and R.share(out[:, 0], ref.layers[:, 0], ref.layers_bound[:, 0]) <= 1.0
    # image 1 differs at no pixel but the doubly empty one, which contributes 0 / (0 + eps) = 0
    assert out[1, 0] == 0.0 and out[0, 0] > 0.0


def test_lpips_nan_reaches_its_own_image_only(dev):
    from ssl_amd import metrics_feat as MF
    _, (f0, f1, w), _ = lpips_set("k5_n3_relu", dev)
    clean = MF.lpips_layers(f0, f1, w)
    g0 = [t.clone() for t in f0]
    g0[2][1, 7, 3, 2] = float("nan")
    out = MF.lpips_layers(g0, f1, w)
    assert bool(torch.isnan(out[1, 2])) and bool(torch.isnan(out[1, 5]))
    keep = torch.ones_like(out, dtype=torch.bool)
    keep[1, 2] = keep[1, 5] = False
    assert torch.equal(_bits(out[keep]), _bits(clean[keep]))


def test_lpips_bits_repeat_batch_layer_and_offset(dev):
    from ssl_amd import metrics_feat as MF
    _, (f0, f1, w), _ = lpips_set("k5_n3_relu", dev)
    K = len(f0)
    a = MF.lpips_layers(f0, f1, w)
    assert torch.equal(_bits(a), _bits(MF.lpips_layers(f0, f1, w)))                         # a repeat
    for n in range(3):                                                                      # image n alone
        alone = MF.lpips_layers([t[n:n + 1].clone() for t in f0], [t[n:n + 1].clone() for t in f1], w)   # (elsewhere in memory)
        assert torch.equal(_bits(alone[0]), _bits(a[n])), n
    for k in range(K):                                                                      # layer k alone
        alone = MF.lpips_layers([f0[k]], [f1[k]], [w[k]])
        assert torch.equal(_bits(alone[:, 0]), _bits(a[:, k])), k

    def shifted(t):                                                                         # a 4-byte-offset view
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        buf[1:] = t.reshape(-1)
        v = buf[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    b = MF.lpips_layers([shifted(t) for t in f0], f1, [shifted(t) for t in w])
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------- DISTS ---
@pytest.mark.parametrize("name", DISTS_NAMES)
def test_dists_score_against_the_restatement(dev, name):
    from ssl_amd import metrics_feat as MF
    _, (x, y, a, b), ref = dists_set(name, dev)
    out = MF.dists_score(x, y, a, b).cpu().numpy()
    assert out.shape == (x[0].shape[0], 3) and np.isfinite(ref.score_bound).all()
    s = R.share(out[:, 0], ref.score, ref.score_bound)
    print(f"dists {name}: score share {s:.3g} max bound {float(ref.score_bound.max()):.3g}")
    assert s <= 1.0
    assert R.share(out[:, 1], ref.structure, ref.score_bound) <= 1.0
    assert R.share(out[:, 2], ref.texture, ref.score_bound) <= 1.0
    if "same" in name:
        assert (np.abs(out[:, 0]) <= ref.score_bound).all()               # y = x: 0 within the bound
    if "negated" in name:
        # anticorrelated structure and texture: S1, S2 < 0; and the bound is finer than one fp32 rounding of the score
        assert (out[:, 0] > 1.0).all() and (ref.score_bound < R.U * np.abs(ref.score)).all()


def test_dists_one_element_planes_and_nan(dev):
    from ssl_amd import metrics_feat as MF
    gen = torch.Generator().manual_seed(4)
    x, y = torch.randn(2, 6, 1, 1, generator=gen), torch.randn(2, 6, 1, 1, generator=gen)
    a, b = torch.zeros(6), torch.rand(6, generator=gen) + 0.1
    out = MF.dists_score([x.to(dev)], [y.to(dev)], a.to(dev), b.to(dev)).cpu()
    assert (out[:, 0] == 0.0).all() and (out[:, 2] == 1.0).all()          # S2 = 1 exactly on every plane: score 1 - 1
    _, (xs, ys, al, be), _ = dists_set("edges_n3_noise", dev)
    clean = MF.dists_score(xs, ys, al, be)
    bad = [t.clone() for t in xs]
    bad[2][1, 0] = float("nan")                                           # a NaN plane of image 1
    out = MF.dists_score(bad, ys, al, be)
    assert bool(torch.isnan(out[1]).all())
    assert torch.equal(_bits(out[[0, 2]]), _bits(clean[[0, 2]]))


def _dists_raw(x, y, a, b, ws_extra=0):
    """ssg_dists_score through the C ABI: (out, the workspace as doubles)"""
    from ssl_amd.engine import address_array
    L = _L()
    K, N = len(x), x[0].shape[0]
    Cs, H, W = (np.ascontiguousarray([t.shape[i] for t in x], dtype=np.int32) for i in (1, 2, 3))
    nb = L.ssg_dists_workspace_bytes(K, N, Cs.ctypes.data, H.ctypes.data, W.ctypes.data)
    ws = torch.full((nb // 8 + ws_extra,), -7.0, dtype=torch.float64, device=x[0].device)
    out = torch.empty((N, 3), dtype=torch.float64, device=x[0].device)
    ax, ay = address_array([t.data_ptr() for t in x]), address_array([t.data_ptr() for t in y])
    rc = L.ssg_dists_score(K, N, ax.ctypes.data, ay.ctypes.data, Cs.ctypes.data, H.ctypes.data, W.ctypes.data,
                           a.data_ptr(), b.data_ptr(), ws.data_ptr(), nb, out.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out, ws


def test_dists_bits_repeat_batch_layer_and_offset(dev):
    from ssl_amd import metrics_feat as MF
    _, (x, y, a, b), _ = dists_set("edges_n3_noise", dev)
    chunk = _geometry()[1]
    full = MF.dists_score(x, y, a, b)
    assert torch.equal(_bits(full), _bits(MF.dists_score(x, y, a, b)))
    for n in range(3):
        alone = MF.dists_score([t[n:n + 1].clone() for t in x], [t[n:n + 1].clone() for t in y], a, b)   # (elsewhere in memory)
        assert torch.equal(_bits(alone[0]), _bits(full[n])), n
    # layer k alone: its chunk partials (5 doubles per chunk, chunks ordered layer, image, channel, chunk) are the bits
    # of its range in the whole call's workspace
    _, ws = _dists_raw(x, y, a, b)
    at, ch = 0, 0
    for k, t in enumerate(x):
        N, Ck, H, W = t.shape
        n = 5 * N * Ck * (-(-(H * W) // chunk))
        _, alone = _dists_raw([x[k]], [y[k]], a[ch:ch + Ck].contiguous(), b[ch:ch + Ck].contiguous())
        assert alone.numel() == n and torch.equal(_bits(alone), _bits(ws[at:at + n])), k
        at, ch = at + n, ch + Ck
    assert at == ws.numel()

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    got = MF.dists_score([shifted(t) for t in x], y, shifted(a), b)
    assert torch.equal(_bits(got), _bits(full))


# --------------------------------------------------------------------------------- refusals, workspace tails ---
def _ints(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def test_refusals_and_workspace_tails(dev):
    from ssl_amd import _lib
    from ssl_amd.engine import address_array
    L = _L()
    E = _lib.CONSTANTS
    st = torch.cuda.current_stream().cuda_stream
    N, shapes = 2, [(3, 4, 5), (6, 1, 1)]
    f0 = [torch.rand(N, *s, device=dev) for s in shapes]
    f1 = [torch.rand(N, *s, device=dev) for s in shapes]
    w = [torch.rand(s[0], device=dev) for s in shapes]
    al, be = torch.rand(9, device=dev), torch.rand(9, device=dev)
    Cs, H, W = (_ints([s[i] for s in shapes]) for i in range(3))
    a0, a1, aw = (address_array([t.data_ptr() for t in ts]) for ts in (f0, f1, w))
    nl = L.ssg_lpips_workspace_bytes(2, N, Cs.ctypes.data, H.ctypes.data, W.ctypes.data)
    nd = L.ssg_dists_workspace_bytes(2, N, Cs.ctypes.data, H.ctypes.data, W.ctypes.data)
    assert nl == 8 * N * 2 and nd == 40 * N * 9
    ws = torch.full((max(nl, nd) // 8 + 16,), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((N * 3 + 4,), -7.0, dtype=torch.float64, device=dev)

    def lp(K=2, n=N, p0=a0, p1=a1, pw=aw, c=Cs, h=H, wd=W, wsp=None, nb=nl, o=None):
        return L.ssg_lpips_layers(K, n, p0.ctypes.data if p0 is not None else None, p1.ctypes.data, pw.ctypes.data,
                                  c.ctypes.data, h.ctypes.data, wd.ctypes.data, ws.data_ptr() if wsp is None else wsp, nb,
                                  out.data_ptr() if o is None else o, st)

    def ds(K=2, n=N, p0=a0, p1=a1, c=Cs, h=H, wd=W, pa=None, wsp=None, nb=nd, o=None):
        return L.ssg_dists_score(K, n, p0.ctypes.data, p1.ctypes.data if p1 is not None else None, c.ctypes.data,
                                 h.ctypes.data, wd.ctypes.data, al.data_ptr() if pa is None else pa, be.data_ptr(),
                                 ws.data_ptr() if wsp is None else wsp, nb, out.data_ptr() if o is None else o, st)

    zero = address_array([f0[0].data_ptr(), 0])
    odd = address_array([f0[0].data_ptr() + 2, f0[1].data_ptr()])
    many = _ints([1] * 17)
    for call in (lp, ds):
        assert call(K=0) == E["SSG_E_BADARG"] and call(K=17, c=many, h=many, wd=many) == E["SSG_E_BADARG"]
        assert call(n=0) == E["SSG_E_BADARG"]
        assert call(c=_ints([3, 0])) == E["SSG_E_BADARG"] and call(h=_ints([0, 1])) == E["SSG_E_BADARG"]
        assert call(wd=_ints([5, -1])) == E["SSG_E_BADARG"]
        assert call(p0=zero) == E["SSG_E_BADARG"]
        assert call(wsp=0) == E["SSG_E_BADARG"] and call(o=0) == E["SSG_E_BADARG"]
        assert call(nb=(nl if call is lp else nd) - 1) == E["SSG_E_WORKSPACE"]
        assert call(p0=odd) == E["SSG_E_ALIGN"]
        assert call(wsp=ws.data_ptr() + 4) == E["SSG_E_ALIGN"] and call(o=out.data_ptr() + 4) == E["SSG_E_ALIGN"]
        assert call(h=_ints([1 << 20, 1]), wd=_ints([1 << 20, 1])) == E["SSG_E_TOOLARGE"]
    assert lp(p0=None) == E["SSG_E_BADARG"] and ds(p1=None) == E["SSG_E_BADARG"]
    assert ds(pa=al.data_ptr() + 2) == E["SSG_E_ALIGN"]
    assert L.ssg_lpips_workspace_bytes(0, N, Cs.ctypes.data, H.ctypes.data, W.ctypes.data) == 0
    assert L.ssg_dists_workspace_bytes(2, N, Cs.ctypes.data, H.ctypes.data, _ints([5, 0]).ctypes.data) == 0
    torch.cuda.synchronize()
    assert bool((ws == -7.0).all()) and bool((out == -7.0).all())          # every refusal left the outputs untouched
    # the sentinels behind what each call may write
    assert lp() == 0
    torch.cuda.synchronize()
    assert bool((ws[nl // 8:] == -7.0).all()) and bool((out[N * 3:] == -7.0).all()) and bool((out[:N * 3] != -7.0).all())
    ws.fill_(-7.0), out.fill_(-7.0)
    assert ds() == 0
    torch.cuda.synchronize()
    assert bool((ws[nd // 8:] == -7.0).all()) and bool((out[N * 3:] == -7.0).all()) and bool((out[:N * 3] != -7.0).all())
    assert bool((ws[:nd // 8] != -7.0).all())


def test_wrappers_refuse_what_the_kernels_cannot_read_whatever_the_flag(dev):
    """half, fp64, CPU and mixed-device tensors never reach the C ABI, with set_native_criteria on or off"""
    from ssl_amd import metrics_feat as MF
    from ssl_amd.losses import set_native_criteria
    good = lambda: torch.rand(2, 4, 3, 3, device=dev)
    w, al = torch.rand(4, device=dev), torch.rand(4, device=dev)
    bad = {"half": good().half(), "bf16": good().bfloat16(), "fp64": good().double(), "cpu": good().cpu(), "list": [1.0]}
    if torch.cuda.device_count() > 1:
        bad["other gpu"] = good().to("cuda:1")
    for flag in (True, False):
        prev = set_native_criteria(flag)
        try:
            for name, t in bad.items():
                for args in (([t], [good()], [w]), ([good()], [t], [w])):
                    with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                        MF.lpips_layers(*args)
                for args in (([t], [good()], al, al), ([good()], [t], al, al)):
                    with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                        MF.dists_score(*args)
            for t in (w.half(), w.double(), w.cpu()):
                with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                    MF.lpips_layers([good()], [good()], [t])
                with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                    MF.dists_score([good()], [good()], t, al)
                with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                    MF.dists_score([good()], [good()], al, t)
            # and what they can read is served either way: the wrappers ARE the kernels
            assert MF.lpips_layers([good()], [good()], [w]).shape == (2, 2)
            assert MF.dists_score([good()], [good()], al, al).shape == (2, 3)
        finally:
            set_native_criteria(prev)


# ---------------------------------------------------------------------------------------------- LDS poison ---
def poison_cases():
    """every kernel output of the LPIPS and DISTS cases, the second grid trip included (the one case in which a
    workgroup writes `sh` and the fold's LDS words again, trip after trip), for test_gpu_featmetric_poison.py"""
    from ssl_amd import metrics_feat as MF
    dev = torch.device("cuda:0")
    out = []
    for name in LPIPS_NAMES:
        _, (f0, f1, w), _ = lpips_set(name, dev)
        out.append(MF.lpips_layers(f0, f1, w))
    for name in DISTS_NAMES:
        _, (x, y, a, b), _ = dists_set(name, dev)
        out.append(MF.dists_score(x, y, a, b))
    return out


# ---------------------------------------------------------------------------------------------- end to end ---
@pytest.fixture(scope="module")
def nets(dev):
    from ssl_amd import metrics_feat as MF
    return (MF.LPIPS('alex', C.lpips_state('alex')[0]).to(dev), MF.LPIPS('vgg', C.lpips_state('vgg')[0]).to(dev),
            MF.DISTS(C.dists_state()[0]).to(dev))


class _fixed_features:
    """Inside the block `net.features(x)` returns the maps computed once for x (looked up by address): the library's
    convolutions need not give the same bits from pass to pass, and a bound on the criterion holds on equal features."""

    def __init__(self, net, *inputs):
        self.net = net
        with torch.no_grad():
            self.table = {x.data_ptr(): net.features(x) for x in inputs}

    def __enter__(self):
        self.net.features = lambda x: self.table[x.data_ptr()]
        return [self.table[k] for k in self.table]

    def __exit__(self, *exc):
        del self.net.features
        return False


def _both_paths(call):
    """(native, torch lines) of one module call.  The first must go through exactly one call of a kernel wrapper and
    the second through none: a silent fall-back of the hot path to the torch lines fails here."""
    from ssl_amd import metrics_feat as MF
    from ssl_amd.losses import set_native_criteria
    calls, saved = [], (MF.lpips_layers, MF.dists_score)

    def spy(fn):
        def wrapped(*args):
            calls.append(fn.__name__)
            return fn(*args)
        return wrapped

    MF.lpips_layers, MF.dists_score = spy(saved[0]), spy(saved[1])
    try:
        native = call()
        assert len(calls) == 1, calls
        prev = set_native_criteria(False)
        try:
            lines = call()
        finally:
            set_native_criteria(prev)
        assert len(calls) == 1, calls
        return native, lines
    finally:
        MF.lpips_layers, MF.dists_score = saved


@pytest.mark.parametrize("shape", C.IMAGE_SHAPES)
def test_modules_native_against_torch_lines(dev, nets, shape):
    sr, gt = (t.to(dev) for t in C.images(shape))
    alex, vgg, dists = nets
    a, b = sr * 2 - 1, gt * 2 - 1
    with torch.no_grad():
        for net in (alex, vgg):
            with _fixed_features(net, a, b) as (f0, f1):
                ref = R.lpips(f0, f1, list(net.lins))
                native, lines = _both_paths(lambda: net(a, b))
            assert native.shape == lines.shape == (shape[0], 1, 1, 1) and native.dtype == lines.dtype == torch.float32
            # the native value is cast to fp32 once: one rounding more than the kernel's bound
            nb = ref.value_bound + R.U * np.abs(ref.value)
            sn, sl = R.share(native.reshape(-1), ref.value, nb), R.share(lines.reshape(-1), ref.value, ref.torch_value_bound)
            print(f"lpips {net.pnet_type} {shape}: native share {sn:.3g}, torch lines' share of the wider bound {sl:.3g}")
            assert sn <= 1.0 and sl <= 1.0
            # and the whole call, both network passes included, either way
            native, lines = _both_paths(lambda: net(sr, gt, normalize=True))
            sw = R.share(native.reshape(-1), lines.reshape(-1).double(), ref.torch_value_bound + nb)
            print(f"      whole call, native against torch lines: share of the wider bound {sw:.3g}")
            assert sw <= 1.0
        with _fixed_features(dists, gt, sr) as (f0, f1):
            ref = R.dists(f0, f1, dists.alpha, dists.beta)
            native, lines = _both_paths(lambda: dists(gt, sr))
        assert native.shape == lines.shape == (shape[0],)
        nb = ref.score_bound + R.U * np.abs(ref.score)
        sn, sl = R.share(native, ref.score, nb), R.share(lines, ref.score, ref.torch_score_bound)
        print(f"dists {shape}: native share {sn:.3g}, torch lines' share of the wider bound {sl:.3g}")
        assert sn <= 1.0 and sl <= 1.0
        again = dists.features(gt)
        print("      features of a second pass differ from the first by at most",
              max(float((p - q).abs().max()) for p, q in zip(again, f0)))
        native, lines = _both_paths(lambda: dists(gt, sr))
        sw = R.share(native, lines.double(), ref.torch_score_bound + nb)
        print(f"      whole call, native against torch lines: share of the wider bound {sw:.3g}")
        assert sw <= 1.0
    x = sr.clone().requires_grad_(True)                  # an input that requires grad takes the torch lines
    assert alex(x, gt, normalize=True).requires_grad and dists(gt, x).requires_grad


def test_l2pooling_is_finite_on_a_large_map(dev):
    """The library's depthwise convolution of the squares returns small negative values on large maps, and the package's
    own (out + 1e-12).sqrt() is NaN there (found at the validation shape, 64 x 2040 x 1356; this size shows it too):
    L2pooling clamps at 0 and equals the package's line wherever that line is a number."""
    from ssl_amd import metrics_feat as MF
    pool = MF.L2pooling(channels=64).to(dev)
    x = torch.relu(torch.randn(1, 64, 512, 1356, device=dev, generator=torch.Generator(device=dev).manual_seed(3)))
    with torch.no_grad():
        got = pool(x)
        conv = torch.nn.functional.conv2d(x ** 2, pool.filter, stride=2, padding=1, groups=64)
        line = (conv + 1e-12).sqrt()
    print(f"l2pooling: the convolution's minimum {float(conv.min()):.3g}, NaN in the package's line {int(torch.isnan(line).sum())}")
    assert got.shape == (1, 64, 256, 678) and bool(torch.isfinite(got).all())
    ok = ~torch.isnan(line)
    # (two passes of the convolution need not give the same bits; its absolute error is of the size of its negative
    # values, 1e-6, so near 0 the roots may differ by sqrt(2e-6))
    assert torch.allclose(got[ok], line[ok], rtol=1e-5, atol=1.5e-3)
    assert float(got[~ok].abs().max() if bool((~ok).any()) else 0.0) <= 1.5e-3


def test_calculate_metric_on_uint8_bgr_arrays_and_the_val_block(dev):
    from ssl_amd import metrics
    aw, dw = C.lpips_state('alex')[0], C.dists_state()[0]
    gen = np.random.default_rng(5)
    gt = gen.integers(0, 256, (45, 67, 3), dtype=np.uint8)
    sr = np.clip(gt.astype(np.int32) + gen.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
    block = C.val_metrics_block()
    block["lpips"]["lpips_weights"], block["dists"]["dists_weights"] = aw, dw
    from ssl_amd import metrics_feat as MF
    got = {k: metrics.calculate_metric(dict(img=sr, img2=gt), opt) for k, opt in block.items()}
    built = len(MF._models)
    again = {k: metrics.calculate_metric(dict(img=sr, img2=gt), opt) for k, opt in block.items()}
    assert len(MF._models) == built                            # one network per weights source, not one per call
    # (two passes of the library's convolutions need not give the same bits, so neither do two calls: the tolerance of
    # the comparison below)
    assert all(abs(again[k] - got[k]) <= 2e-5 * max(1.0, abs(got[k])) for k in got), (again, got)
    assert all(np.isfinite(v) for v in got.values()) and got["lpips"] > 0 and 0 < got["dists"] < 1
    # the same images as a model's tensors through the averager: tensor2img's quantisation gives the arrays back
    to_t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, :, ::-1].transpose(2, 0, 1))).float().div(255)[None].to(dev)
    avg = metrics.MetricAverager()
    avg.add_all(to_t(sr), to_t(gt), block)
    res = avg.result()
    assert set(res) == set(block)
    for k in block:
        assert abs(res[k] - got[k]) <= 2e-5 * max(1.0, abs(got[k])), (k, res[k], got[k])
    pair = metrics.lpips_dists(to_t(sr), to_t(gt), crop_border=4, lpips_weights=aw, dists_weights=dw)
    assert pair.shape == (1, 2) and pair.dtype == torch.float64 and pair.is_cuda
    assert metrics.calculate_metric(dict(img=gt, img2=gt), block["lpips"]) == 0.0
