"""LDL's artifact map and loss without a GPU: the new symbols are exported, the C ABI refuses bad arguments before it
launches anything, and the torch restatement of the contract (ssl_amd/csrc/ssg_ldl.hip, header comment) that the GPU
tests use at sizes no fixture covers matches the reference's own outputs (tests/golden/f18_ldl_artifact.npz)."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

LDL_SYMBOLS = ("ssg_ldl_workspace_bytes", "ssg_artifact_map", "ssg_artifact_map_backward", "ssg_ldl_loss",
               "ssg_local_variance")


def restated_map(o, g, e, k):
    """The contract in torch: r = sum_c |g - o|, P = var_unbiased(r)^(1/5) per image, V = unbiased variance of the
    k x k reflect-padded window, w = P V, 0 where r < r_e.  Returns (w, V of r)."""
    r = torch.sum(torch.abs(g - o), 1, keepdim=True)
    P = torch.var(r, dim=(1, 2, 3), unbiased=True, keepdim=True) ** (1 / 5)
    pad = (k - 1) // 2
    win = F.pad(r, [pad, pad, pad, pad], mode='reflect').unfold(2, k, 1).unfold(3, k, 1)
    V = torch.var(win, dim=(-1, -2), unbiased=True)
    w = P * V
    if e is not None:
        r_e = torch.sum(torch.abs(g - e), 1, keepdim=True)
        w = torch.where(r < r_e, torch.zeros_like(w), w)
    return w, V


def restated_loss(o, g, e, k, lam=1.0, reduction='mean'):
    """(loss, d loss / d o, w) of L1Loss(w * o, w * g) through the restated map, by torch.autograd."""
    x = o.detach().clone().requires_grad_(True)
    w, _ = restated_map(x, g, e, k)
    d = torch.abs(w * x - w * g)
    loss = lam * (d.mean() if reduction == 'mean' else d.sum())
    loss.backward()
    return loss.detach(), x.grad, w.detach()


def test_ldl_symbols_are_exported():
    from ssl_amd import _lib
    import ssl_amd.losses as losses
    from ssl_amd.losses import loss_util
    _lib.build()
    L = ctypes.CDLL(_lib.SO_PATH)
    hdr = open(_lib.HEADER).read()
    for name in LDL_SYMBOLS:
        assert hasattr(L, name) and name in _lib.PROTOTYPES and f"{name}(" in hdr, name
    for name in ("get_local_weights", "get_artifact_map", "get_refined_artifact_map"):
        assert callable(getattr(loss_util, name)) and getattr(losses, name) is getattr(loss_util, name)
    assert losses.ArtifactLoss().ksize == 7 and losses.ArtifactLoss().reduction == 'mean'
    assert _lib.lib().ssg_ldl_workspace_bytes(64, 128, 128) >= 4 * 4 * 64 * 128 * 128


def test_ldl_argument_checks_need_no_gpu():
    """SSG_E_BADARG (-1) for null pointers and even / non-positive k, SSG_E_TOOLARGE (-2) for k > 15,
    SSG_E_IMAGESMALL (-4) for a side <= (k-1)/2, SSG_E_WORKSPACE (-3) for a short workspace, SSG_E_ALIGN (-5) for one
    that is not 16-byte aligned: all decided before a launch (the pointers below are never dereferenced)."""
    from ssl_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(8)
    big = 1 << 40
    amap = lambda o, k, H=16, W=16, C=3, out=one, ws=big, e=None: L.ssg_artifact_map(o, one, e, 2, C, H, W, k, out, one,
                                                                                     ws, None)
    for k in (6, 0, -3, 1, 2):
        assert amap(one, k) == -1, k
    assert amap(None, 7) == -1 and amap(one, 7, out=None) == -1 and amap(one, 7, C=0) == -1
    assert amap(one, 17) == -2 and amap(one, 31) == -2
    assert amap(one, 7, H=3) == -4 and amap(one, 7, W=3) == -4 and amap(one, 9, H=4) == -4 and amap(one, 3, W=1) == -4
    assert amap(one, 7, ws=16) == -3 and amap(one, 7, H=4, W=5, ws=L.ssg_ldl_workspace_bytes(2, 4, 5) - 1) == -3
    assert L.ssg_artifact_map(one, one, one, 0, 3, 16, 16, 7, one, one, big, None) == -1      # B = 0
    assert L.ssg_artifact_map_backward(one, one, None, None, 2, 3, 16, 16, 7, one, one, big, None) == -1
    assert L.ssg_artifact_map_backward(one, one, None, one, 2, 3, 16, 16, 8, one, one, big, None) == -1
    assert L.ssg_artifact_map_backward(one, one, None, one, 2, 3, 16, 16, 19, one, one, big, None) == -2
    assert L.ssg_artifact_map_backward(one, one, None, one, 2, 3, 16, 16, 7, one, one, 0, None) == -3
    assert L.ssg_ldl_loss(one, one, one, 2, 3, 16, 16, 7, 1.0, 1, None, one, one, big, None) == -1
    assert L.ssg_ldl_loss(one, None, one, 2, 3, 16, 16, 7, 1.0, 1, one, one, one, big, None) == -1
    assert L.ssg_ldl_loss(one, one, one, 2, 3, 16, 16, 4, 1.0, 1, one, one, one, big, None) == -1
    assert L.ssg_ldl_loss(one, one, one, 2, 3, 16, 16, 16, 1.0, 1, one, one, one, big, None) == -1
    assert L.ssg_ldl_loss(one, one, one, 2, 3, 16, 16, 17, 1.0, 1, one, one, one, big, None) == -2
    assert L.ssg_ldl_loss(one, one, one, 2, 3, 16, 7, 15, 1.0, 1, one, one, one, big, None) == -4
    assert L.ssg_ldl_loss(one, one, one, 2, 3, 16, 16, 7, 1.0, 1, one, one, one, 100, None) == -3
    assert L.ssg_local_variance(one, 2, 16, 16, 7, None, None, None, one, big, None) == -1    # nothing to compute
    assert L.ssg_local_variance(one, 2, 16, 16, 7, one, one, None, one, big, None) == -1      # grad_v without grad_r
    assert L.ssg_local_variance(one, 2, 16, 16, 5, one, None, None, one, 8, None) == -3
    assert L.ssg_ldl_workspace_bytes(0, 16, 16) == 0
    assert amap(one, 7) == -5 and amap(one, 7, e=one) == -5    # a workspace off 16-byte alignment: SSG_E_ALIGN


def test_restatement_matches_the_reference_fixture(golden):
    """The restatement above against the reference's own get_local_weights / get_artifact_map /
    get_refined_artifact_map, loss and autograd gradient: to 1e-6, NaN pattern included (output == GT)."""
    f = golden("f18_ldl_artifact")
    saw_nan = False
    for i in range(int(f["n_cases"])):
        c = lambda key: f[f"c{i}_{key}"]
        o, g, e = (torch.from_numpy(c(key)) for key in ("o", "g", "e"))
        k, lam = int(c("k")), float(c("lam"))
        loss, grad, w = restated_loss(o, g, e, k, lam)
        w_plain, _ = restated_map(o, g, None, k)
        r = torch.sum(torch.abs(g - o), 1, keepdim=True)
        _, V = restated_map(o, g, None, k)
        for mine, ref in ((w, c("w")), (w_plain, c("w_plain")), (V, c("local")), (r, c("r"))):
            assert mine.shape == ref.shape
            assert np.abs(mine.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1e-30), i
        assert abs(float(loss) - float(c("loss"))) <= 1e-6 * abs(float(c("loss"))), i
        gr, gref = grad.numpy(), c("grad")
        assert np.array_equal(np.isnan(gr), np.isnan(gref)), i
        fin = ~np.isnan(gref)
        saw_nan |= bool((~fin).any())
        assert np.abs(gr[fin] - gref[fin]).max() <= 1e-6 * np.abs(gref[fin]).max(), i
    assert saw_nan      # the constant-residual image is in the fixture and its gradient is NaN in the reference


def test_reference64_matches_the_reference_fixture(golden):
    """The fp64 yardstick of the GPU tests (ldl_reference.py) against the same outputs of the reference, to the same
    1e-6 and NaN pattern as the fp32 restatement above; its fp32-decided residual and mask equal the reference's
    bit for bit."""
    from ldl_reference import local_variance64, mask32, reference64, residual32
    f = golden("f18_ldl_artifact")
    saw_nan = False
    for i in range(int(f["n_cases"])):
        c = lambda key: f[f"c{i}_{key}"]
        o, g, e = (torch.from_numpy(c(key)) for key in ("o", "g", "e"))
        k, lam = int(c("k")), float(c("lam"))
        loss, grad, w, undecided = reference64(o, g, e, k, lam)
        _, _, w_plain, _ = reference64(o, g, None, k, lam)
        r = residual32(o, g)
        assert r.dtype == np.float32 and np.array_equal(r, c("r")), i
        assert np.array_equal(mask32(o, g, e).numpy(), c("mask")), i
        assert np.array_equal((w == 0).numpy() & (c("w_plain") > 0), c("mask") & (c("w_plain") > 0)), i
        V, _ = local_variance64(torch.from_numpy(c("r")), k)
        for mine, ref in ((w, c("w")), (w_plain, c("w_plain")), (V, c("local"))):
            assert mine.shape == ref.shape and mine.dtype == torch.float64
            assert np.abs(mine.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1e-30), i
        assert abs(float(loss) - float(c("loss"))) <= 1e-6 * abs(float(c("loss"))), i
        gr, gref = grad.numpy(), c("grad")
        assert np.array_equal(np.isnan(gr), np.isnan(gref)), i
        fin = ~np.isnan(gref)
        saw_nan |= bool((~fin).any())
        assert np.abs(gr[fin] - gref[fin]).max() <= 1e-6 * np.abs(gref[fin]).max(), i
        assert undecided.shape == c("mask").shape and undecided.dtype == torch.bool
        # the map's backward for an upstream gradient and the local variance's: against the fp32 restatement's autograd
        up = torch.randn(c("w").shape, generator=torch.Generator().manual_seed(i))
        _, gmap, _, _ = reference64(o, g, e, k, upstream=up)
        y = o.clone().requires_grad_(True)
        restated_map(y, g, e, k)[0].backward(up)
        fin = ~torch.isnan(y.grad)
        assert torch.equal(torch.isnan(gmap), ~fin), i
        if fin.any():
            assert float((gmap - y.grad)[fin].abs().max()) <= 1e-5 * float(y.grad[fin].abs().max()), i
    assert saw_nan


def test_fixture_covers_the_traps(golden):
    """The fixture holds what the GPU tests lean on: every k of 3, 7, 9; the 4 x 5 image; pixels with r == r_e exactly
    (not masked: the test is strict) and masked pixels; an image whose output equals its GT.  Masked pixels with
    r = 0 exist, but only inside that image (r = 0 < r_e everywhere, gradient all NaN): a masked r = 0 next to finite
    gradients is covered by kind `zeros` of test_gpu_ldl.py alone."""
    f = golden("f18_ldl_artifact")
    n = int(f["n_cases"])
    assert {int(f[f"c{i}_k"]) for i in range(n)} >= {3, 7, 9}
    assert any(f[f"c{i}_o"].shape[-2:] == (4, 5) for i in range(n))
    ties = sum(int(f[f"c{i}_ties"].sum()) for i in range(n))
    assert ties > 10 and all(not (f[f"c{i}_ties"] & f[f"c{i}_mask"]).any() for i in range(n))
    assert any(f[f"c{i}_mask"].any() for i in range(n))
    assert any((f[f"c{i}_o"] == f[f"c{i}_g"]).reshape(f[f"c{i}_o"].shape[0], -1).all(1).any() for i in range(n))
    assert any(((f[f"c{i}_r"] == 0) & f[f"c{i}_mask"]).any() for i in range(n))
