"""LDL's artifact map and loss on the MI355X (ssl_amd/csrc/ssg_ldl.hip): against the reference's own outputs
(tests/golden/f18_ldl_artifact.npz) and against the torch restatement of test_cpu_ldl.py at the callers' sizes, on
border-heavy shapes, for C = 1 and 4, the map's backward for any upstream gradient, reproducibility and the API."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_cpu_ldl import restated_loss, restated_map

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(shape, seed, noise=0.08, ema_noise=0.06):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    g = torch.rand(shape, generator=gen)
    o = (g + noise * torch.randn(shape, generator=gen)).clamp(0, 1)
    e = (g + ema_noise * torch.randn(shape, generator=gen)).clamp(0, 1)
    return o.to(DEV), g.to(DEV), e.to(DEV)


def _hip(o, g, e, k, lam=1.0, reduction='mean'):
    from ssl_amd.losses import ArtifactLoss
    x = o.detach().clone().requires_grad_(True)
    loss = ArtifactLoss(loss_weight=lam, ksize=k, reduction=reduction)(x, g, e)
    loss.backward()
    return loss.detach(), x.grad


def test_hip_against_the_reference_fixture(golden):
    from ssl_amd.losses import get_artifact_map, get_local_weights, get_refined_artifact_map
    f = golden("f18_ldl_artifact")
    for i in range(int(f["n_cases"])):
        c = lambda key: f[f"c{i}_{key}"]
        o, g, e = (torch.from_numpy(c(key)).to(DEV) for key in ("o", "g", "e"))
        k, lam = int(c("k")), float(c("lam"))
        w = get_refined_artifact_map(g, o, e, k).cpu().numpy()
        w_ref = c("w")
        assert np.abs(w - w_ref).max() <= 1e-5 * max(np.abs(w_ref).max(), 1e-30), i
        assert np.array_equal(w == 0, w_ref == 0), i                      # the mask decisions (and V = 0 images)
        assert (w[c("mask")] == 0).all() and (w[c("ties") & (w_ref > 0)] > 0).all(), i
        wp = get_artifact_map(g, o, k).cpu().numpy()
        assert np.abs(wp - c("w_plain")).max() <= 1e-5 * max(np.abs(c("w_plain")).max(), 1e-30), i
        lw = get_local_weights(torch.from_numpy(c("r")).to(DEV), k).cpu().numpy()
        assert np.abs(lw - c("local")).max() <= 1e-5 * np.abs(c("local")).max(), i
        loss, grad = _hip(o, g, e, k, lam)
        assert abs(float(loss) - float(c("loss"))) <= 1e-5 * abs(float(c("loss"))), i
        gr, gref = grad.cpu().numpy(), c("grad")
        assert np.array_equal(np.isnan(gr), np.isnan(gref)), i           # output == GT: that image's gradient is NaN
        fin = ~np.isnan(gref)
        assert np.abs(gr[fin] - gref[fin]).max() <= 1e-5 * np.abs(gref[fin]).max(), i


def _compare_to_restatement(o, g, e, k, lam=1.0, reduction='mean', tol=1e-5):
    """HIP loss and gradient against the restatement on the GPU.  Where fp32 cannot decide, the two may differ: a mask
    decision with r within rounding of r_e, or a product pair w*o, w*g that rounds to one value in one evaluation of w
    and not in the other (a sign tie of the L1).  Such pixels are counted and bounded, and their windows (their
    weight feeds the gradient of every pixel within k/2) are left out of the element-wise comparison."""
    loss, grad = _hip(o, g, e, k, lam, reduction)
    rl, rg, rw = restated_loss(o, g, e, k, lam, reduction)
    from ssl_amd.losses import get_refined_artifact_map
    w = get_refined_artifact_map(g, o, e, k) if e is not None else None
    n_pix = o.shape[0] * o.shape[2] * o.shape[3]
    odd = torch.zeros_like(rw, dtype=torch.bool)
    if w is not None:
        flips = (w == 0) != (rw == 0)
        odd |= flips
        assert int(flips.sum()) <= max(2, n_pix // 100000), int(flips.sum())
    d_ref = rw * o - rw * g
    ties = ((d_ref.abs() <= 4e-7 * (rw * o).abs()) & (o != g) & (rw > 0)).any(1, keepdim=True)
    odd |= ties
    assert int(ties.sum()) <= max(4, n_pix // 20000), int(ties.sum())
    near = F.max_pool2d(odd.float(), k, 1, k // 2) > 0
    keep = (~near).expand_as(grad)
    assert abs(float(loss) - float(rl)) <= tol * abs(float(rl))
    scale = float(rg.abs().max())
    err = float((grad - rg).abs()[keep].max())
    assert err <= tol * scale, (err, scale)
    return loss, grad


@pytest.mark.parametrize("shape", [(64, 3, 128, 128), (12, 3, 256, 256)])
def test_hip_against_restatement_at_the_callers_sizes(shape):
    o, g, e = _inputs(shape, 7)
    _compare_to_restatement(o, g, e, 7)


@pytest.mark.parametrize("H,W", [(4, 4), (4, 9), (5, 7), (6, 4), (7, 9), (8, 5), (9, 6), (9, 9)])
def test_border_heavy_shapes(H, W):
    """Images where most pixels lie within k/2 of an edge: one source pixel sits at two (or three) taps of the same
    window, which a neighbour scatter would count once."""
    o, g, e = _inputs((3, 3, H, W), 100 * H + W)
    _compare_to_restatement(o, g, e, 7)
    if min(H, W) > 4:
        _compare_to_restatement(o, g, e, 9)
    _compare_to_restatement(o, g, None, 3)


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("k", [3, 5, 7, 11, 15])
def test_channels_and_window_sizes(C, k):
    o, g, e = _inputs((2, C, 37, 45), 31 * C + k)
    _compare_to_restatement(o, g, e, k)
    _compare_to_restatement(o, g, e, k, lam=0.25, reduction='sum')


def test_map_backward_with_any_upstream_gradient():
    from ssl_amd.losses import get_artifact_map, get_local_weights, get_refined_artifact_map
    for shape, k in (((2, 3, 24, 30), 7), ((1, 4, 5, 9), 7), ((3, 1, 17, 12), 5), ((2, 3, 40, 33), 13)):
        o, g, e = _inputs(shape, sum(shape) + k)
        up = torch.randn((shape[0], 1) + shape[2:], device=DEV)
        for ema in (e, None):
            x = o.clone().requires_grad_(True)
            (get_refined_artifact_map(g, x, ema, k) if ema is not None else get_artifact_map(g, x, k)).backward(up)
            y = o.clone().requires_grad_(True)
            w, _ = restated_map(y, g, ema, k)
            w.backward(up)
            assert torch.allclose(x.grad, y.grad, rtol=0, atol=1e-5 * float(y.grad.abs().max())), (shape, k)
        # get_local_weights alone: any residual (negative values too), its own backward
        r = torch.randn((shape[0], 2) + shape[2:], device=DEV)
        x = r.clone().requires_grad_(True)
        v = get_local_weights(x, k)
        up2 = torch.randn_like(v)
        v.backward(up2)
        y = r.clone().requires_grad_(True)
        pad = k // 2
        vr = torch.var(F.pad(y, [pad] * 4, mode='reflect').unfold(2, k, 1).unfold(3, k, 1), dim=(-1, -2), unbiased=True)
        vr.backward(up2)
        assert torch.allclose(v, vr, rtol=0, atol=1e-5 * float(vr.detach().abs().max()))
        assert torch.allclose(x.grad, y.grad, rtol=0, atol=1e-5 * float(y.grad.abs().max()))


def test_gradient_is_bit_reproducible():
    o, g, e = _inputs((16, 3, 96, 80), 3)
    runs = [_hip(o, g, e, 7) for _ in range(3)]
    for loss, grad in runs[1:]:
        assert torch.equal(grad, runs[0][1]) and torch.equal(loss, runs[0][0])


def test_none_reduction_and_half_inputs():
    from ssl_amd.losses import ArtifactLoss
    o, g, e = _inputs((2, 3, 20, 24), 11)
    x = o.clone().requires_grad_(True)
    out = ArtifactLoss(loss_weight=2.0, reduction='none')(x, g, e)
    assert out.shape == o.shape
    y = o.clone().requires_grad_(True)
    w, _ = restated_map(y, g, e, 7)
    ref = 2.0 * torch.abs(w * y - w * g)
    assert torch.allclose(out, ref, rtol=0, atol=1e-5 * float(ref.detach().abs().max()))
    up = torch.rand_like(out)
    out.backward(up)
    ref.backward(up)
    assert torch.allclose(x.grad, y.grad, rtol=0, atol=1e-5 * float(y.grad.abs().max()))
    # the 'mean' of 'none' is the fused 'mean'
    fused = ArtifactLoss(loss_weight=2.0)(o, g, e)
    assert abs(float(fused) - float(out.mean())) <= 1e-5 * float(fused)
    # fp16 / bf16 are computed in fp32, the gradient comes back in the input's dtype
    for dt in (torch.float16, torch.bfloat16):
        h = o.to(dt).requires_grad_(True)
        ArtifactLoss()(h, g.to(dt), e.to(dt)).backward()
        assert h.grad.dtype == dt and torch.isfinite(h.grad.float()).all()


def test_gt_or_ema_requiring_grad_raises():
    from ssl_amd.losses import ArtifactLoss, get_refined_artifact_map
    o, g, e = _inputs((1, 3, 16, 16), 5)
    with pytest.raises(ValueError, match="gt"):
        ArtifactLoss()(o.clone().requires_grad_(True), g.clone().requires_grad_(True), e)
    with pytest.raises(ValueError, match="ema"):
        get_refined_artifact_map(g, o.clone().requires_grad_(True), e.clone().requires_grad_(True), 7)
    with pytest.raises(RuntimeError, match="GPU"):
        ArtifactLoss()(o.cpu(), g.cpu())
    with pytest.raises(RuntimeError, match="reflect|image side"):
        ArtifactLoss()(o[..., :3, :], g[..., :3, :])
