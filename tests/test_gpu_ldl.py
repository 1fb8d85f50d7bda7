"""LDL's artifact map and loss on the MI355X (ssl_amd/csrc/ssg_ldl.hip): against the reference's own outputs
(tests/golden/f18_ldl_artifact.npz), against the torch restatement of test_cpu_ldl.py and against the fp64 reference of
ldl_reference.py (which test_cpu_ldl.py pins to the same fixture) at the callers' sizes, on images with more partial
sums than one pass of the folding loops, on minimal and tile-edge sides for every k, in six input regimes, for C = 1
and 4, the map's backward for any upstream gradient, the callers' two lines as written, side streams and graph replay
through the C ABI, reproducibility and the API.

Bounds: 1e-5 of max|reference| for w, the loss (relative) and the gradient: the project's bar of every parity test,
here against fp64.  Every fp64 comparison prints one `LDL64` line (pytest -s) with the measured ratios;
profiles/ldl_fp64_parity.txt holds the table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ldl_reference import local_variance64, reference64
from raw_loss import RawLoss, replays_as_hip_graph, side_stream_equals_default_stream
from test_cpu_ldl import restated_loss, restated_map

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


KINDS = ("callers", "unclamped", "fine", "offset", "smooth", "zeros")
TOL = 1e-5      # of max|fp64 reference|: w, loss (relative), gradient


def _inputs_cpu(shape, seed, noise=0.08, ema_noise=0.06, kind="callers"):
    """(output, gt, ema) on the CPU, seeded.  n1, n2 standard normal:
    callers    gt rand, output clamp(gt + 0.08 n1), ema clamp(gt + 0.06 n2): what the two callers feed
    unclamped  gt + 1.5 n1 / gt + 1.2 n2: values outside [0,1], residuals up to ~15 (early training)
    fine       gt + 1e-3 n: var(r) ~ 1e-6, tiny w, large pow(var, -0.8) (nearly converged)
    offset     gt + 0.5 + 0.03 n: mean(r) / std(r) ~ 30, the backward's r_q sum G - sum G mu cancels
    smooth     gt a bicubic upsample of a coarse random grid, residuals 3 x 3 box-filtered noise: image-like
    zeros      callers, then output = gt at a seeded 5 % of pixels (all channels) and ema = gt at every second one of
               those: r = 0 exactly, masked (r_e > 0) and not masked (r = r_e = 0; every such pixel without ema)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    B, C, H, W = shape
    if kind == "smooth":
        coarse = torch.rand((B, C, H // 16 + 2, W // 16 + 2), generator=gen)
        g = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    else:
        g = torch.rand(shape, generator=gen)
    n1, n2 = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    if kind in ("callers", "zeros"):
        o, e = (g + noise * n1).clamp(0, 1), (g + ema_noise * n2).clamp(0, 1)
    elif kind == "unclamped":
        o, e = g + 1.5 * n1, g + 1.2 * n2
    elif kind == "fine":
        o, e = g + 1e-3 * n1, g + 1e-3 * n2
    elif kind == "offset":
        o, e = g + 0.5 + 0.03 * n1, g + 0.5 + 0.03 * n2
    elif kind == "smooth":
        o, e = g + 0.02 * F.avg_pool2d(n1, 3, 1, 1), g + 0.015 * F.avg_pool2d(n2, 3, 1, 1)
    else:
        raise ValueError(kind)
    if kind == "zeros":
        pick = torch.rand((B, 1, H, W), generator=gen) < 0.05
        o = torch.where(pick, g, o)
        second = torch.zeros(B * H * W, dtype=torch.bool)
        second[pick.flatten().nonzero().flatten()[::2]] = True
        e = torch.where(second.view(B, 1, H, W), g, e)
    return o.contiguous(), g.contiguous(), e.contiguous()


def _inputs(shape, seed, noise=0.08, ema_noise=0.06, kind="callers"):
    return tuple(t.to(DEV) for t in _inputs_cpu(shape, seed, noise, ema_noise, kind))


def _hip(o, g, e, k, lam=1.0, reduction='mean'):
    from ssl_amd.losses import ArtifactLoss
    x = o.detach().clone().requires_grad_(True)
    loss = ArtifactLoss(loss_weight=lam, ksize=k, reduction=reduction)(x, g, e)
    loss.backward()
    return loss.detach(), x.grad


def _ratio(got, ref):
    """max |got - ref| over max |ref| on the finite entries of ref (both on the CPU, ref fp64)."""
    fin = torch.isfinite(ref)
    if not fin.any():
        return 0.0
    return float((got.double() - ref)[fin].abs().max()) / max(float(ref[fin].abs().max()), 1e-300)


def _exclusion(undecided, k, n_pix, like):
    """The gradient elements left out of the element-wise comparison: the k x k neighbourhood of every pixel whose L1
    sign fp32 does not decide (its weight feeds the gradient of every pixel within k/2).  The caps are conditions on
    the inputs, not measurements: at most max(4, n_pix // 20000) such pixels and at most 1 % of the tensor left out."""
    near = (F.max_pool2d(undecided.float(), k, 1, k // 2) > 0).expand_as(like)
    return ~near, int(undecided.sum()), float(near.float().mean())


def _compare_to_fp64(o, g, e, k, lam=1.0, reduction='mean', label="", hip=None, local=False):
    """The HIP loss, gradient (ArtifactLoss), map (get_refined_artifact_map / get_artifact_map) and the map's backward
    for a random upstream against ldl_reference.reference64, TOL of max|reference| each; with `local`, also
    get_local_weights and its backward on the residual.  The mask is bit-defined: no pixel may differ."""
    from ssl_amd.losses import get_artifact_map, get_local_weights, get_refined_artifact_map
    loss, grad = hip if hip is not None else _hip(o, g, e, k, lam, reduction)
    oc, gc, ec = o.cpu(), g.cpu(), None if e is None else e.cpu()
    rl, rg, rw, undecided = reference64(oc, gc, ec, k, lam, reduction)
    B, C, H, W = o.shape
    n_pix = B * H * W
    x = o.detach().clone().requires_grad_(True)
    w = get_refined_artifact_map(g, x, e, k) if e is not None else get_artifact_map(g, x, k)
    up = torch.randn((B, 1, H, W), generator=torch.Generator().manual_seed(n_pix + k))
    w.backward(up.to(DEV))
    _, rgm, _, _ = reference64(oc, gc, ec, k, upstream=up)
    wc, gradc, gmapc = w.detach().cpu(), grad.cpu(), x.grad.cpu()
    flips = int(((wc == 0) != (rw == 0)).sum())
    keep, n_und, share = _exclusion(undecided, k, n_pix, rg)
    e_w, e_l = _ratio(wc, rw), abs(float(loss) - float(rl)) / max(abs(float(rl)), 1e-300)
    e_g = _ratio(torch.where(keep, gradc.double(), rg), rg)
    e_m = _ratio(gmapc, rgm)
    e_v = e_lg = 0.0
    if local:
        r = torch.sum(torch.abs(gc - oc), 1, keepdim=True)
        upl = torch.rand(r.shape, generator=torch.Generator().manual_seed(k))
        y = r.clone().to(DEV).requires_grad_(True)
        v = get_local_weights(y, k)
        v.backward(upl.to(DEV))
        rv, rlg = local_variance64(r, k, upl)
        e_v, e_lg = _ratio(v.detach().cpu(), rv), _ratio(y.grad.cpu(), rlg)
    print(f"LDL64 {label or 'case'} shape={tuple(o.shape)} k={k} ema={e is not None} {reduction} w={e_w:.2e} "
          f"loss={e_l:.2e} grad={e_g:.2e} mapgrad={e_m:.2e} localV={e_v:.2e} localgrad={e_lg:.2e} flips={flips} "
          f"undecided={n_und} excluded={100 * share:.3f}%")
    assert flips == 0, flips
    assert n_und <= max(4, n_pix // 20000) and share <= 0.01, (n_und, share)
    assert torch.equal(torch.isnan(gradc), torch.isnan(rg)) and torch.equal(torch.isnan(gmapc), torch.isnan(rgm))
    assert e_w <= TOL, e_w
    assert e_l <= TOL, e_l
    assert e_g <= TOL, e_g
    assert e_m <= TOL, e_m
    assert e_v <= TOL and e_lg <= TOL, (e_v, e_lg)
    return loss, grad


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
    _compare_to_fp64(o, g, e, k, lam, reduction, label="restated", hip=(loss, grad))
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
    for shape in ((16, 3, 96, 80), (2, 3, 520, 530)):
        o, g, e = _inputs(shape, 3)
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


# ------------------------------------------------------------------------------------- against fp64 (ldl_reference) ----
@pytest.mark.parametrize("kind", KINDS)
def test_fp64_every_kind_at_the_callers_sizes(kind):
    """(Seed 13 for the five other kinds: kind `fine` holds about seven undecided pixels in 65,536 on average, the cap is
    four; with this seed the fp64 reference alone counts two.  A condition on the inputs, met before any kernel runs.)"""
    shapes = [(64, 3, 128, 128), (12, 3, 256, 256)] if kind == "callers" else [(4, 3, 128, 128)]
    for shape in shapes:
        o, g, e = _inputs(shape, 7 if kind == "callers" else 13, kind=kind)
        _compare_to_fp64(o, g, e, 7, label=kind, local=shape[0] == 4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [3, 15])
def test_fp64_every_kind_small_and_large_window(kind, k):
    """(The seed is one for which the inputs meet the caps on undecided pixels, checked with the fp64 reference alone:
    kind `fine` puts an output within two ulp of its GT once in ~6,000 elements, and one such pixel at k = 15 takes
    7 % of this small tensor out of the comparison.)"""
    o, g, e = _inputs((2, 3, 37, 45), 200 + k, kind=kind)
    if kind == "zeros":
        r0 = (o == g).all(1)
        assert r0.any() and ((e == g).all(1) & r0).any() and ((e != g).any(1) & r0).any()
    for ema in (e, None):
        _compare_to_fp64(o, g, ema, k, label=kind)
        _compare_to_fp64(o, g, ema, k, lam=0.25, reduction='sum', label=kind)


def _partial_counts(B, H, W):
    """(nb1, ntile) per image as ssg_ldl.hip lays them out: blocks of 256 threads x 4 pixels, tiles of 32 x 16; checked
    against ssg_ldl_workspace_bytes (four fp32 planes, then 16 bytes per partial, each region rounded up to 256)."""
    from ssl_amd import _lib
    nb1, ntile = -(-(H * W) // 1024), -(-W // 32) * -(-H // 16)
    up = lambda v: (v + 255) & ~255
    assert _lib.lib().ssg_ldl_workspace_bytes(B, H, W) == 4 * up(4 * B * H * W) + up(16 * B * nb1) + up(16 * B * ntile)
    return nb1, ntile


@pytest.mark.parametrize("shape,kind,k", [((2, 3, 520, 530), "callers", 7), ((1, 3, 520, 530), "smooth", 11),
                                          ((1, 1, 1040, 300), "callers", 3)])
def test_fp64_more_partials_than_one_pass(shape, kind, k):
    """image_stats folds nb1 per-block and ntile per-tile partials 256 at a time: both loops take a second trip here
    (and, with two images, at the per-image offsets b * nb1, b * ntile)."""
    nb1, ntile = _partial_counts(shape[0], shape[2], shape[3])
    assert nb1 > 256 and ntile > 256, (nb1, ntile)
    o, g, e = _inputs(shape, 21, kind=kind)
    _compare_to_fp64(o, g, e, k, label=kind + "-large")


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11, 13, 15])
def test_fp64_minimal_sides(k):
    """Sides of k/2 + 1: one source pixel is the window's direct tap, its left reflection and its right reflection at
    once, all three terms of mult()."""
    R = k // 2
    for H, W in ((R + 1, R + 1), (R + 1, R + 4), (2 * R + 1, R + 1)):
        for C in (3, 1):
            for kind in ("callers", "unclamped"):
                o, g, e = _inputs((3, C, H, W), 10 * k + C, kind=kind)
                _compare_to_fp64(o, g, e, k, label=kind + "-minimal", local=True)


@pytest.mark.parametrize("k", [7, 15])
@pytest.mark.parametrize("H,W", [(17, 33), (16, 32), (33, 65)])
def test_fp64_tile_edges(H, W, k):
    """One-pixel last tiles and exact multiples of the 32 x 16 tile."""
    for kind in ("callers", "unclamped"):
        o, g, e = _inputs((3, 3, H, W), H + W + k, kind=kind)
        _compare_to_fp64(o, g, e, k, label=kind + "-tile-edge", local=True)


def test_fp64_constant_residual_image_inside_a_batch():
    """Image 1 of three has output == GT: its whole gradient is NaN (0 * inf in the pow backward, as the reference), the
    other two images hold no NaN and match, and so does the loss -- on images of several tiles."""
    o, g, e = _inputs((3, 3, 40, 70), 77)
    o[1] = g[1]
    for ema in (e, None):
        loss, grad = _compare_to_fp64(o, g, ema, 7, label="constant-image")
        assert torch.isnan(grad[1]).all() and torch.isfinite(grad[0]).all() and torch.isfinite(grad[2]).all()
        assert torch.isfinite(loss)


@pytest.mark.parametrize("layout", ["contiguous", "channels_last", "slice"])
def test_callers_two_lines_as_written(layout):
    """ldlssl_model.py:220-224 / realesrgan_model.py:222-226, unchanged, on this package's get_refined_artifact_map and
    L1Loss: the fused ArtifactLoss to 1e-6, the fp64 reference to TOL."""
    from ssl_amd.losses import L1Loss, get_refined_artifact_map
    o, gt, output_ema = _inputs((4, 3, 64, 96), 5)
    if layout == "channels_last":
        base = o.contiguous(memory_format=torch.channels_last)
    elif layout == "slice":
        wide = torch.zeros((4, 3, 64, 200), device=DEV)
        wide[..., 3:195:2] = o
        base = wide[..., 3:195:2]
        assert not base.is_contiguous()
    else:
        base = o
    assert torch.equal(base, o)
    if layout == "slice":
        leaf = wide.clone().requires_grad_(True)
        output = leaf[..., 3:195:2]
    else:
        output = base.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    assert output.stride() == base.stride()
    cri = L1Loss(loss_weight=1.0, reduction='mean')
    pixel_weight = get_refined_artifact_map(gt, output, output_ema, 7)
    l = cri(torch.mul(pixel_weight, output), torch.mul(pixel_weight, gt))
    l.backward()
    got = leaf.grad[..., 3:195:2] if layout == "slice" else output.grad
    loss, grad = _hip(o, gt, output_ema, 7)
    scale = float(grad.abs().max())
    assert abs(float(l.detach()) - float(loss)) <= 1e-6 * abs(float(loss))
    assert float((got - grad).abs().max()) <= 1e-6 * scale
    _compare_to_fp64(o, gt, output_ema, 7, label="two-lines-" + layout, hip=(l.detach(), got.contiguous()))


@pytest.mark.parametrize("shape,k", [((2, 2, 24, 30), 7), ((1, 1, 40, 44), 13)])
@pytest.mark.parametrize("mean", [1.0, 0.0])
def test_local_weights_on_a_residual_with_a_mean(shape, k, mean):
    """get_local_weights alone: residual = 1 + 0.1 randn (the gather's r_q sum G - sum G mu cancels) and = randn, with an
    all-positive and a random upstream, against the fp64 local variance."""
    from ssl_amd.losses import get_local_weights
    gen = torch.Generator().manual_seed(k)
    r = mean + (0.1 if mean else 1.0) * torch.randn(shape, generator=gen)
    for up in (torch.rand(shape, generator=gen) + 0.1, torch.randn(shape, generator=gen)):
        x = r.clone().to(DEV).requires_grad_(True)
        v = get_local_weights(x, k)
        v.backward(up.to(DEV))
        rv, rgr = local_variance64(r, k, up)
        e_v, e_g = _ratio(v.detach().cpu(), rv), _ratio(x.grad.cpu(), rgr)
        print(f"LDL64 local-mean={mean} shape={shape} k={k} positive_upstream={bool((up > 0).all())} localV={e_v:.2e} "
              f"localgrad={e_g:.2e}")
        assert e_v <= TOL and e_g <= TOL, (e_v, e_g)


# ----------------------------------------------------------------------------------- streams and graphs (C ABI) ----
def _raw_loss(shape, k=7):
    """ssg_ldl_loss through the C ABI (raw_loss.RawLoss): loss and grad."""
    from ssl_amd import _lib
    B, C, H, W = shape
    L = _lib.lib()
    return RawLoss(L.ssg_ldl_loss, L.ssg_ldl_workspace_bytes(B, H, W),
                   lambda o, g, e: (o.data_ptr(), g.data_ptr(), e.data_ptr(), B, C, H, W, k, 1.0, 1),
                   (torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV)))


def test_side_stream_equals_default_stream():
    """Three launches in a line on the caller's stream; fixed-order sums: the same bits on any stream."""
    shape = (4, 3, 96, 80)
    o, g, e = _inputs(shape, 41)
    a = side_stream_equals_default_stream(lambda: _raw_loss(shape), (o, g, e))
    loss, grad = _hip(o, g, e, 7)
    assert torch.equal(a.loss[0], loss) and torch.equal(a.grad, grad)


def test_loss_replays_as_hip_graph():
    """Three batches: the second one replayed twice."""
    shape = (4, 3, 96, 80)
    first, second = _inputs(shape, 51), _inputs(shape, 52, kind="unclamped")
    want = replays_as_hip_graph(lambda: _raw_loss(shape), (first, second, second))
    assert not torch.equal(want[1], _hip(*first, 7)[1])      # the second batch really differs


# ------------------------------------------------------------------------ shared with test_gpu_lds_poison.py ----
def poison_cases():
    """What the LDS-poison test runs on the product build and again on the poisoned profiling build: every output of a
    minimal-side shape, a tile-edge shape, 4 x 3 x 128 x 128 (k = 7, 15, 7) and get_local_weights with its backward."""
    from ssl_amd.losses import get_local_weights, get_refined_artifact_map
    out = []
    for shape, k, seed in (((3, 3, 8, 11), 15, 1), ((3, 3, 17, 33), 7, 2), ((4, 3, 128, 128), 7, 3)):
        o, g, e = _inputs(shape, seed)
        out += list(_hip(o, g, e, k))
        x = o.clone().requires_grad_(True)
        w = get_refined_artifact_map(g, x, e, k)
        w.backward(torch.ones_like(w) * 0.5)
        out += [w.detach(), x.grad]
    r = (1 + 0.1 * torch.randn((2, 2, 24, 30), generator=torch.Generator().manual_seed(4))).to(DEV).requires_grad_(True)
    v = get_local_weights(r, 13)
    v.backward(torch.ones_like(v))
    out += [v.detach(), r.grad]
    torch.cuda.synchronize()
    return out
