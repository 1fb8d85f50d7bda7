"""BebyGAN's best-buddy loss and flat mask on the MI355X (ssl_amd/csrc/ssg_bbl.hip) against the fp64 restatement of
the contract (bbl_reference.py, which test_cpu_bbl.py pins to the reference's own outputs, tests/golden/f19_bbl.npz).

How a pick is judged.  The index is a discrete choice and fp32 cannot decide near-ties, so indices are not compared
directly: for every row the fp64 score of the candidate the GPU picked must lie within tau of the fp64 minimum,
    tau = 2 * 128 * 2^-24 * d * (alpha + beta) * max(|x|, |gt|)^2,
the fp32 evaluation bound of the expanded score (about 4 sums of up to 28 terms each), doubled because two scores are
compared -- derived, not measured.  A row whose fp64 gap between the best candidate and the best candidate of other
content exceeds tau is "decided": there the GPU's pick must be the fp64 argmin's very content, and where identical
patches are identical in fp32 as well, its lowest index.  Every input must leave at most 10 % of its rows undecided
(asserted on the reference alone).

Values: p1 is bit for bit F.unfold(x); sel_p2 within 1e-6 of the fp64 candidate at the GPU's index; the loss within
1e-6 relative and the gradient exactly (apart from the sign where |p1 - sel| < 1e-6, at most 1e-4 of the elements) of
the fp64 contract evaluated at the GPU's validated indices; against the pure fp64 loss only the loose bound
|dloss| <= share of rows picked differently * max|p1 - sel| holds.

Every comparison prints one `BBL64` line (pytest -s); profiles/bbl_parity.txt holds the table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bbl_reference as R
from raw_loss import RawLoss, replays_as_hip_graph, side_stream_equals_default_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (GT kind, shape, output: (blur radius, noise sigma, 8-bit?), alpha, beta)
RECIPES = {
    "tex blur2+n.1 a1 b.1": ("tex", (2, 3, 96, 96), (2, 0.1, False), 1.0, 0.1),
    "tex blur2+n.1 a1 b1": ("tex", (2, 3, 96, 96), (2, 0.1, False), 1.0, 1.0),
    "tex blur1+n.05 a1 b1": ("tex", (2, 3, 96, 96), (1, 0.05, False), 1.0, 1.0),
    "tex blur1+n.02 a1 b0": ("tex", (2, 3, 96, 96), (1, 0.02, False), 1.0, 0.0),
    "tex 8bit blur2 a1 b.1": ("tex8", (2, 3, 96, 96), (2, 0.0, True), 1.0, 0.1),
    "smooth odd blur2 a1 b.1": ("smooth", (2, 3, 99, 80), (2, 0.0, False), 1.0, 0.1),
    "tex blur2+n.1 a0 b1": ("tex", (2, 3, 96, 96), (2, 0.1, False), 0.0, 1.0),
    "tex C1 blur2+n.1 a1 b.1": ("tex", (2, 1, 96, 96), (2, 0.1, False), 1.0, 0.1),
}
SIDES = [(12, 12), (13, 13), (12, 13), (50, 41), (99, 80), (33, 100)]


def make_inputs(kind, shape, out, seed):
    """(x, gt) on the CPU, fp32, seeded."""
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        gt = R.smooth_noise(rng, shape, 3.0).float()
    else:
        gt = R.textured_gt(rng, shape)
    if kind == "tex8":
        gt = torch.round(gt * 255) / 255
    radius, noise, q8 = out
    x = R.degraded(rng, gt, radius, noise)
    if q8:
        x = torch.round(x.clamp(0, 1) * 255) / 255
    return x, gt


def reference_view(x, gt, alpha, beta, k=3, s=3, rows=None):
    """What the fp64 reference alone says about an input: scores, candidates, argmin, decided rows, tau, the share of
    self-picks and of picks per pyramid level."""
    sc, p1, cand = R.scores(x, gt, alpha, beta, k, s, rows)
    best = R.argmin_lowest(sc)
    t = R.tau(cand.shape[-1], alpha, beta, x, gt)
    decided = R.gap_to_distinct(sc, cand, best) > t
    _, sizes = R.candidates(gt, k, s)
    own = torch.arange(sc.shape[1]) if rows is None else rows
    levels = [float((best < sizes[0]).double().mean()),
              float(((best >= sizes[0]) & (best < sizes[0] + sizes[1])).double().mean()),
              float((best >= sizes[0] + sizes[1]).double().mean())]
    return dict(sc=sc, cand=cand, best=best, tau=t, decided=decided, sizes=sizes,
                self_share=float((best == own[None]).double().mean()), levels=levels)


def hip_search(x, gt, alpha, beta, k=3, s=3):
    from ssl_amd import engine
    ind, p1, sel = engine.bbl_search(x.to(DEV), gt.to(DEV), alpha, beta, k, s)
    torch.cuda.synchronize()
    return ind.cpu().long(), p1.cpu(), sel.cpu()


def hip_loss(x, gt, alpha, beta, k=3, s=3, loss_weight=1.0, reduction='mean'):
    from ssl_amd.losses import BestBuddyLoss
    xs = x.to(DEV).requires_grad_(True)
    loss = BestBuddyLoss(loss_weight, reduction, alpha, beta, k, s)(xs, gt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), xs.grad.cpu()


def check(name, x, gt, alpha, beta, k=3, s=3, rows=None, image=None, gpu=None, loss_weight=1.0, reduction='mean',
          exact_ties=False):
    """Every assertion of the module docstring on one input.  rows / image: judge the picks on a row subset of one
    image of the batch (the training size); the values are then checked on that image's rows too, the loss and the
    gradient on the whole batch at the GPU's indices.  exact_ties: the input's identical patches are identical in fp32
    too (a GT on the 1/256 grid: the fixed-tap pyramid is then exact in fp32), so the lowest index must win."""
    ind, p1, sel = gpu if gpu is not None else hip_search(x, gt, alpha, beta, k, s)
    loss_weight = float(np.float32(loss_weight))                     # the C ABI takes it as a float
    B, C, H, W = x.shape
    xs, gs = (x, gt) if image is None else (x[image:image + 1], gt[image:image + 1])
    v = reference_view(xs, gs, alpha, beta, k, s, rows)
    sc, cand, best, tau, decided = v["sc"], v["cand"], v["best"], v["tau"], v["decided"]
    undecided = 1.0 - float(decided.double().mean())
    assert undecided <= 0.10, (name, undecided)                      # the condition on the input
    M = cand.shape[1]
    assert int(ind.min()) >= 0 and int(ind.max()) < M
    assert torch.equal(p1, F.unfold(x, k, padding=0, stride=s).permute(0, 2, 1))
    ind_v = ind if image is None else ind[image:image + 1]
    sel_v = sel if image is None else sel[image:image + 1]
    if rows is not None:
        ind_v, sel_v = ind_v[:, rows], sel_v[:, rows]
    excess = sc.gather(2, ind_v[..., None])[..., 0] - sc.min(-1).values
    worst = float(excess.max())
    differ = float((ind_v != best).double().mean())
    print(f"BBL64 {name}: shape {tuple(x.shape)} a {alpha} b {beta} k {k} s {s} rows {sc.shape[1]} M {M} tau {tau:.3e} "
          f"worst excess {worst:.3e} ({worst / tau:.4f} tau) undecided {undecided:.4f} picked differently {differ:.4f} "
          f"self {v['self_share']:.3f} levels {v['levels'][0]:.3f}/{v['levels'][1]:.3f}/{v['levels'][2]:.3f}")
    assert worst <= tau, (name, worst, tau)
    sel64 = cand.gather(1, ind_v[..., None].expand(-1, -1, cand.shape[-1]))
    best64 = cand.gather(1, best[..., None].expand(-1, -1, cand.shape[-1]))
    assert bool((sel64 == best64).all(-1)[decided].all()), name      # decided rows: the argmin's very content
    if exact_ties:                                                    # and the lowest index of identical patches
        assert torch.equal(ind_v[decided], best[decided]), name
    assert float((sel_v.double() - sel64).abs().max()) <= 1e-6, name
    # the loss and the gradient at the GPU's indices, whole batch
    cand_all = cand if image is None else R.candidates(gt, k, s)[0]
    loss, grad = hip_loss(x, gt, alpha, beta, k, s, loss_weight, reduction)
    loss64, grad64, diff = R.loss_and_grad(x, cand_all, ind, k, s, loss_weight, reduction)
    assert abs(float(loss) - float(loss64)) <= 1e-6 * float(loss64), (name, float(loss), float(loss64))
    near = F.fold(((diff.abs() < 1e-6) & (diff != 0)).double().permute(0, 2, 1), (H, W), kernel_size=k, stride=s) > 0
    assert float(near.double().mean()) <= 1e-4, name
    assert torch.equal(grad[~near], grad64.float()[~near]), name
    if rows is None and image is None:
        pure, _, dpure = R.loss_and_grad(x, cand, best, k, s, loss_weight, reduction)
        scale = loss_weight if reduction == 'mean' else loss_weight * diff.numel()
        bound = differ * max(float(diff.abs().max()), float(dpure.abs().max())) * scale
        print(f"BBL64 {name}: loss {float(loss):.8g} at GPU indices {float(loss64):.8g} pure fp64 {float(pure):.8g} "
              f"|dloss| {abs(float(loss) - float(pure)):.3e} loose bound {bound:.3e}")
        assert abs(float(loss64) - float(pure)) <= bound + 1e-12 * float(pure), name
    return v


# ------------------------------------------------------------------------------------------------ the fixture ----
def test_hip_against_the_reference_fixture(golden):
    """F19: every decided row's sel_p2 equals the reference's to 1e-6; loss and gradient within 1e-6 of their maximum
    wherever the picks agree row for row; the flat masks bit for bit."""
    from ssl_amd.losses import get_flat_mask
    z = golden("f19_bbl")
    for i in range(int(z["n_cases"])):
        c = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        x, gt = torch.from_numpy(c["x"]), torch.from_numpy(c["gt"])
        alpha, beta = float(c["alpha"]), float(c["beta"])
        v = check(f"F19 c{i}", x, gt, alpha, beta)
        ind, p1, sel = hip_search(x, gt, alpha, beta)
        assert torch.equal(p1, torch.from_numpy(c["p1"]))
        err = (sel - torch.from_numpy(c["sel_p2"])).abs().amax(-1)
        assert float(err[v["decided"]].max()) <= 1e-6
        if float(err.max()) <= 1e-6:     # the same picks in every row: the same loss and gradient
            loss, grad = hip_loss(x, gt, alpha, beta)
            assert abs(float(loss) - float(c["loss"])) <= 1e-6 * float(c["loss"])
            assert float((grad - torch.from_numpy(c["grad"])).abs().max()) <= 1e-6 * float(np.abs(c["grad"]).max())
        if "mask" in c:
            assert torch.equal(get_flat_mask(gt.to(DEV)).cpu(), torch.from_numpy(c["mask"]))
    img = torch.from_numpy(z["m_img"]).to(DEV)
    for k in (11, 3):
        assert torch.equal(get_flat_mask(img, kernel_size=k).cpu(), torch.from_numpy(z[f"m_mask_k{k}"]))


# ---------------------------------------------------------------------------------------------- the recipes ----
@pytest.mark.parametrize("name", list(RECIPES))
def test_recipes_at_96(name):
    kind, shape, out, alpha, beta = RECIPES[name]
    x, gt = make_inputs(kind, shape, out, 1000 + list(RECIPES).index(name))
    check(name, x, gt, alpha, beta)


def test_recipes_search_other_patches_and_every_level():
    """On the reference alone: at least two recipes have under 20 % self-picks, at least one selects from all three
    pyramid levels (a GT plus small noise would make every row pick itself and test nothing)."""
    low_self = all_levels = 0
    for i, (name, (kind, shape, out, alpha, beta)) in enumerate(RECIPES.items()):
        x, gt = make_inputs(kind, shape, out, 1000 + i)
        v = reference_view(x, gt, alpha, beta)
        low_self += v["self_share"] < 0.20
        all_levels += min(v["levels"]) > 0
    assert low_self >= 2 and all_levels >= 1, (low_self, all_levels)


def test_training_size():
    """16 x 3 x 192 x 192 (N = 4,096, M = 5,376): all rows of image 0 and 512 rows of image 15 against fp64."""
    shape = (16, 3, 192, 192)
    x, gt = make_inputs("tex", shape, (2, 0.1, False), 77)
    gpu = hip_search(x, gt, 1.0, 1.0)
    check("training size image 0", x, gt, 1.0, 1.0, image=0, gpu=gpu)
    rows = torch.from_numpy(np.sort(np.random.default_rng(5).choice(4096, 512, replace=False)))
    check("training size image 15", x, gt, 1.0, 1.0, rows=rows, image=15, gpu=gpu)


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("C", [1, 3])
def test_sides_and_channels(H, W, C):
    """Sides 12 (the smallest: gt/4 is 3 x 3), 13, 50 x 41, 99 x 80: remainders mod 3, odd pyramid sides, N and M not
    multiples of 32."""
    x, gt = make_inputs("tex", (2, C, H, W), (2, 0.1, False), 11 * H + W + C)
    v = check(f"sides {H}x{W} C{C}", x, gt, 1.0, 0.1)
    if (H, W) == (50, 41):
        assert v["sc"].shape[1] % 32 and v["sc"].shape[2] % 32


@pytest.mark.parametrize("alpha,beta,k,s", [(1.0, 0.0, 3, 3), (0.0, 1.0, 3, 3), (0.3, 2.5, 3, 3), (1.0, 1.0, 2, 3),
                                            (1.0, 0.5, 3, 4), (1.0, 1.0, 1, 1), (1.0, 1.0, 5, 5)])
def test_weights_and_window_geometry(alpha, beta, k, s):
    """alpha = 0, beta = 0, unequal weights; stride > k (pixels between patches get a zero gradient), k = 1, 2 and
    k = 5 with C = 1 (d = 25)."""
    C = 1 if k == 5 else 3
    x, gt = make_inputs("tex", (2, C) + ((16, 20) if k == 1 else (60, 72)), (1, 0.05, False), 300 + 10 * k + s)
    check(f"a{alpha} b{beta} k{k} s{s}", x, gt, alpha, beta, k, s, loss_weight=0.7, reduction='sum' if k == 2 else 'mean')


def test_d_above_27_runs_the_16_step_kernel():
    x, gt = make_inputs("tex", (2, 7, 48, 36), (1, 0.05, False), 55)      # d = 28 with k = 2
    check("C7 k2 (d 28)", x, gt, 1.0, 1.0, 2, 2)
    x, gt = make_inputs("tex", (1, 31, 24, 24), (1, 0.05, False), 56)     # d = 31 with k = 1
    check("C31 k1 (d 31)", x, gt, 1.0, 0.5, 1, 2)


def test_exactly_repeated_patches_lowest_index_wins():
    """A GT quantised to 256 levels (the 1/256 grid, on which the fixed-tap pyramid is exact in fp32 and fp64 alike)
    with constant regions and a repeated textured block: identical candidate patches tie exactly, at every level, and
    the lowest index must win (exact_ties: the fp64 lowest-index argmin on every decided row).  The output equals the
    GT in the flat regions, so those rows' best candidates are the repeated ones."""
    rng = np.random.default_rng(91)
    gt = R.textured_gt(rng, (2, 3, 96, 96))
    gt[:, :, :36, :48] = torch.from_numpy(rng.random((2, 3, 1, 1))).float()
    gt[:, :, 60:, 48:] = 0.25
    gt[1, :, 40:52, :24] = gt[1, :, 4:16, 60:84]                           # a repeated textured block
    gt = torch.round(gt * 256) / 256
    x = torch.round(R.degraded(rng, gt, 1, 0.02).clamp(0, 1) * 256) / 256
    x[:, :, :36, :48] = gt[:, :, :36, :48]
    x[:, :, 60:, 48:] = gt[:, :, 60:, 48:]
    v = check("repeated patches 256 levels", x, gt, 1.0, 1.0, exact_ties=True)
    cand, best = v["cand"], v["best"]
    # rows whose best candidate has a later identical twin: there the rule decided something
    twins = 0
    for b in range(2):
        same = (cand[b][None] == cand[b][best[b]][:, None]).all(-1)
        twins += int((same.sum(-1) > 1).sum())
    assert twins >= 200, twins


# ------------------------------------------------------------------------------------------- the Python layer ----
def test_channels_last_and_strided_inputs():
    from ssl_amd import engine
    x, gt = make_inputs("tex", (2, 3, 48, 60), (1, 0.05, False), 17)
    want = engine.bbl_search(x.to(DEV), gt.to(DEV))
    xc = x.to(DEV).contiguous(memory_format=torch.channels_last)
    big = torch.zeros((2, 3, 48, 120), device=DEV)
    big[..., ::2] = gt.to(DEV)
    got = engine.bbl_search(xc, big[..., ::2])
    assert not xc.is_contiguous() and not big[..., ::2].is_contiguous()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_callers_two_lines_against_the_fused_loss():
    """p1, sel_p2 = best_buddy.forward(x=output, gt=gt); l = cri_pix_bb(p1, sel_p2) with ssl_amd.losses.L1Loss, as the
    reference's caller writes them, against BestBuddyLoss: the same loss and gradient (to the rounding of the one
    scale factor, which the two paths form differently: 1e-6 relative)."""
    from ssl_amd.losses import BBL, BestBuddyLoss, L1Loss
    x, gt = make_inputs("tex", (2, 3, 50, 41), (2, 0.1, False), 23)
    best_buddy, cri_pix_bb = BBL(), L1Loss(loss_weight=1.0, reduction='mean')
    output = x.to(DEV).requires_grad_(True)
    p1, sel_p2 = best_buddy.forward(x=output * 1.0, gt=gt.to(DEV))
    assert p1.requires_grad and not sel_p2.requires_grad
    l = cri_pix_bb(p1, sel_p2)
    l.backward()
    x2 = x.to(DEV).requires_grad_(True)
    l2 = BestBuddyLoss()(x2, gt.to(DEV))
    l2.backward()
    assert abs(l.item() - l2.item()) <= 1e-6 * l2.item()
    assert torch.equal(output.grad == 0, x2.grad == 0)
    assert float((output.grad - x2.grad).abs().max()) <= 1e-6 * float(x2.grad.abs().max())
    assert float(x2.grad[:, :, 48:, :].abs().max()) == 0 and float(x2.grad[:, :, :, 39:].abs().max()) == 0


def test_gt_requiring_grad_raises_and_cpu_tensors_raise():
    from ssl_amd.losses import BBL, BestBuddyLoss
    x, gt = make_inputs("tex", (1, 3, 24, 24), (1, 0.05, False), 3)
    with pytest.raises(ValueError, match="gt"):
        BestBuddyLoss()(x.to(DEV), gt.to(DEV).requires_grad_(True))
    with pytest.raises(RuntimeError, match="GPU"):
        BBL().forward(x, gt)
    with pytest.raises(NotImplementedError, match="31"):
        BBL(ksize=4, stride=4).forward(torch.zeros(1, 3, 64, 64, device=DEV), torch.zeros(1, 3, 64, 64, device=DEV))


def test_two_runs_are_bit_identical():
    x, gt = make_inputs("tex", (4, 3, 96, 96), (2, 0.1, False), 31)
    a, b = hip_search(x, gt, 1.0, 1.0), hip_search(x, gt, 1.0, 1.0)
    for u, w in zip(a, b):
        assert torch.equal(u, w)
    la, lb = hip_loss(x, gt, 1.0, 1.0), hip_loss(x, gt, 1.0, 1.0)
    assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])


# ----------------------------------------------------------------------------------- streams and graphs (C ABI) ----
def _raw_loss(shape):
    """ssg_bbl_loss through the C ABI (raw_loss.RawLoss): loss, grad and ind."""
    from ssl_amd import _lib
    B, C, H, W = shape
    L = _lib.lib()
    return RawLoss(L.ssg_bbl_loss, L.ssg_bbl_workspace_bytes(B, C, H, W, 3, 3),
                   lambda x, g: (x.data_ptr(), g.data_ptr(), B, C, H, W, 3, 3, 1.0, 1.0, 1.0, 1),
                   (torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV),
                    torch.zeros((B, (H // 3) * (W // 3)), dtype=torch.int32, device=DEV)))


def _dev_inputs(shape, seed):
    return tuple(t.to(DEV) for t in make_inputs("tex", shape, (2, 0.1, False), seed))


def test_side_stream_equals_default_stream():
    shape = (2, 3, 96, 81)
    x, g = _dev_inputs(shape, 41)
    a = side_stream_equals_default_stream(lambda: _raw_loss(shape), (x, g))
    loss, grad = hip_loss(x.cpu(), g.cpu(), 1.0, 1.0)
    assert torch.equal(a.loss[0].cpu(), loss) and torch.equal(a.grad.cpu(), grad)


def test_loss_replays_as_hip_graph():
    """The captured call is a single chain of four launches."""
    shape = (2, 3, 96, 81)
    first, second = _dev_inputs(shape, 51), _dev_inputs(shape, 52)
    want = replays_as_hip_graph(lambda: _raw_loss(shape), (first, second))
    first_run = _raw_loss(shape)
    first_run(*first)
    assert not torch.equal(first_run.outputs()[1], want[1])      # the second batch really differs


def test_c_abi_refusals_on_the_device():
    """The refusals of test_cpu_bbl.py with real device pointers: nothing is launched, the outputs stay untouched."""
    from ssl_amd import _lib
    L = _lib.lib()
    x, g = _dev_inputs((1, 3, 24, 24), 5)
    ind = torch.full((1, 64), -7, dtype=torch.int32, device=DEV)
    nb = L.ssg_bbl_workspace_bytes(1, 3, 24, 24, 3, 3)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)

    def search(H=24, W=24, k=3, s=3, a=1.0, b=1.0, wsp=ws.data_ptr(), n=nb, C=3):
        return L.ssg_bbl_search(x.data_ptr(), g.data_ptr(), 1, C, H, W, k, s, a, b, ind.data_ptr(), None, None, wsp, n, None)

    assert search(s=2) == -1 and search(a=0.0, b=0.0) == -1 and search(a=-0.5) == -1
    assert search(k=4, s=4) == -2
    assert search(H=11) == -4 and search(W=8) == -4
    assert search(n=nb - 1) == -3
    assert search(wsp=ws.data_ptr() + 4) == -5
    mask = torch.full((1, 1, 24, 24), -7.0, device=DEV)
    fm = lambda H=24, W=24, k=11: L.ssg_flat_mask(x.data_ptr(), 1, H, W, k, 0.025, mask.data_ptr(), None)
    assert fm(k=4) == -1 and fm(k=17) == -2 and fm(H=5) == -4 and fm(k=15, W=7) == -4
    torch.cuda.synchronize()
    assert int((ind != -7).sum()) == 0 and int((mask != -7).sum()) == 0
    assert search() == 0 and fm() == 0
    torch.cuda.synchronize()
    assert int((ind == -7).sum()) == 0 and int((mask == -7).sum()) == 0


# ------------------------------------------------------------------------------------------------- flat mask ----
DELTA = 1e-6    # luminance error <= 3 * 2^-24, std 1-Lipschitz in it up to sqrt(n / (n - 1)), the two-pass variance adds
                # about 60 * 2^-24 relative (1e-7 at thresh 0.025): 1e-6 is 3 x the sum


def check_mask(name, img, k=11, thresh=0.025):
    from ssl_amd.losses import get_flat_mask
    std = R.flat_std(img, k)
    close = (std - thresh).abs() <= DELTA
    assert float(close.double().mean()) <= 1e-3, (name, float(close.double().mean()))     # the condition on the input
    got = get_flat_mask(img.to(DEV), kernel_size=k, std_thresh=thresh).cpu()
    assert got.shape == (img.shape[0], 1) + tuple(img.shape[2:]) and got.dtype == img.dtype
    want = (std < thresh).float()
    wrong = int((got != want)[~close].sum())
    print(f"BBL64 mask {name}: shape {tuple(img.shape)} k {k} thresh {thresh} flat share {float(want.mean()):.4f} within delta "
          f"{int(close.sum())} disagreements outside delta {wrong} (inside {int((got != want)[close].sum())})")
    assert wrong == 0, (name, wrong)
    assert bool(((got == 0) | (got == 1)).all())
    return float(want.mean())


@pytest.mark.parametrize("k", [3, 11, 15])
def test_flat_mask_natural_like_and_noise(k):
    rng = np.random.default_rng(60 + k)
    share = check_mask("natural-like 8bit", R.natural_like_u8(rng, 2, 120, 144), k)
    assert 0.05 < share < 0.95
    check_mask("noise", torch.from_numpy(rng.random((2, 3, 64, 80))).float(), k)
    check_mask("faint noise", 0.5 + 0.02 * torch.from_numpy(rng.standard_normal((2, 3, 64, 80))).float(), k, 0.0125)


@pytest.mark.parametrize("k", [3, 5, 11, 15])
def test_flat_mask_minimal_sides_and_tile_edges(k):
    """H or W = k // 2 + 1 (the smallest the reflect pad allows) and sides around the 32 x 16 tile."""
    rng = np.random.default_rng(70 + k)
    m = k // 2 + 1
    for H, W in ((m, m), (m, 40), (37, m), (16, 32), (17, 33), (15, 31), (33, 65), (48, 64)):
        check_mask(f"{H}x{W}", R.natural_like_u8(rng, 2, 64, 80)[:, :, :H, :W].contiguous(), k)


def test_flat_mask_training_size_and_scale():
    from ssl_amd.losses import get_flat_mask
    rng = np.random.default_rng(80)
    img = R.natural_like_u8(rng, 4, 192, 192)
    check_mask("192", img)
    up = get_flat_mask(img[:1, :, :48, :48].to(DEV), scale=2)
    want = get_flat_mask(F.interpolate(img[:1, :, :48, :48].to(DEV), scale_factor=2, mode='bicubic', align_corners=False))
    assert up.shape == (1, 1, 96, 96) and torch.equal(up, want)
    x = img.to(DEV).requires_grad_(True)
    assert not get_flat_mask(x).requires_grad


# ------------------------------------------------------------------------ shared with test_gpu_bbl_poison.py ----
def poison_cases():
    """What the LDS-poison test runs on the product build and again on the poisoned profiling build: every output of
    the search, the loss and the mask on a minimal-side shape, an odd shape and 2 x 3 x 96 x 96."""
    from ssl_amd import engine
    out = []
    for shape, seed in (((2, 3, 12, 13), 1), ((2, 3, 50, 41), 2), ((2, 3, 96, 96), 3)):
        x, g = _dev_inputs(shape, seed)
        out += list(engine.bbl_search(x, g, 1.0, 0.5))
        xs = x.clone().requires_grad_(True)
        loss = engine.bbl_loss(xs, g, 1.0, 0.5)
        loss.backward()
        out += [loss.detach().reshape(1), xs.grad]
        for k in (3, 11, 15):
            out.append(engine.flat_mask(g, k, 0.05))
    torch.cuda.synchronize()
    return out
