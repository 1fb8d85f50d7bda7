"""Range of the deterministic gradient's fixed-point conversion in the dense-tile backward.

The deterministic backward converts every contribution to fixed point before a 64-bit integer atomic (ssg_common.hpp:
grad_fix_scale_of puts |G|max * scale into [2^35, 2^36) when the bound of |G| is the exact maximum).  The dense-tile
backward converts whole-tile sums over all offset rows its wave owns, and a wave owns ALL of them when the plan holds more
dense tiles than the device has wave slots (qs = 1: the full-size dense-mask step).  On a plain step edge the fp64 oracle
puts such a sum at 2^15.5 |G|max for an interior tile (tests/test_cpu_fix_range.py shows it on the reference alone):
2^50.5 .. 2^51.5 after scaling, by where |G|max falls in its binade.  The magic-number conversion fix_round() holds
2^51 and does not saturate beyond: it returns 2^51 + excess / 2 -- percents of max|grad| on hundreds of pixels,
bit-reproducible, no fault and no NaN.  The dense backward's flushes therefore go through grad_add_wide().

What the cases showed on the library BEFORE that change (profiles/fix_range.txt keeps both tables):
  large (qs = 1), weight factor 2^0 (|G|max * scale = 2^35.78): gradient 1.5e-2 of its maximum off, fused and
    materialising; the other three weights (2^35.03 .. 2^35.53) within 8e-7.  The tile-major instantiation under a full
    mask: 1.5e-2 off the fp32-atomic step at factor 2^0.25.
  control (the block alone, 24 tiles, qs = 5, tile-major): 6.2e-2 and 1.3e-2 off at the two weights in the upper half of
    the binade (2^35.99, 2^35.74) -- although the reference's NET sum over a fifth of the offset rows reaches 2^49.8
    only.  With the split fixed in the profiling build the same case is 7.9e-2 / 6.2e-2 / 1.4e-1 off at 1 / 5 / 25 parts:
    splitting does not shrink what a wave converts.  (Consistent with how the border sums are grouped: the wave of the
    first part adds the tile's sum_b for all offsets, every wave subtracts its own share, so the pieces cancel across
    waves only.  The reference reach describes one wave per tile; for split tiles it understates them.)  The split is no
    protection, and neither are small shapes.
After the change every case is within 9e-7 of the oracle.

Construction: the 32 x 96 step-edge block in an image with more dense tiles than wave slots (dense threshold 1, every
other tile ONE edge pixel: the oracle sees ~3.6 k rows), so the device chooses qs = 1 by itself; the tile count is read
back from the plan and the split asserted, so the cases cannot pass vacuously on a device with more CUs.  The same block
alone (24 tiles, qs = 5) is the control for the split.  Witnesses per case: the fp64 oracle's gradient (1e-5 of its
maximum, the suite's rule), a second run (bit for bit) and the fp32-atomic step, which never converts.

Every case prints one FIXRANGE line (pytest -s) before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

import fix_range_reference as fr
import test_gpu_parity as tp
from oracle import ssg_oracle as orc

pytestmark = pytest.mark.gpu

KS, KW, SIGMA = 49, 13, 1.0
WEIGHTS = [1e3 * 2.0 ** (j / 4) for j in range(4)]   # one octave: |G|max moves through its binade, the scale with it


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _loss_case(sr, gt, mask, ks, kw, tiles, cus):
    """fp64 reference of a loss case at weights 1e3 (computed once per module) and the reach of its whole-tile sums at
    the split the device will choose."""
    ref = fr.loss_reference(sr, gt, mask, ks, kw, SIGMA, 1e3, 1e3)
    parts = fr.offset_parts(tiles, cus, ks)
    reach = fr.tile_reach(sr, ref["gD"], ref["pos"], ks, kw, fr.tile_rows(ks), 32, parts)
    return dict(sr=sr, gt=gt, mask=mask, ref=ref, tiles=tiles, parts=parts, reach=reach)


@pytest.fixture(scope="module")
def large49(cus):
    sr, gt, mask, _, tiles = fr.embedded_case(KS, cus, fr.CASE_SEED)
    return _loss_case(sr, gt, mask, KS, KW, tiles, cus)


@pytest.fixture(scope="module")
def control49(cus):
    sr, gt = fr.control_pair(fr.CASE_SEED)
    return _loss_case(sr, gt, np.ones((32, 96), np.float32), KS, KW, 24, cus)


@pytest.fixture(scope="module")
def large25(cus):
    """(25,9): 8 x 32 tiles, two waves per tile -- as many tiles as the device has wave slots per half, and one more."""
    need = fr.wave_slots(cus, 25) // fr.waves_per_tile(25) + 1
    sr, gt, mask, block, tiles = fr.embedded_case(25, cus, fr.CASE_SEED, need)
    return dict(sr=sr, gt=gt, mask=mask, block=block, tiles=tiles, parts=fr.offset_parts(tiles, cus, 25))


def scaled(ref, f):
    """The reference at weights f x 1e3: both losses and the gradient are linear in the pair of weights, the SSG rows do
    not depend on them (an exact statement about the fp64 reference, not an approximation of it)."""
    out = dict(ref)
    for k in ("l1", "kl", "grad", "gD"):
        out[k] = ref[k] * f
    return out


def plan_counts(step):
    """(dense tiles, rows outside them, tile-major slots) of a finished step, from the plan in its workspace."""
    from ssl_amd import _lib
    B, C, H, W = step.shape
    lay = (ctypes.c_size_t * 9)()
    assert _lib.lib().ssg_loss_workspace_layout(B, H, W, step.capacity, step.cfg[0], 0 if step.materialise else 1, lay) == 0
    plan = step.ws[lay[2]: lay[2] + 16].view(torch.int32).cpu().numpy()
    return int(plan[1]) + int(plan[3]), int(plan[0]), int(lay[8])


def tm_active(step, n):
    """ssg_common.hpp's tm_active(): the call's dense tiles live in the tile-major regions."""
    nd, sparse, slots = plan_counts(step)
    return 0 < nd <= slots and 5 * (n - sparse) >= 3 * 128 * nd


def fused_rows(step, n):
    """(s_sr, s_gt) of a finished FUSED step: rebuilt from the tile-major regions (tp.tile_major_ssg), or -- a call whose
    tiles did not go tile-major -- from its row-major scratch rows: a dense-tile row still holds e = exp(-d / sigma) and a
    non-zero fp64 row scale 1 / (sum e + eps) (s = their fp64 product rounded once, ssg_grad_rows' own), a direct row is
    normalised (scale 0)."""
    if tm_active(step, n):
        return tp.tile_major_ssg(step)
    from ssl_amd import _lib
    B, C, H, W = step.shape
    ks, cap = step.cfg[0], step.capacity
    lay = (ctypes.c_size_t * 9)()
    assert _lib.lib().ssg_loss_workspace_layout(B, H, W, cap, ks, 1, lay) == 0
    rs = step.ws[lay[3]: lay[3] + 16 * cap].view(torch.float64).cpu().numpy().reshape(2, cap)
    assert (rs >= 0).all()
    out = []
    for img in range(2):
        rows = step.ws[lay[4 + img]: lay[4 + img] + 4 * cap * ks * ks].view(torch.float32).view(cap, ks * ks)[:n].cpu().numpy()
        sc = rs[img, :n, None]
        out.append(np.where(sc != 0, (rows.astype(np.float64) * sc).astype(np.float32), rows))
    return out


def report(name, shape, tiles, parts, gmax, reach, err, **more):
    tail = "".join(f" {k}={v:.3g}" if isinstance(v, float) else f" {k}={v}" for k, v in more.items())
    print(f"\nFIXRANGE {name} shape={shape[0]}x{shape[1]} tiles={tiles} parts={parts} Gmax={gmax:.4g} "
          f"reach_bits={fr.reach_bits(reach):.2f} err/max={err:.3g}{tail}")


def run_k49(dev, cus, case, w, materialise, want_parts, name):
    from ssl_amd import engine
    sr, gt, mask = case["sr"], case["gt"], case["mask"]
    H, W = mask.shape
    ref = scaled(case["ref"], w / 1e3)
    N = int(mask.sum())
    srt, gtt, mt = tp.T(sr[None], dev), tp.T(gt[None], dev), tp.T(mask[None, None], dev)
    prev = engine.set_dense_threshold(1)
    try:
        def make(det):
            return engine.LossStep(1, 3, H, W, KS, KW, SIGMA, 1e-10, True, w, w, device=dev, deterministic=det,
                                   materialise=materialise, capacity=N + 64)
        step = make(True)
        loss, grad = step(srt, gtt, mt)
        loss, grad = loss.clone(), grad.clone()
        n = int(step.counts[0])
        assert n == N == ref["n_edges"]
        # the split the device chose: every tile of the image is a dense tile, and the device's rule gives `want_parts`
        tiles, sparse, _ = plan_counts(step)
        assert tiles == case["tiles"] and sparse == 0, f"plan holds {tiles} dense tiles (+{sparse} rows), predicted {case['tiles']}"
        parts = fr.offset_parts(tiles, cus, KS)
        assert parts == want_parts == case["parts"], (f"{cus} CUs split {tiles} tiles {parts} ways, this case needs "
                                                      f"{want_parts}: it would not test what it is for")
        if materialise:
            s_sr, s_gt = step.ssg_sr[:n].cpu().numpy(), step.ssg_gt[:n].cpu().numpy()
        else:
            s_sr, s_gt = fused_rows(step, n)
        gref, nflip = tp.ref_grad_with_gpu_signs(sr[None], mask[None], KS, KW, SIGMA, ref, s_sr, s_gt, w_l1=w)
        gmx = np.abs(gref).max()
        err = tp.maxerr(grad.cpu(), gref) / gmx
        loss2, grad2 = step(srt, gtt, mt)
        same = torch.equal(loss, loss2) and torch.equal(grad, grad2)
        step_a = make(False)
        loss_a, grad_a = step_a(srt, gtt, mt)
        err_a = float((grad_a - grad).abs().max()) / float(grad.abs().max())
        err_a64 = tp.maxerr(grad_a.cpu(), gref) / gmx
        report(name, (H, W), tiles, parts, float(np.abs(ref["gD"]).max()), case["reach"], err,
               form="materialising" if materialise else "fused", tile_major=tm_active(step, n), w=float(w), maxgrad=float(gmx),
               atomic_vs_det=err_a, atomic_vs_oracle=err_a64, reproducible=same, sign_ties=nflip)
        assert tp.maxerr(s_sr, ref["s_sr"]) <= 1e-5 and tp.maxerr(s_gt, ref["s_gt"]) <= 1e-5
        assert abs(float(loss[0]) - ref["l1"]) <= 1e-5 * ref["l1"]
        assert bool(torch.isfinite(grad).all())
        assert err <= 1e-5, f"deterministic gradient {err:.3g} of max|grad| from the fp64 oracle (fp32 atomics: {err_a64:.3g})"
        assert same
        assert torch.equal(loss_a, loss) and err_a <= 1e-5
    finally:
        engine.set_dense_threshold(prev)


@pytest.mark.parametrize("materialise", [False, True])
@pytest.mark.parametrize("j", range(4))
def test_k49_step_one_wave_per_tile_vs_oracle(dev, cus, large49, j, materialise):
    """The (49,13) deterministic step, sigma 1, on the step-edge block inside 132 x 512 (528 dense tiles on 256 CUs: qs = 1,
    one wave sums all 2,401 offsets of its tile before the conversion; reference reach 2^50.54): SSG rows 1e-5, L1 1e-5
    relative, gradient 1e-5 of its maximum against the fp64 oracle (the GPU's sign at fp32-undecided L1 entries), a
    second run bit for bit, and the fp32-atomic step (no conversion) to 1e-5 -- fused and materialising, at four weights
    over one octave so that one of them has the largest scale the rule can give.  (One edge pixel per filler tile keeps
    the tiles out of the tile-major regions -- they must be 60 % full on average: this is the row-major instantiation of
    the dense backward, whose flush is the same code; test_k49_tile_major_step_one_wave_per_tile covers the other.)"""
    run_k49(dev, cus, large49, WEIGHTS[j], materialise, 1, "k49-large")


@pytest.mark.parametrize("materialise", [False, True])
@pytest.mark.parametrize("j", range(4))
def test_k49_step_control_five_waves_per_tile_vs_oracle(dev, cus, control49, j, materialise):
    """CONTROL for the split: the same block alone, 32 x 96 = 24 dense tiles, qs = 5 -- a fifth of the offset rows per
    conversion (reference reach of the net sum 2^49.8), the regime of every other (49,13) oracle test; here the edge
    fills every tile and the weights walk through the binade.  Same checks.  (With fix_round() in the flushes two of the
    four weights failed here too: see the module docstring.)"""
    run_k49(dev, cus, control49, WEIGHTS[j], materialise, 5, "k49-control")


def test_k49_tile_major_step_one_wave_per_tile(dev, cus):
    """The TILE-MAJOR instantiation at qs = 1: the same image under a FULL mask (every tile 128 edge pixels: the tiles fit
    the regions and run tile-major, 67,584 rows).  No oracle at that size in a test's time; the witnesses are the ones on
    the device -- the fp32-atomic step, which never converts, to 1e-5 of max|grad|, and a second run bit for bit -- and
    the plan: tile count, split and tile-major decision are asserted."""
    from ssl_amd import engine
    sr, gt, _, _, tiles = fr.embedded_case(KS, cus, fr.CASE_SEED)
    H, W = sr.shape[1:]
    srt, gtt, mt = tp.T(sr[None], dev), tp.T(gt[None], dev), torch.ones((1, 1, H, W), device=dev)
    prev = engine.set_dense_threshold(1)
    try:
        worst = 0.0
        for w in WEIGHTS:
            step = engine.LossStep(1, 3, H, W, KS, KW, SIGMA, 1e-10, True, w, w, device=dev, deterministic=True, materialise=False)
            loss, grad = step(srt, gtt, mt)
            loss, grad = loss.clone(), grad.clone()
            n = int(step.counts[0])
            nd, sparse, _ = plan_counts(step)
            assert n == H * W and nd == tiles and sparse == 0 and tm_active(step, n)
            parts = fr.offset_parts(nd, cus, KS)
            assert parts == 1, f"{cus} CUs split {nd} tiles {parts} ways"
            loss2, grad2 = step(srt, gtt, mt)
            same = torch.equal(loss, loss2) and torch.equal(grad, grad2)
            del step
            step_a = engine.LossStep(1, 3, H, W, KS, KW, SIGMA, 1e-10, True, w, w, device=dev, deterministic=False, materialise=False)
            loss_a, grad_a = step_a(srt, gtt, mt)
            err_a = float((grad_a - grad).abs().max()) / float(grad_a.abs().max())
            del step_a
            print(f"\nFIXRANGE k49-tile-major shape={H}x{W} tiles={nd} parts={parts} Gmax=n/a reach_bits=n/a err/max=n/a "
                  f"form=fused tile_major=True w={w:.4g} maxgrad={float(grad_a.abs().max()):.3g} atomic_vs_det={err_a:.3g} "
                  f"reproducible={same}")
            worst = max(worst, err_a)
            assert bool(torch.isfinite(grad).all()) and same and torch.equal(loss_a, loss)
        assert worst <= 1e-5
    finally:
        engine.set_dense_threshold(prev)


def test_k25_map_backward_one_part_vs_oracle(dev, cus, large25):
    """ssg_map + backward at (25,9), qs = 1 (1,056 tiles of 8 x 32 on 256 CUs), exact |G| maximum from ssg_grad_rows: the
    cotangent +1 where the offset pixel lies on the bright side of the edge and -1 elsewhere makes every row of a tile
    push the same way.  Against the oracle's VJP at 1e-5 of its maximum.  The reach (2^48.05 at tile level: two bits and
    more to spare) is printed, not asserted: a guard."""
    from ssl_amd import engine
    ks, kw = 25, 9
    sr, mask, (y0, x0, h, w) = large25["sr"], large25["mask"], large25["block"]
    H, W = mask.shape
    pos = orc.mask_to_pos(mask)
    n = len(pos)
    xo = pos[:, 1, None, None] - ks // 2 + np.arange(ks)[None, None, :] + np.zeros((1, ks, 1), np.int64)
    cot = np.where(xo >= x0 + w // 2, 1.0, -1.0)
    sr64 = sr.astype(np.float64)
    S = orc.ssg_epilogue(orc.distance(sr64, pos, ks, kw), kw, 3, SIGMA, True)
    gD = orc.ssg_epilogue_backward(S, cot.reshape(n, -1), ks, kw, 3, SIGMA, True)
    gref = orc.distance_backward(sr64, pos, ks, kw, gD)
    reach = fr.tile_reach(sr, gD, pos, ks, kw, 8, 32, large25["parts"])
    prev = engine.set_dense_threshold(1)
    try:
        x = tp.T(sr[None], dev).clone().requires_grad_(True)
        el = engine.edge_list(mask=tp.T(mask[None, None], dev), ks=ks, capacity=n + 64)
        assert int(el.counts[0]) == n
        plan = el.plan[:4].cpu().numpy()
        tiles = int(plan[1]) + int(plan[3])
        assert tiles == large25["tiles"] and int(plan[0]) == 0, f"plan holds {tiles} dense tiles, predicted {large25['tiles']}"
        parts = fr.offset_parts(tiles, cus, ks)
        assert parts == 1 == large25["parts"], f"{cus} CUs split {tiles} tiles {parts} ways"
        s = engine.ssg_map(x, el.edges, el.counts, n, ks, kw, SIGMA, order=el.order, fwd=el.fwd, deterministic=True)
        (s * tp.T(cot.reshape(n, -1), dev)).sum().backward()
        g1 = x.grad[0].clone()
        err = tp.maxerr(g1.cpu(), gref) / np.abs(gref).max()
        report("k25-map", (H, W), tiles, parts, float(np.abs(gD).max()), reach, err, maxgrad=float(np.abs(gref).max()))
        assert tp.maxerr(s.detach().cpu(), S) <= 1e-5
        assert err <= 1e-5
    finally:
        engine.set_dense_threshold(prev)


def test_k25_loss_step_margin_under_the_a_priori_bound(dev, cus, large25):
    """A (25,9) loss step takes its scale from the a-priori bound of |G| (loss_grad_bound: 4 kfac (w_l1 + w_kl) / (N P)),
    far above the true maximum at sigma 1: the same step-edge image at qs = 1 converts values of about 2^38.5 -- printed
    as documentation of the margin; gradient against the fp64 oracle at the rule the (25,9) loss tests use
    (grad_tol_from_oracle), second run bit for bit."""
    from ssl_amd import engine
    ks, kw = 25, 9
    sr, gt, mask = large25["sr"], large25["gt"], large25["mask"]
    H, W = mask.shape
    case = _loss_case(sr, gt, mask, ks, kw, large25["tiles"], cus)
    ref, N = case["ref"], int(mask.sum())
    bound = np.float32(4.0 / (SIGMA * 3 * kw * kw) * 2e3 / (N * ks * ks))
    bits = float(np.log2(case["reach"] * np.abs(ref["gD"]).max() * fr.fix_scale(bound)))
    prev = engine.set_dense_threshold(1)
    try:
        step = engine.LossStep(1, 3, H, W, ks, kw, SIGMA, 1e-10, True, 1e3, 1e3, device=dev, deterministic=True, capacity=N + 64)
        args = (tp.T(sr[None], dev), tp.T(gt[None], dev), tp.T(mask[None, None], dev))
        loss, grad = step(*args)
        loss, grad = loss.clone(), grad.clone()
        n = int(step.counts[0])
        tiles, sparse, _ = plan_counts(step)
        assert n == N and tiles == large25["tiles"] and sparse == 0 and fr.offset_parts(tiles, cus, ks) == 1
        gref, nflip = tp.ref_grad_with_gpu_signs(sr[None], mask[None], ks, kw, SIGMA, ref, step.ssg_sr[:n].cpu().numpy(),
                                                 step.ssg_gt[:n].cpu().numpy())
        err = tp.maxerr(grad.cpu(), gref) / np.abs(gref).max()
        report("k25-loss-apriori", (H, W), tiles, 1, float(np.abs(ref["gD"]).max()), case["reach"], err,
               bound=float(bound), converted_bits=bits, sign_ties=nflip)
        assert bits < 51.0
        assert err * np.abs(gref).max() <= tp.grad_tol_from_oracle(sr[None], gt[None], mask[None], ks, kw, SIGMA, ref)
        loss2, grad2 = step(*args)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    finally:
        engine.set_dense_threshold(prev)
