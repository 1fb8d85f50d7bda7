"""The diffusion kernels (ssl_amd/csrc/ssg_diffusion.hip) on the GPU against tests/diffusion_reference.py: the per-sample
combinations, p_sample, the canvas gather and stitch and the splitter BIT FOR BIT against torch's lines on the CPU (and,
for the canvas and the splitter, against what the reference itself recorded, tests/golden/f36_diffusion.npz); the
training criterion within its derived bound around the fp64 restatement, whose gradients are torch.autograd's."""
import pytest
import torch

import diffusion_cases as C
import diffusion_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fix(golden):
    return golden("f36_diffusion")


@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    from ssl_amd import _lib
    return _lib.lib()


_SCHEDULES = {}


def schedule(name="linear_eps", p2=False, **over):
    """(the schedule on the GPU, its tables on the CPU by name with sigma and p2 as the GPU made them)"""
    from ssl_amd.diffusion import Schedule
    key = (name, p2, tuple(sorted(over.items())))
    if key not in _SCHEDULES:
        s = Schedule(**dict(C.SCHEDULES[name], **over), **(C.P2 if p2 else {}), device=DEV)
        tab = {b: getattr(s, b).cpu() for b in C.BUFFERS}
        tab["sigma"], tab["p2"] = s.sigma.cpu(), None if s.p2 is None else s.p2.cpu()
        _SCHEDULES[key] = (s, tab)
    return _SCHEDULES[key]


def on_gpu(view, offset):
    """A CPU (B, 1, 1, n) tensor as a contiguous GPU tensor that starts `offset` floats into its storage."""
    flat = torch.empty(view.numel() + 3, dtype=view.dtype, device=DEV)
    out = flat[offset:offset + view.numel()].view(view.shape)
    out.copy_(view)
    assert out.data_ptr() % 16 == (4 * offset) % 16
    return out


def shapes(lib):
    return [(B, n) for B in C.BATCHES for n in C.sample_counts(lib.ssg_diff_chunk())]


def _inputs(B, n, seed, specials=True):
    """three CPU (B, 1, 1, n) tensors, their GPU copies at offsets that differ from tensor to tensor, and t"""
    cpu = [v.view(B, 1, 1, n) for v in C.sample_inputs(B, n, seed, specials)]
    gpu = [on_gpu(v, (seed + 1 + 3 * j) % 4) for j, v in enumerate(cpu)]
    return cpu, gpu


# ------------------------------------------------------------------------------------------------- section 2 ---
@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("which", range(6))
def test_combinations_and_p_sample_are_torchs_bits(lib, B, which):
    n = C.sample_counts(lib.ssg_diff_chunk())[which]
    s, tab = schedule()
    (a, b, z), (ga, gb, gz) = _inputs(B, n, 10 * B + which)
    t = C.timesteps(B, 1000, which)
    gt = t.to(DEV)
    pairs = [(s.q_sample(ga, gt, gb), R.combine(tab["sqrt_alphas_cumprod"], a, tab["sqrt_one_minus_alphas_cumprod"], b, t, False)),
             (s.get_v(ga, gb, gt), R.combine(tab["sqrt_alphas_cumprod"], b, tab["sqrt_one_minus_alphas_cumprod"], a, t, True)),
             (s.predict_start_from_noise(ga, gt, gb),
              R.combine(tab["sqrt_recip_alphas_cumprod"], a, tab["sqrt_recipm1_alphas_cumprod"], b, t, True)),
             (s.predict_start_from_z_and_v(ga, gb, gt),
              R.combine(tab["sqrt_alphas_cumprod"], a, tab["sqrt_one_minus_alphas_cumprod"], b, t, True)),
             (s.q_posterior(ga, gb, gt)[0], R.combine(tab["posterior_mean_coef1"], a, tab["posterior_mean_coef2"], b, t, False))]
    for k, (got, want) in enumerate(pairs):
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert R.same_bits(got, want) == 0, k
    for param in ("eps", "x0", "v"):
        sp, tp = schedule("linear_eps", parameterization=param)
        for clip in (False, True):
            want, want0 = R.p_sample(tp, a, b, t, z, param, clip, return_x0=True)
            got, got0 = sp.p_sample(ga, gb, gt, gz, clip_denoised=clip, return_x0=True)
            assert R.same_bits(got, want) == 0 and R.same_bits(got0, want0) == 0, (param, clip)
            assert R.same_bits(sp.p_sample(ga, gb, gt, gz, clip_denoised=clip), want) == 0, (param, clip)
    assert torch.equal(gb.cpu().view(torch.int32), b.view(torch.int32))         # (x0's clamp_ did not reach the input)


def test_every_workgroup_makes_a_second_trip(lib):
    """One sample of 2 grid_cap + 1 chunks, the last of 5 elements, offsets 1, 2, 3: the grid-stride trips of every
    kernel built on the chunk schedule."""
    from ssl_amd import diffusion
    n = C.second_trip_count(lib.ssg_diff_chunk(), lib.ssg_diff_grid_cap())
    assert lib.ssg_diff_workspace_bytes(1, n) == 8 * (2 * lib.ssg_diff_grid_cap() + 1)
    s, tab = schedule()
    (a, b, z), (ga, gb, gz) = _inputs(1, n, 2, specials=False)
    t = torch.tensor([617])
    gt = t.to(DEV)
    want = R.combine(tab["sqrt_alphas_cumprod"], a, tab["sqrt_one_minus_alphas_cumprod"], b, t, False)
    assert R.same_bits(s.q_sample(ga, gt, gb), want) == 0
    want, want0 = R.p_sample(tab, a, b, t, z, "eps", True, return_x0=True)
    got, got0 = s.p_sample(ga, gb, gt, gz, clip_denoised=True, return_x0=True)
    assert R.same_bits(got, want) == 0 and R.same_bits(got0, want0) == 0
    logvar = C.logvar_table(1000, 1)
    p = ga.detach().requires_grad_(True)
    loss, x0, _ = diffusion.p_losses_criterion(p, gb, gz, gt, s, logvar.to(DEV), "l2", 1.0, 0.5)
    loss.backward()
    ref = R.criterion64(a, b, z, t, tab, logvar, "l2", 1.0, 0.5)
    b_scal, b_grad, _, Rm = R.criterion_bounds(ref, "l2", 1.0, 0.5)
    assert R.share(loss, ref["scalars"][3], b_scal[3]) <= 1.0
    assert R.share(p.grad, ref["grad_pred"], b_grad) <= 1.0
    assert R.share(diffusion.loss_sums(ga, gb, "l2"), ref["S"], Rm * ref["S"]) <= 1.0
    assert R.same_bits(x0, R.combine(tab["sqrt_recip_alphas_cumprod"], z, tab["sqrt_recipm1_alphas_cumprod"], a, t, True)) == 0


def test_t_outside_the_table_reads_nothing_and_gives_nan(lib):
    s, tab = schedule("linear_v")
    (a, b, _), (ga, gb, _) = _inputs(3, 7, 5, specials=False)
    t = torch.tensor([3, 40, -1])                      # T = 40
    got = s.q_sample(ga, t.to(DEV), gb).cpu()
    want = R.combine(tab["sqrt_alphas_cumprod"], a[:1], tab["sqrt_one_minus_alphas_cumprod"], b[:1], t[:1], False)
    assert R.same_bits(got[:1], want) == 0 and bool(torch.isnan(got[1:]).all())


def test_other_dtypes_and_the_switch_take_torchs_lines(lib):
    from ssl_amd.losses import set_native_criteria
    s, tab = schedule()
    (a, b, _), (ga, gb, _) = _inputs(2, 33, 6, specials=False)
    t = C.timesteps(2, 1000).to(DEV)
    lines = lambda x, y: (s.sqrt_alphas_cumprod[t].view(2, 1, 1, 1) * x + s.sqrt_one_minus_alphas_cumprod[t].view(2, 1, 1, 1) * y)
    prev = set_native_criteria(False)
    try:
        assert torch.equal(s.q_sample(ga, t, gb), lines(ga, gb))
    finally:
        set_native_criteria(prev)
    h = s.q_sample(ga.half(), t, gb.half())
    assert h.dtype == lines(ga.half(), gb.half()).dtype and torch.equal(h, lines(ga.half(), gb.half()))
    x = ga.detach().requires_grad_(True)                 # in a graph: torch's lines, differentiable
    s.q_sample(x, t, gb).sum().backward()
    assert torch.equal(x.grad, s.sqrt_alphas_cumprod[t].view(2, 1, 1, 1).expand_as(x))
    with pytest.raises(RuntimeError):
        s.q_sample(a, C.timesteps(2, 1000), b)           # CPU tensors, a schedule on the GPU


def test_strided_t_and_logvar_are_read_as_tensors(lib):
    """t and logvar reach the kernels as addresses: views with a stride must give the values of the view."""
    from ssl_amd import diffusion
    s, tab = schedule(p2=True)
    (a, b, z), (ga, gb, gz) = _inputs(3, 41, 9, specials=False)
    t = C.timesteps(3, 1000, 9)
    wide = torch.stack([t, (t + 500) % 1000], 1).flatten().to(DEV)
    gt = wide[::2]
    assert not gt.is_contiguous() and torch.equal(gt.cpu(), t)
    want = R.combine(tab["sqrt_alphas_cumprod"], a, tab["sqrt_one_minus_alphas_cumprod"], b, t, False)
    assert R.same_bits(s.q_sample(ga, gt, gb), want) == 0
    assert R.same_bits(s.p_sample(ga, gb, gt, gz), R.p_sample(tab, a, b, t, z, "eps", False)) == 0
    logvar = C.logvar_table(1000, 9)
    lv2 = torch.stack([logvar, -logvar], 1).to(DEV)[:, 0]
    assert not lv2.is_contiguous()
    got = diffusion.p_losses_criterion(ga, gb, gz, gt, s, lv2, "l2", 1.0, 0.5)
    ref = diffusion.p_losses_criterion(ga, gb, gz, t.to(DEV), s, logvar.to(DEV), "l2", 1.0, 0.5)
    assert R.same_bits(got[0], ref[0].cpu()) == 0 and R.same_bits(got[1], ref[1].cpu()) == 0


# ------------------------------------------------------------------------------------------------- section 3 ---
def _criterion(lib, B, n, seed, loss_type, p2, elbo, learn, with_x0, capsys=None, lsw=1.0, upstream=1.0):
    from ssl_amd import diffusion
    s, tab = schedule(p2=p2)
    (pred, target, xn), (gp, gt_, gx) = _inputs(B, n, seed, specials=False)
    gx0 = C.sample_inputs(B, n, seed + 50, specials=False, count=1)[0].view(B, 1, 1, n) * 1e-3 if with_x0 else None
    t = C.timesteps(B, 1000, seed)
    logvar = C.logvar_table(1000, seed)

    def run():
        p = gp.detach().requires_grad_(True)
        lv = logvar.to(DEV).requires_grad_(learn)
        loss, x0, logged = diffusion.p_losses_criterion(p, gt_, gx, t.to(DEV), s, lv, loss_type, lsw, elbo)
        total = upstream * loss
        if with_x0:
            total = total + (on_gpu(gx0, 2) * x0).sum()
        total.backward()
        return loss.detach(), x0.detach(), p.grad, lv.grad, logged

    loss, x0, grad, glv, logged = run()
    ref = R.criterion64(pred, target, xn, t, tab, logvar, loss_type, lsw, elbo, tab["p2"], upstream, gx0)
    b_scal, b_grad, per, Rm = R.criterion_bounds(ref, loss_type, lsw, elbo, upstream, gx0)
    shares = dict(simple=R.share(logged["train/loss_simple"], ref["scalars"][0], b_scal[0]),
                  vlb=R.share(logged["train/loss_vlb"], ref["scalars"][2], b_scal[2]),
                  loss=R.share(loss, ref["scalars"][3], b_scal[3]), grad=R.share(grad, ref["grad_pred"], b_grad))
    assert R.same_bits(logged["train/loss"], loss.cpu()) == 0 and loss.dtype == torch.float32 and loss.dim() == 0
    if learn:
        shares["gamma"] = R.share(logged["train/loss_gamma"], ref["scalars"][1], b_scal[1])
        shares["dlogvar"] = R.share(glv, ref["grad_logvar"], R.logvar_bound(per, t, 1000, ref["grad_logvar"]))
        assert int((glv != 0).sum()) <= len(set(t.tolist()))
    else:
        assert glv is None and "train/loss_gamma" not in logged
    if capsys is not None:
        with capsys.disabled():
            print(f"\n  kernels B={B} n={n} {loss_type} p2={p2} elbo={elbo} learn={learn} x0={with_x0}: shares "
                  + " ".join(f"{k}={v:.3f}" for k, v in shares.items()))
    assert max(shares.values()) <= 1.0, shares
    want0 = R.combine(tab["sqrt_recip_alphas_cumprod"], xn, tab["sqrt_recipm1_alphas_cumprod"], pred, t, True)
    assert R.same_bits(x0, want0) == 0
    # a repeated call gives the same bits
    again = run()
    for u, v in zip((loss, x0, grad, glv), again[:4]):
        assert (u is None and v is None) or R.same_bits(u, v.cpu()) == 0
    assert all(R.same_bits(logged[k], again[4][k].cpu()) == 0 for k in logged)
    # sample b of the batch is the sample alone (at another address, so at another alignment)
    S = diffusion.loss_sums(gp, gt_, loss_type)
    assert R.share(S, ref["S"], Rm * ref["S"]) <= 1.0
    for b in range(B):
        alone = diffusion.loss_sums(gp[b:b + 1].clone(), gt_[b:b + 1].clone(), loss_type)
        assert R.same_bits(alone, S[b:b + 1].cpu()) == 0, b
    return shares


@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("which", range(6))
def test_criterion_meets_its_bound_on_every_shape(lib, B, which, capsys):
    n = C.sample_counts(lib.ssg_diff_chunk())[which]
    k = 6 * C.BATCHES.index(B) + which
    _criterion(lib, B, n, 20 + k, "l1", bool(k & 1), 0.5 * ((k >> 1) & 1), bool((k >> 2) & 1), bool((k >> 3) & 1), capsys)
    _criterion(lib, B, n, 60 + k, "l2", not (k & 1), 0.5 * (1 - ((k >> 1) & 1)), not ((k >> 2) & 1), not ((k >> 3) & 1), capsys)


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_criterion_options_crossed(lib, loss_type, capsys):
    n = lib.ssg_diff_chunk() + 1
    for k in range(16):
        _criterion(lib, 3, n, 100 + k, loss_type, bool(k & 1), 0.5 * ((k >> 1) & 1), bool((k >> 2) & 1), bool((k >> 3) & 1),
                   capsys, lsw=0.7, upstream=1.5)


def test_a_nan_reaches_the_loss_and_its_own_sample_only(lib):
    from ssl_amd import diffusion
    s, tab = schedule()
    (pred, target, xn), (gp, gt_, gx) = _inputs(3, 50, 7, specials=False)
    gp[1, 0, 0, 17] = float("nan")
    t = C.timesteps(3, 1000, 7).to(DEV)
    p = gp.detach().requires_grad_(True)
    loss, x0, logged = diffusion.p_losses_criterion(p, gt_, gx, t, s, C.logvar_table(1000).to(DEV), "l2")
    loss.backward()
    assert bool(torch.isnan(loss)) and all(bool(torch.isnan(v)) for v in logged.values())
    S = diffusion.loss_sums(gp, gt_, "l2").cpu()
    assert torch.isnan(S).tolist() == [False, True, False]
    assert int(torch.isnan(x0).sum()) == 1 and bool(torch.isnan(x0[1, 0, 0, 17]))
    g = p.grad.cpu()
    assert bool(torch.isfinite(g[0]).all()) and bool(torch.isfinite(g[2]).all()) and bool(torch.isnan(g[1, 0, 0, 17]))


def test_criterion_off_the_native_domain_takes_torchs_lines(lib):
    from ssl_amd import diffusion
    from ssl_amd.losses import set_native_criteria
    s, tab = schedule(p2=True)
    (pred, target, xn), (gp, gt_, gx) = _inputs(3, 40, 8, specials=False)
    t = C.timesteps(3, 1000, 8).to(DEV)
    lv = C.logvar_table(1000).to(DEV)
    prev = set_native_criteria(False)
    try:
        loss, x0, logged = diffusion.p_losses_criterion(gp, gt_, gx, t, s, lv, "l1", 1.0, 0.5)
    finally:
        set_native_criteria(prev)
    want = diffusion._criterion_torch(gp, gt_, gx, t, s, lv, "l1", 1.0, 0.5)
    assert torch.equal(loss, want[0]) and torch.equal(x0, want[1])
    native = diffusion.p_losses_criterion(gp, gt_, gx, t, s, lv, "l1", 1.0, 0.5)
    assert abs(float(native[0]) - float(loss)) <= 1e-5 * abs(float(loss))


# ------------------------------------------------------------------------------------------------- section 4 ---
@pytest.mark.parametrize("case", C.CANVAS)
@pytest.mark.parametrize("B", C.CANVAS_BATCHES)
def test_canvas_gather_stitch_and_step_are_the_references_bits(lib, fix, case, B):
    from ssl_amd import diffusion
    ts, overlap, h, w = case
    tiles, grid = diffusion.canvas_tiles(h, w, ts, overlap)
    x, sc = C.canvas_inputs(case, B)
    gx, gsc = x.to(DEV), sc.to(DEV)
    tx, tc = diffusion.canvas_gather(gx, tiles, ts), diffusion.canvas_gather(gsc, tiles, ts)
    assert R.same_bits(tx, R.canvas_gather(x, tiles, ts)) == 0 and R.same_bits(tc, R.canvas_gather(sc, tiles, ts)) == 0
    preds = C.stand_in_network(tx, tc)
    weights = diffusion.gaussian_weights(ts, ts, B, C.CANVAS_C, device=DEV)
    w_cpu = weights.cpu()
    # the reference's own indexing of its prediction list (for B = 1 the same as one tile per sample)
    want = R.canvas_stitch(preds.cpu(), tiles, x.shape, w_cpu, sources=R.reference_sources(grid, B))
    got = diffusion.canvas_stitch(preds, tiles, x.shape, weights, grid, per_sample=False)
    assert R.same_bits(got, want) == 0
    name = C.canvas_name(case, B)
    recorded = name + "_stitched" in fix.files
    assert recorded or B not in C.CANVAS_FIXTURE_B.get(case, C.CANVAS_BATCHES)
    if recorded:
        assert R.same_bits(got, torch.from_numpy(fix[name + "_stitched"])) == 0
    # one tile per sample, one (ts, ts) plane of weights, and the unweighted average
    assert R.same_bits(diffusion.canvas_stitch(preds, tiles, x.shape, weights[0, 0]), R.canvas_stitch(preds.cpu(), tiles, x.shape, w_cpu)) == 0
    assert R.same_bits(diffusion.canvas_stitch(preds, tiles, x.shape), R.canvas_stitch(preds.cpu(), tiles, x.shape, None)) == 0
    # the whole step against the reference-order lines
    s, tab = schedule()
    t = torch.full((B,), 17, dtype=torch.int64)
    noise = C.canvas_inputs(case, B, seed=5)[0]
    out, x0 = diffusion.p_sample_canvas_step(s, C.stand_in_network, gx, gsc, t.to(DEV), noise.to(DEV), ts, overlap, weights,
                                             clip_denoised=True, return_x0=True, per_sample=False)
    want_out, want_x0 = R.p_sample(tab, x, want, t, noise, "eps", True, return_x0=True)
    assert R.same_bits(out, want_out) == 0 and R.same_bits(x0, want_x0) == 0
    if recorded:
        quiet = diffusion.p_sample_canvas_step(s, C.stand_in_network, gx, gsc, t.to(DEV), torch.zeros_like(gx), ts, overlap,
                                               weights, clip_denoised=True, per_sample=False)
        assert R.same_bits(quiet, torch.from_numpy(fix[name + "_mean"])) == 0


@pytest.mark.parametrize("case", C.SPLITTER)
def test_splitter_is_the_references_bits(lib, fix, case):
    from ssl_amd.diffusion import ImageSpliterTh
    h, w, patch, stride, sf = case
    sp = ImageSpliterTh(C.splitter_input(case).to(DEV), patch, stride, sf=sf)
    for k, (pch, info) in enumerate(sp):
        assert pch.is_cuda
        sp.update(C.splitter_patch_result(pch, sf, k), info)
    out = sp.gather()
    assert out.is_cuda and R.same_bits(out, torch.from_numpy(fix[C.splitter_name(case) + "_out"])) == 0
