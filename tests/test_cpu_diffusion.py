"""What of the diffusion fork's pieces (ssl_amd/diffusion.py, ssl_amd/csrc/ssg_diffusion.hip) can be checked without a
device: the schedule, its respacing, the canvas geometry, the Gaussian weights and the splitter against what the
reference itself recorded (tests/golden/f36_diffusion.npz, written by make_golden_diffusion.py); the oracles of
tests/diffusion_reference.py against the same recordings; the Python API on CPU tensors (the reference's torch lines),
bit for bit; the bound of the criterion on torch's own fp32 lines; every refusal of the C ABI; and that the order of the
stitch is observable."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import diffusion_cases as C
import diffusion_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ssg_diff_chunk", "ssg_diff_grid_cap", "ssg_diff_workspace_bytes", "ssg_diff_combine", "ssg_diff_p_sample",
         "ssg_diff_loss_sums", "ssg_diff_loss_finish", "ssg_diff_loss_grad", "ssg_diff_canvas_gather",
         "ssg_diff_canvas_stitch")


@pytest.fixture(scope="module")
def fix(golden):
    return golden("f36_diffusion")


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- section 1 ----
@pytest.mark.parametrize("name", sorted(C.SCHEDULES))
def test_schedule_tables_are_the_references_bits(fix, name):
    from ssl_amd.diffusion import Schedule
    s = Schedule(**C.SCHEDULES[name])
    for b in C.BUFFERS:
        got = getattr(s, b)
        assert got.dtype == torch.float32 and got.shape == (s.num_timesteps,)
        assert _bits_equal(got.numpy(), fix[f"sched_{name}_{b}"]), b
    assert bool(s.lvlb_weights[0] == s.lvlb_weights[1])
    kw = dict(C.SCHEDULES[name])
    restated = R.schedule_tables(R.beta_schedule(kw.pop("beta_schedule"), kw.pop("timesteps"),
                                                 **{k: v for k, v in kw.items() if k in ("linear_start", "linear_end", "cosine_s")}),
                                 kw["parameterization"], kw["v_posterior"])
    for b in C.BUFFERS:
        assert _bits_equal(restated[b].numpy(), fix[f"sched_{name}_{b}"]), b
    assert _bits_equal(s.sigma.numpy(), (0.5 * s.posterior_log_variance_clipped).exp().numpy()) and s.p2 is None


def test_p2_table_and_unknown_names():
    from ssl_amd.diffusion import Schedule, make_beta_schedule
    s = Schedule(**C.SCHEDULES["linear_eps"], **C.P2)
    snr = 1.0 / (1 - s.alphas_cumprod) - 1
    assert _bits_equal(s.p2.numpy(), (1 / (C.P2["p2_k"] + snr) ** C.P2["p2_gamma"]).numpy())
    with pytest.raises(ValueError):
        make_beta_schedule("quadratic", 10)
    with pytest.raises(NotImplementedError):
        Schedule(parameterization="mu")


@pytest.mark.parametrize("steps", C.RESPACED)
def test_respacing_is_the_references_bits(fix, steps):
    from ssl_amd.diffusion import Schedule, space_timesteps
    s = Schedule(**C.SCHEDULES["linear_eps"]).respaced(steps)
    assert s.num_timesteps == steps and s.ori_timesteps == fix[f"respaced_{steps}_steps"].tolist()
    assert s.ori_timesteps == sorted(space_timesteps(1000, [steps]))
    for b in C.BUFFERS:
        assert _bits_equal(getattr(s, b).numpy(), fix[f"respaced_{steps}_{b}"]), b
    base = R.schedule_tables(R.beta_schedule("linear", 1000, 0.00085, 0.0120))
    restated = R.schedule_tables(R.respaced_betas(base["alphas_cumprod"], s.ori_timesteps))
    for b in C.BUFFERS:
        assert _bits_equal(restated[b].numpy(), fix[f"respaced_{steps}_{b}"]), b
    if steps == 1000:
        # every step is kept, and still the tables are not the original ones: the new betas come from float32 quotients
        assert not _bits_equal(s.betas.numpy(), Schedule(**C.SCHEDULES["linear_eps"]).betas.numpy())


def test_space_timesteps_forms():
    from ssl_amd.diffusion import space_timesteps
    assert space_timesteps(300, [10, 15, 20]) == space_timesteps(300, "10,15,20") and len(space_timesteps(300, [10, 15, 20])) == 45
    assert space_timesteps(100, "ddim25") == set(range(0, 100, 4))
    with pytest.raises(ValueError):
        space_timesteps(10, [11])
    with pytest.raises(ValueError):
        space_timesteps(100, "ddim33")


# ---- section 2 on the CPU: the reference's lines ----
def test_combinations_on_cpu_are_the_recorded_results(fix):
    from ssl_amd.diffusion import Schedule
    s = Schedule(**C.SCHEDULES["linear_eps"])
    tab = {b: getattr(s, b) for b in C.BUFFERS}
    a, b, _ = (v.view(3, 1, 1, 37) for v in C.sample_inputs(3, 37, 0))
    t = C.timesteps(3, 1000)
    got = dict(q_sample=s.q_sample(a, t, b), get_v=s.get_v(a, b, t), predict_start_from_noise=s.predict_start_from_noise(a, t, b),
               predict_start_from_z_and_v=s.predict_start_from_z_and_v(a, b, t), q_posterior=s.q_posterior(a, b, t)[0])
    want = dict(q_sample=R.combine(tab["sqrt_alphas_cumprod"], a, tab["sqrt_one_minus_alphas_cumprod"], b, t, False),
                get_v=R.combine(tab["sqrt_alphas_cumprod"], b, tab["sqrt_one_minus_alphas_cumprod"], a, t, True),
                predict_start_from_noise=R.combine(tab["sqrt_recip_alphas_cumprod"], a, tab["sqrt_recipm1_alphas_cumprod"], b, t, True),
                predict_start_from_z_and_v=R.combine(tab["sqrt_alphas_cumprod"], a, tab["sqrt_one_minus_alphas_cumprod"], b, t, True),
                q_posterior=R.combine(tab["posterior_mean_coef1"], a, tab["posterior_mean_coef2"], b, t, False))
    for k in got:
        recorded = torch.from_numpy(fix["combine_" + k])
        assert R.same_bits(got[k], recorded) == 0 and R.same_bits(want[k], recorded) == 0, k
    mean, var, logvar = s.q_posterior(a, b, t)
    assert var.shape == logvar.shape == (3, 1, 1, 1) and torch.equal(var.flatten(), s.posterior_variance[t])


@pytest.mark.parametrize("param", ["eps", "x0", "v"])
@pytest.mark.parametrize("clip", [False, True])
def test_p_sample_on_cpu_is_the_oracle(param, clip):
    from ssl_amd.diffusion import Schedule
    s = Schedule(**dict(C.SCHEDULES["linear_v"], parameterization=param))
    tab = dict({b: getattr(s, b) for b in C.BUFFERS}, sigma=s.sigma)
    x, m, z = (v.view(3, 1, 1, 29) for v in C.sample_inputs(3, 29, 3))
    t = C.timesteps(3, s.num_timesteps)
    want, want0 = R.p_sample(tab, x, m, t, z, param, clip, return_x0=True)
    got, got0 = s.p_sample(x, m.clone(), t, z, clip_denoised=clip, return_x0=True)
    assert R.same_bits(got, want) == 0 and R.same_bits(got0, want0) == 0
    assert R.same_bits(s.p_sample(x, m.clone(), t, z, clip_denoised=clip), want) == 0
    # sample 0 has t = 0: no noise reaches it
    quiet = R.p_sample(tab, x, m, t, torch.zeros_like(z), param, clip)
    finite = torch.isfinite(want[0]) & torch.isfinite(z[0])
    assert torch.equal(want[0][finite], quiet[0][finite])


def test_t_is_checked_on_the_host_only_where_it_lives_there():
    from ssl_amd.diffusion import Schedule
    s = Schedule(**C.SCHEDULES["linear_v"])
    x = torch.zeros(2, 1, 1, 4)
    for bad in (torch.tensor([0, 40]), torch.tensor([-1, 3])):
        with pytest.raises(IndexError):
            s.q_sample(x, bad, x)
    with pytest.raises(ValueError):
        s.q_sample(x, torch.tensor([0, 1], dtype=torch.int32), x)
    with pytest.raises(ValueError):
        s.q_sample(x, torch.tensor([0, 1, 2]), x)


# ---- section 3 ----
def _criterion_case(B, n, loss_type, p2, seed):
    from ssl_amd.diffusion import Schedule
    s = Schedule(**C.SCHEDULES["linear_eps"], **(C.P2 if p2 else {}))
    tab = {b: getattr(s, b) for b in C.BUFFERS}
    pred, target, xn = (v.view(B, 1, 1, n) for v in C.sample_inputs(B, n, seed, specials=False))
    gx0 = C.sample_inputs(B, n, seed + 50, specials=False, count=1)[0].view(B, 1, 1, n) * 1e-3
    return s, tab, pred, target, xn, gx0, C.timesteps(B, 1000, seed), C.logvar_table(1000, seed)


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("p2", [False, True])
@pytest.mark.parametrize("elbo", [0.0, 0.5])
def test_torchs_fp32_lines_meet_the_criterions_bound(loss_type, p2, elbo, capsys):
    s, tab, pred, target, xn, gx0, t, logvar = _criterion_case(5, 263, loss_type, p2, 11)
    ref = R.criterion64(pred, target, xn, t, tab, logvar, loss_type, 1.0, elbo, s.p2, grad_x0=gx0)
    b_scal, b_grad, per, _ = R.criterion_bounds(ref, loss_type, 1.0, elbo, grad_x0=gx0, torch32=True)
    got = R.criterion_torch32(pred, target, xn, t, tab, logvar, loss_type, 1.0, elbo, s.p2, grad_x0=gx0)
    shares = [R.share(got["scalars"][k], ref["scalars"][k], b_scal[k]) for k in range(4)]
    shares.append(R.share(got["grad_pred"], ref["grad_pred"], b_grad))
    shares.append(R.share(got["grad_logvar"], ref["grad_logvar"], R.logvar_bound(per, t, 1000)))
    # the kernels' bound is the narrower one everywhere
    k_scal, k_grad, k_per, _ = R.criterion_bounds(ref, loss_type, 1.0, elbo, grad_x0=gx0)
    assert all(k < b for k, b in zip(k_scal, b_scal)) and bool((k_grad <= b_grad).all()) and bool((k_per < per).all())
    with capsys.disabled():
        print(f"\n  torch fp32 {loss_type} p2={p2} elbo={elbo}: shares of the bound simple/gamma/vlb/loss/grad/dlogvar = "
              + " ".join(f"{v:.3f}" for v in shares))
    assert max(shares) <= 1.0, shares
    # x0 is not a matter of bounds
    want = R.combine(tab["sqrt_recip_alphas_cumprod"], xn, tab["sqrt_recipm1_alphas_cumprod"], pred, t, True)
    assert R.same_bits(got["x0"], want) == 0


def test_the_restatements_gradients_are_the_closed_forms():
    """criterion64 differentiates with autograd; the kernels use closed forms.  The two agree to fp64's precision."""
    s, tab, pred, target, xn, gx0, t, logvar = _criterion_case(5, 64, "l2", True, 12)
    lsw, elbo, g = 0.7, 0.5, 1.5
    r = R.criterion64(pred, target, xn, t, tab, logvar, "l2", lsw, elbo, s.p2, upstream=g, grad_x0=gx0)
    B, n = 5, 64
    coef = (lsw * r["w"] / r["e"] + elbo * r["vw"]) / B
    want = g * coef.view(B, 1, 1, 1) / n * (-2 * r["d"]) - r["rb"] * gx0.double()
    assert float((want - r["grad_pred"]).abs().max()) <= 1e-12 * float(want.abs().max())
    dlv = torch.zeros(1000, dtype=torch.float64).index_add_(0, t, g * lsw * (1 - r["w"] * r["m"] / r["e"]) / B)
    assert float((dlv - r["grad_logvar"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("learn", [False, True])
def test_criterion_on_cpu_is_the_references_lines(learn):
    from ssl_amd.diffusion import p_losses_criterion
    s, tab, pred, target, xn, gx0, t, logvar = _criterion_case(3, 37, "l2", True, 13)
    lv = torch.nn.Parameter(logvar.clone()) if learn else logvar
    p = pred.clone().requires_grad_(True)
    loss, x0, logged = p_losses_criterion(p, target, xn, t, s, lv, "l2", 1.0, 0.5)
    (loss + (gx0 * x0).sum()).backward()
    want = R.criterion_torch32(pred, target, xn, t, tab, logvar, "l2", 1.0, 0.5, s.p2, grad_x0=gx0)
    assert R.same_bits(loss.detach(), want["scalars"][3]) == 0 and R.same_bits(x0.detach(), want["x0"]) == 0
    assert R.same_bits(p.grad, want["grad_pred"]) == 0
    keys = ["train/loss_simple", "train/loss_gamma", "logvar", "train/loss_vlb", "train/loss"] if learn else \
        ["train/loss_simple", "train/loss_vlb", "train/loss"]
    assert list(logged) == keys and not any(v.requires_grad for v in logged.values())
    assert R.same_bits(logged["train/loss_simple"], want["scalars"][0]) == 0
    assert R.same_bits(logged["train/loss_vlb"], want["scalars"][2]) == 0
    if learn:
        assert R.same_bits(lv.grad, want["grad_logvar"]) == 0 and R.same_bits(logged["train/loss_gamma"], want["scalars"][1]) == 0
    with pytest.raises(NotImplementedError):
        p_losses_criterion(p, target, xn, t, s, lv, "huber")
    with pytest.raises(ValueError):
        p_losses_criterion(p, target, xn, t, s, lv[:10])


def test_the_p2_weight_is_the_references_broadcast():
    """ddpmssl.py:397-401 multiplies the (B,) loss_simple by a (B, 1, 1, 1) weight: the loss is (B, 1, 1, B) and every
    sample ends up weighted by the batch mean of the P2 weights.  The package's torch lines are that line's bits for
    B > 1, the fp64 restatement is its value, and the per-sample reading is observably something else."""
    from ssl_amd.diffusion import p_losses_criterion
    s, tab, pred, target, xn, gx0, t, logvar = _criterion_case(5, 37, "l2", True, 14)
    m = ((target - pred) ** 2).mean([1, 2, 3])
    weight = s.p2.gather(-1, t).reshape(5, 1, 1, 1)                      # extract_into_tensor(..., t, target.shape)
    lvt = logvar[t]
    line = weight * m / torch.exp(lvt) + lvt
    assert line.shape == (5, 1, 1, 5)
    p = pred.clone().requires_grad_(True)
    lv = torch.nn.Parameter(logvar.clone())
    loss, _, logged = p_losses_criterion(p, target, xn, t, s, lv, "l2", 1.0, 0.0)
    assert R.same_bits(loss.detach(), line.mean()) == 0 and R.same_bits(logged["train/loss_gamma"], line.mean()) == 0
    ref = R.criterion64(pred, target, xn, t, tab, logvar, "l2", 1.0, 0.0, s.p2)
    assert abs(float(ref["scalars"][3]) - float(line.double().mean())) <= 1e-5 * abs(float(line.mean()))
    wbar = s.p2[t].double().mean()
    assert abs(float(ref["scalars"][3]) - float((wbar * m.double() / lvt.double().exp() + lvt.double()).mean())) <= 1e-6
    per_sample = float((s.p2[t] * m / torch.exp(lvt) + lvt).mean())
    assert abs(per_sample - float(line.mean())) > 1e-3 * abs(float(line.mean()))
    loss.backward()
    want = R.criterion_torch32(pred, target, xn, t, tab, logvar, "l2", 1.0, 0.0, s.p2)
    assert R.same_bits(p.grad, want["grad_pred"]) == 0 and R.same_bits(lv.grad, want["grad_logvar"]) == 0


# ---- section 4 ----
@pytest.mark.parametrize("case", C.CANVAS)
def test_canvas_tiles_are_the_references(fix, case):
    from ssl_amd.diffusion import canvas_tiles
    ts, overlap, h, w = case
    tiles, grid = canvas_tiles(h, w, ts, overlap)
    assert (tiles, grid) == R.canvas_tiles(h, w, ts, overlap) and len(tiles) == grid[0] * grid[1]
    for B in C.CANVAS_FIXTURE_B.get(case, C.CANVAS_BATCHES):
        assert [tuple(v) for v in fix[C.canvas_name(case, B) + "_tiles"].tolist()] == tiles
    covered = np.zeros((h, w), dtype=bool)
    for oy, ox in tiles:
        assert 0 <= oy <= h - ts and 0 <= ox <= w - ts
        covered[oy:oy + ts, ox:ox + ts] = True
    assert covered.all()


def test_canvas_tiles_quirks_and_refusals():
    from ssl_amd.diffusion import canvas_tiles
    tiles, grid = canvas_tiles(19, 21, 8, 4)
    assert grid == (5, 4)                                   # `rows` count along the WIDTH (21), `cols` along the height
    assert tiles[0] == (0, 0) and tiles[1] == (4, 0) and tiles[3] == (11, 0)      # col is the inner loop and moves y
    assert tiles[-1] == (11, 13)                            # the corner keeps both snaps
    for h, w in ((7, 8), (8, 7), (0, 8)):
        with pytest.raises(ValueError):
            canvas_tiles(h, w, 8, 4)
    with pytest.raises(ValueError):
        canvas_tiles(16, 16, 8, 8)


def test_gaussian_weights_are_the_references(fix):
    from ssl_amd.diffusion import gaussian_weights
    for n in (8, 64):
        w = gaussian_weights(n, n, 2, C.CANVAS_C)
        assert w.dtype == torch.float64 and w.shape == (2, C.CANVAS_C, n, n)
        assert _bits_equal(w[1, 3].numpy(), fix[f"weights_{n}"]) and _bits_equal(R.gaussian_weights(n, n).numpy(), fix[f"weights_{n}"])
    w = gaussian_weights(8, 8)[0, 0]
    assert not torch.equal(w, w.flip(0)) and torch.equal(w, w.flip(1))      # the y midpoint is n / 2, x's (n - 1) / 2


def _canvas_oracle(case, B, order=None):
    ts, overlap, h, w = case
    tiles, grid = R.canvas_tiles(h, w, ts, overlap)
    x, sc = C.canvas_inputs(case, B)
    preds = C.stand_in_network(R.canvas_gather(x, tiles, ts), R.canvas_gather(sc, tiles, ts))
    weights = torch.tile(R.gaussian_weights(ts, ts), (B, C.CANVAS_C, 1, 1))
    return R.canvas_stitch(preds, tiles, x.shape, weights, sources=R.reference_sources(grid, B), order=order), preds


@pytest.mark.parametrize("case", C.CANVAS)
def test_stitch_oracle_and_cpu_path_are_the_recorded_results(fix, case):
    from ssl_amd import diffusion
    ts, overlap, h, w = case
    for B in C.CANVAS_FIXTURE_B.get(case, C.CANVAS_BATCHES):
        recorded = torch.from_numpy(fix[C.canvas_name(case, B) + "_stitched"])
        want, preds = _canvas_oracle(case, B)
        assert R.same_bits(want, recorded) == 0
        tiles, grid = diffusion.canvas_tiles(h, w, ts, overlap)
        x, sc = C.canvas_inputs(case, B)
        assert torch.equal(diffusion.canvas_gather(x, tiles, ts), R.canvas_gather(x, tiles, ts))
        weights = diffusion.gaussian_weights(ts, ts, B, C.CANVAS_C)
        got = diffusion.canvas_stitch(preds, tiles, x.shape, weights, grid, per_sample=False)
        assert R.same_bits(got, recorded) == 0
        # the whole step on the CPU: the recorded model_mean is p_sample without noise
        s = diffusion.Schedule(**C.SCHEDULES["linear_eps"])
        t = torch.full((B,), 17, dtype=torch.int64)
        out = diffusion.p_sample_canvas_step(s, C.stand_in_network, x, sc, t, torch.zeros_like(x), ts, overlap, weights,
                                             clip_denoised=True, return_x0=True, per_sample=False)
        assert R.same_bits(out[0], torch.from_numpy(fix[C.canvas_name(case, B) + "_mean"])) == 0
        if case not in C.CANVAS_FIXTURE_B:
            assert R.same_bits(out[1], torch.from_numpy(fix[C.canvas_name(case, B) + "_x0"])) == 0


def test_the_stitch_order_is_observable():
    """Accumulating in the reversed tile order changes bits where many tiles overlap, so a kernel that walked the tiles
    in another order could not pass; and the all-fp32 form of the add differs from torch's mixed-precision one."""
    case = C.CANVAS_HEAVY
    want, preds = _canvas_oracle(case, 1)
    ts, overlap, h, w = case
    tiles, grid = R.canvas_tiles(h, w, ts, overlap)
    backwards, _ = _canvas_oracle(case, 1, order=list(reversed(range(len(tiles)))))
    assert R.same_bits(backwards, want) > 0
    # the package's stitch follows the order of the tile list it is handed: reversed list, reversed oracle
    from ssl_amd import diffusion
    weights = diffusion.gaussian_weights(ts, ts, 1, C.CANVAS_C)
    flipped = list(reversed(tiles))
    flipped_preds = torch.cat([preds[k:k + 1] for k in reversed(range(len(tiles)))])
    assert R.same_bits(diffusion.canvas_stitch(flipped_preds, flipped, want.shape, weights), backwards) == 0
    assert R.same_bits(diffusion.canvas_stitch(preds, tiles, want.shape, weights), want) == 0
    w32 = R.gaussian_weights(ts, ts).float()
    acc, cnt = torch.zeros(1, C.CANVAS_C, h, w), torch.zeros(1, C.CANVAS_C, h, w)
    for k, (oy, ox) in enumerate(tiles):
        acc[:, :, oy:oy + ts, ox:ox + ts] += preds[k:k + 1] * w32
        cnt[:, :, oy:oy + ts, ox:ox + ts] += w32
    assert R.same_bits(acc / cnt, want) > 0


@pytest.mark.parametrize("case", C.SPLITTER)
def test_splitter_on_cpu_is_the_references(fix, case):
    from ssl_amd.diffusion import ImageSpliterTh
    h, w, patch, stride, sf = case
    im = C.splitter_input(case)
    sp = ImageSpliterTh(im, patch, stride, sf=sf)
    windows = []
    for k, (pch, info) in enumerate(sp):
        windows.append(info)
        sp.update(C.splitter_patch_result(pch, sf, k), info if k % 2 else None)
    name = C.splitter_name(case)
    assert windows == [tuple(v) for v in fix[name + "_windows"].tolist()] == R.splitter_windows(h, w, patch, stride, sf)
    assert len(sp) == len(windows) and R.same_bits(sp.gather(), torch.from_numpy(fix[name + "_out"])) == 0


# ---- the C ABI ----
def test_exports_declarations_and_bindings(L):
    from ssl_amd import _lib, diffusion
    with open(os.path.join(ROOT, "include", "ssg_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "ssl_amd", "csrc", "ssg_host.hpp")) as f:
        host = f.read()
    with open(os.path.join(ROOT, "ssl_amd", "csrc", "ssg_diffusion.hip")) as f:
        beside = f.read()
    for name in NAMES:
        assert name in _lib.PROTOTYPES and getattr(L, name).argtypes == _lib.PROTOTYPES[name][1], name
        assert re.search(r"\b%s\(" % name, header), name
        # every entry point is defined beside its kernels; nothing of the family crosses the host seam
        assert len(re.findall(r"^[a-z_ ]+\b%s\(" % name, beside, flags=re.M)) == 1, name
    assert "diff" not in host
    assert "ssg_diff_combine" in re.findall(r"/\* 6, additive:.*?\*/", header, flags=re.S)[-1]
    assert L.ssg_abi_version() == 6
    assert (diffusion.EPS, diffusion.X0, diffusion.V) == (0, 1, 2)
    chunk, cap = L.ssg_diff_chunk(), L.ssg_diff_grid_cap()
    assert chunk >= 4 and chunk % 4 == 0 and cap >= 1
    assert L.ssg_diff_workspace_bytes(3, 2 * chunk + 7) == 8 * 9 and L.ssg_diff_workspace_bytes(1, 1) == 8
    assert L.ssg_diff_workspace_bytes(0, 5) == L.ssg_diff_workspace_bytes(5, 0) == 0
    assert L.ssg_diff_workspace_bytes(2 ** 20, chunk << 12) == 0            # 2^32 chunks
    with open(os.path.join(ROOT, "ssl_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert " ssg_diffusion " in make and "ssg_diffusion.o prof/ssg_diffusion.o: EXTRA = -ffp-contract=off" in make


def test_every_refusal_is_decided_before_a_launch(L):
    """Host memory stands where the device's would: a call that passed its checks would launch on it, so every call here
    must be refused, and what it was handed must be untouched."""
    from ssl_amd import _lib
    E = {k: _lib.CONSTANTS["SSG_E_" + k] for k in ("BADARG", "TOOLARGE", "WORKSPACE", "ALIGN")}
    buf = np.full(64, 0x5a5a5a5a, dtype=np.uint32)
    before = buf.copy()
    p = buf.ctypes.data                       # 8-byte aligned at least
    assert p % 8 == 0
    chunk = L.ssg_diff_chunk()
    nan = float("nan")

    def combine(x=p, y=p, t=p, A=p, Bt=p, T=4, B=2, n=5, sub=0, clamp=0, lo=0.0, hi=0.0, out=p):
        return L.ssg_diff_combine(x, y, t, A, Bt, T, B, n, sub, clamp, lo, hi, out, None)
    for k in ("x", "y", "t", "A", "Bt", "out"):
        assert combine(**{k: None}) == E["BADARG"], k
    assert combine(T=0) == combine(B=0) == combine(n=0) == E["BADARG"]
    assert combine(clamp=1, lo=1.0, hi=-1.0) == combine(clamp=1, lo=nan, hi=1.0) == E["BADARG"]
    assert combine(B=2 ** 20, n=chunk << 12) == E["TOOLARGE"]
    for k in ("x", "y", "A", "Bt", "out"):
        assert combine(**{k: p + 2}) == E["ALIGN"], k
    assert combine(t=p + 4) == E["ALIGN"]

    def p_sample(x=p, m=p, z=p, t=p, ra=p, rb=p, c1=p, c2=p, sg=p, T=4, B=2, n=5, param=0, clip=0, out=p, x0=None):
        return L.ssg_diff_p_sample(x, m, z, t, ra, rb, c1, c2, sg, T, B, n, param, clip, out, x0, None)
    for k in ("x", "m", "z", "t", "c1", "c2", "sg", "out", "ra", "rb"):
        assert p_sample(**{k: None}) == E["BADARG"], k
    assert p_sample(param=-1) == p_sample(param=3) == p_sample(T=0) == p_sample(B=0) == p_sample(n=0) == E["BADARG"]
    assert p_sample(B=2 ** 20, n=chunk << 12) == E["TOOLARGE"]
    for k in ("x", "m", "z", "ra", "rb", "c1", "c2", "sg", "out", "x0"):
        assert p_sample(**{k: p + 1}) == E["ALIGN"], k
    assert p_sample(t=p + 4) == E["ALIGN"]

    def sums(pred=p, target=p, B=2, n=5, kind=0, ws=p, nbytes=16):
        return L.ssg_diff_loss_sums(pred, target, B, n, kind, ws, nbytes, None)
    assert sums(pred=None) == sums(target=None) == sums(ws=None) == sums(kind=2) == sums(kind=-1) == E["BADARG"]
    assert sums(B=0) == sums(n=0) == E["BADARG"] and sums(B=2 ** 20, n=chunk << 12) == E["TOOLARGE"]
    assert sums(nbytes=15) == E["WORKSPACE"] and sums(n=chunk + 1, nbytes=24) == E["WORKSPACE"]
    assert sums(pred=p + 2) == sums(target=p + 2) == sums(ws=p + 4) == E["ALIGN"]

    def finish(ws=p, nbytes=16, t=p, p2=None, lv=p, vw=p, T=4, B=2, n=5, lsw=1.0, elbo=0.0, S=p, sc=p, co=p, dl=None):
        return L.ssg_diff_loss_finish(ws, nbytes, t, p2, lv, vw, T, B, n, lsw, elbo, S, sc, co, dl, None)
    for k in ("ws", "t", "lv", "vw", "S", "sc", "co"):
        assert finish(**{k: None}) == E["BADARG"], k
    assert finish(lsw=nan) == finish(elbo=nan) == finish(T=0) == finish(B=0) == finish(n=0) == E["BADARG"]
    assert finish(nbytes=8) == E["WORKSPACE"] and finish(B=2 ** 20, n=chunk << 12) == E["TOOLARGE"]
    assert finish(B=2 ** 31, n=1, nbytes=2 ** 34) == E["TOOLARGE"]
    for k in ("ws", "t", "S", "sc", "co", "dl"):
        assert finish(**{k: p + 4}) == E["ALIGN"], k
    for k in ("p2", "lv", "vw"):
        assert finish(**{k: p + 2}) == E["ALIGN"], k

    def grad(pred=p, target=p, gx0=None, t=p, rb=p, T=4, g=p, coef=p, B=2, n=5, kind=1, out=p):
        return L.ssg_diff_loss_grad(pred, target, gx0, t, rb, T, g, coef, B, n, kind, out, None)
    for k in ("pred", "target", "g", "coef", "out"):
        assert grad(**{k: None}) == E["BADARG"], k
    assert grad(gx0=p, t=None) == grad(gx0=p, rb=None) == grad(gx0=p, T=0) == grad(kind=2) == grad(B=0) == grad(n=0) == E["BADARG"]
    for k in ("pred", "target", "gx0", "g", "out"):
        assert grad(**{k: p + 2}) == E["ALIGN"], k
    assert grad(coef=p + 4) == grad(gx0=p, t=p + 4) == E["ALIGN"]

    def gather(src=p, tiles=p, ntiles=2, B=1, C_=4, h=8, w=8, ts=8, out=p):
        return L.ssg_diff_canvas_gather(src, tiles, ntiles, B, C_, h, w, ts, out, None)
    assert gather(src=None) == gather(tiles=None) == gather(out=None) == E["BADARG"]
    for k in ("ntiles", "B", "C_", "h", "w", "ts"):
        assert gather(**{k: 0}) == E["BADARG"], k
    assert gather(ts=9) == gather(h=7) == gather(w=7) == E["BADARG"]
    assert gather(h=2 ** 16, w=2 ** 16) == gather(ntiles=2 ** 24, ts=8) == E["TOOLARGE"]
    assert gather(src=p + 2) == gather(tiles=p + 2) == gather(out=p + 2) == E["ALIGN"]

    def stitch(preds=p, n_preds=2, bstep=1, tiles=p, ntiles=2, wts=None, wsb=0, wsc=0, B=1, C_=4, h=8, w=8, ts=8, out=p):
        return L.ssg_diff_canvas_stitch(preds, n_preds, bstep, tiles, ntiles, wts, wsb, wsc, B, C_, h, w, ts, out, None)
    assert stitch(preds=None) == stitch(tiles=None) == stitch(out=None) == stitch(bstep=2) == stitch(bstep=-1) == E["BADARG"]
    assert stitch(n_preds=0) == stitch(ntiles=0) == stitch(ts=9) == stitch(B=0) == E["BADARG"]
    assert stitch(n_preds=2 ** 24) == stitch(h=2 ** 16, w=2 ** 16) == E["TOOLARGE"]
    assert stitch(preds=p + 2) == stitch(tiles=p + 2) == stitch(out=p + 2) == stitch(wts=p + 4) == E["ALIGN"]
    # two things wrong at once: null pointers and bad scalars, then the shape (bad, then too large), then the workspace's
    # size, then every alignment
    huge = dict(B=2 ** 20, n=chunk << 12)
    assert combine(x=None, **huge) == combine(clamp=1, lo=1.0, hi=-1.0, **huge) == combine(T=0, **huge) == E["BADARG"]
    assert combine(x=p + 2, **huge) == E["TOOLARGE"] and combine(x=p + 2, T=0) == E["BADARG"]
    assert p_sample(param=3, **huge) == p_sample(ra=None, **huge) == p_sample(T=0, **huge) == E["BADARG"]
    assert p_sample(x=p + 1, **huge) == E["TOOLARGE"] and p_sample(t=p + 4, n=0) == E["BADARG"]
    assert sums(kind=2, **huge) == sums(ws=None, **huge) == E["BADARG"]
    assert sums(nbytes=0, **huge) == sums(pred=p + 2, **huge) == E["TOOLARGE"]
    assert sums(nbytes=15, pred=p + 2) == sums(nbytes=15, ws=p + 4) == E["WORKSPACE"] and sums(nbytes=0, B=0) == E["BADARG"]
    assert finish(lsw=nan, **huge) == finish(S=None, **huge) == finish(nbytes=0, T=0) == E["BADARG"]
    assert finish(nbytes=0, **huge) == finish(B=2 ** 31, n=1, nbytes=0) == finish(B=2 ** 31, n=1, ws=p + 4) == E["TOOLARGE"]
    assert finish(nbytes=8, ws=p + 4) == finish(nbytes=8, lv=p + 2) == E["WORKSPACE"]
    assert grad(kind=2, **huge) == grad(gx0=p, t=None, **huge) == grad(pred=p + 2, n=0) == E["BADARG"]
    assert grad(pred=p + 2, **huge) == grad(coef=p + 4, **huge) == E["TOOLARGE"]
    assert gather(src=None, h=2 ** 16, w=2 ** 16) == gather(ntiles=0, h=2 ** 16, w=2 ** 16) == gather(src=p + 2, ts=9) == E["BADARG"]
    assert gather(src=p + 2, h=2 ** 16, w=2 ** 16) == E["TOOLARGE"]
    assert stitch(bstep=2, n_preds=2 ** 24) == stitch(n_preds=0, h=2 ** 16, w=2 ** 16) == stitch(out=p + 2, B=0) == E["BADARG"]
    assert stitch(preds=p + 2, n_preds=2 ** 24) == stitch(wts=p + 4, h=2 ** 16, w=2 ** 16) == E["TOOLARGE"]
    assert np.array_equal(buf, before)


def test_python_refusals():
    from ssl_amd import diffusion
    x = torch.zeros(2, 4, 8, 8)
    with pytest.raises(ValueError):
        diffusion.canvas_gather(x, [(0, 1)], 8)               # leaves the canvas
    with pytest.raises(ValueError):
        diffusion.canvas_gather(x, [], 8)
    with pytest.raises(ValueError):
        diffusion.canvas_gather(torch.zeros(0, 4, 8, 8), [(0, 0)], 8)
    with pytest.raises(ValueError):
        diffusion.canvas_stitch(torch.zeros(3, 4, 8, 8), [(0, 0)], (2, 4, 8, 8))
    with pytest.raises(TypeError):
        diffusion.canvas_stitch(torch.zeros(2, 4, 8, 8), [(0, 0)], (2, 4, 8, 8), torch.ones(8, 8))
    with pytest.raises(ValueError):
        diffusion.canvas_stitch(torch.zeros(2, 4, 8, 8), [(0, 0)], (2, 4, 8, 8), per_sample=False)
    s = diffusion.Schedule(**C.SCHEDULES["linear_v"])
    with pytest.raises(ValueError):
        s.q_sample(torch.zeros(2, 3), torch.tensor([0, 1]), torch.zeros(2, 4))
    with pytest.raises(RuntimeError):
        diffusion._rows(torch.zeros(2, 0))                                   # an empty tensor: SSG_E_BADARG
    with pytest.raises(RuntimeError):
        diffusion.loss_sums(torch.zeros(2, 3), torch.zeros(2, 3))          # no CPU path for the kernels' own probe
