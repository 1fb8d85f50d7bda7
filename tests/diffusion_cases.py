"""The shapes and seeded contents that the diffusion tests, the fixture maker and tools/diffusion_time.py share
(ssl_amd/diffusion.py, ssl_amd/csrc/ssg_diffusion.hip).  torch on the CPU and numpy only; nothing of ssl_amd."""
import numpy as np
import torch

# ---- schedules: name -> the arguments of register_schedule, the parameterization, v_posterior ----
SCHEDULES = {
    # the configuration of the fork's training and test files (v2-finetune_text_T_512.yaml, test.py:273)
    "linear_eps": dict(beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.0120,
                       parameterization="eps", v_posterior=0.),
    "linear_v": dict(beta_schedule="linear", timesteps=40, linear_start=1e-4, linear_end=2e-2, parameterization="v",
                     v_posterior=0.),
    "cosine_x0": dict(beta_schedule="cosine", timesteps=50, cosine_s=8e-3, parameterization="x0", v_posterior=0.),
    "sqrt_linear_eps": dict(beta_schedule="sqrt_linear", timesteps=30, linear_start=1e-4, linear_end=2e-2,
                            parameterization="eps", v_posterior=0.25),
    "sqrt_eps": dict(beta_schedule="sqrt", timesteps=30, linear_start=1e-4, linear_end=2e-2, parameterization="eps",
                     v_posterior=0.),
}
BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
           "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
           "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
           "lvlb_weights")
RESPACED = (200, 1000)            # of "linear_eps"
P2 = dict(p2_gamma=0.5, p2_k=1.0)


# ---- the per-sample kernels: B, n (CH = ssg_diff_chunk()), every tensor offset by 0 .. 3 floats ----
BATCHES = (1, 3, 5)


def sample_counts(chunk):
    return (1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 7)


def second_trip_count(chunk, grid_cap):
    """n of ONE sample with 2 grid_cap + 1 chunks, the last of 5 elements: every workgroup makes a second trip, the
    first a third, and a tail of one head / tail walk remains."""
    return 2 * grid_cap * chunk + 5


def timesteps(B, T, seed=0):
    """(B,) int64 with 0, T - 1 and a repeat wherever B allows."""
    g = torch.Generator().manual_seed(500 + seed)
    t = torch.randint(0, T, (B,), generator=g)
    t[0] = 0
    if B > 1:
        t[-1] = T - 1
    if B > 3:
        t[2] = t[1]
    return t


SPECIALS = (0.0, -0.0, 1e-40, -1e-40, float("inf"), float("-inf"), float("nan"), 1.0, -1.0, 3.0e38)


def offset_tensor(values, offset):
    """`values` (B, n) as a contiguous (B, 1, 1, n) view that starts `offset` floats into its storage."""
    flat = torch.empty(values.numel() + 3, dtype=values.dtype)
    view = flat[offset:offset + values.numel()].view(values.shape[0], 1, 1, -1)
    view.copy_(values.view(values.shape[0], 1, 1, -1))
    return view


def sample_inputs(B, n, seed, specials=True, count=3):
    """`count` fp32 (B, n) tensors of N(0, 1); with specials, +-0, subnormals, +-inf, a NaN and large values strewn over the
    first tensors' leading elements of sample 0 (where n allows)."""
    g = torch.Generator().manual_seed(900 + seed)
    out = [torch.randn(B, n, generator=g) for _ in range(count)]
    if specials:
        for j, v in enumerate(SPECIALS):
            if j < n:
                out[j % count][0, j] = v
    return out


def logvar_table(T, seed=0):
    g = torch.Generator().manual_seed(700 + seed)
    return (0.5 * torch.randn(T, generator=g)).to(torch.float32)


# ---- the canvas: (tile, overlap, h, w) ----
CANVAS = (
    (8, 4, 8, 8),        # one tile
    (8, 4, 8, 21),       # one snapped axis
    (8, 4, 21, 8),
    (8, 4, 19, 21),      # both snapped
    (8, 0, 16, 24),      # no overlap
    (8, 7, 12, 12),      # every stride 1: the heavy overlap
    (64, 32, 96, 160),   # the script's own geometry
)
CANVAS_HEAVY = (8, 7, 12, 12)
CANVAS_C = 4
CANVAS_BATCHES = (1, 2)
CANVAS_FIXTURE_B = {(64, 32, 96, 160): (1,)}     # the fixture holds the large case at B = 1 only (size)


def canvas_name(case, B):
    return "canvas_%d_%d_%d_%d_b%d" % (*case, B)


def canvas_inputs(case, B, seed=0):
    """(x, struct_cond) fp32 (B, C, h, w), seeded."""
    _, _, h, w = case
    g = torch.Generator().manual_seed(1300 + seed + 7 * B + h * 131 + w)
    return torch.randn(B, CANVAS_C, h, w, generator=g), torch.randn(B, CANVAS_C, h, w, generator=g)


def stand_in_network(x, cond):
    """The fixed elementwise function that stands where the U-Net is, evaluated ON THE CPU whatever the device (the
    network is not under test, and the CPU's bits are the fixture's)."""
    y = x.detach().cpu() * 0.75 - cond.detach().cpu() * 0.25
    return y.to(x.device)


# ---- ImageSpliterTh: (h, w, patch, stride, sf) ----
SPLITTER = (
    (20, 17, 8, 6, 1),
    (20, 17, 8, 6, 2),
    (8, 5, 8, 6, 1),      # a side <= the patch
    (7, 19, 8, 6, 2),
)


def splitter_name(case):
    return "split_%d_%d_%d_%d_%d" % case


def splitter_input(case, seed=0):
    h, w = case[:2]
    g = torch.Generator().manual_seed(1700 + seed + h * 37 + w)
    return torch.randn(2, 3, h, w, generator=g)


def splitter_patch_result(pch, sf, k):
    """What stands where the VQGAN is: the patch enlarged by sf (nearest) and scaled by a factor that depends on the
    patch's number, so that the order of the accumulation shows."""
    y = pch.detach().cpu().repeat_interleave(sf, dim=2).repeat_interleave(sf, dim=3) * (1.0 + 0.125 * (k % 5))
    return y.to(pch.device)
