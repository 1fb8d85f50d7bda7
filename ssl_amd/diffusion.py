"""What surrounds the Diffusion fork's U-Net, outside the network, on the kernels of ssl_amd/csrc/ssg_diffusion.hip
(include/ssg_hip.h section (W)).

    Schedule                 DDPM.register_schedule's buffers (Diffusion-Based-SR/ldm/models/diffusion/ddpm.py:234-289) with
                             make_beta_schedule, and respaced(): space_timesteps + the re-registration of test.py:277-292
    Schedule.q_sample, get_v, predict_start_from_noise, predict_start_from_z_and_v, q_posterior
                             the reference's methods, names and argument order; one launch each
    Schedule.p_sample        everything of p_sample behind the network call, one launch
    p_losses_criterion       ddpmssl.py:365-436 between the network's output and the decoder: loss_simple, the P2 weight,
                             logvar, the VLB term, the four logged scalars and x0 = predict_start_from_noise, forward in
                             three launches (sums, finish, x0), backward in one
    canvas_tiles, gaussian_weights, canvas_gather, canvas_stitch, p_sample_canvas_step
                             p_mean_variance_canvas / p_sample_canvas (ddpm.py:2538-2733): all tiles in one launch, the
                             weighted stitch in one launch
    ImageSpliterTh           scripts/util_image.py:686-769; gather() is the same stitch with unit weights

The native domain ("Which calls take the kernels"): fp32 contiguous GPU tensors on one device, no input that
requires a gradient (the criterion excepted: it is the differentiable piece),
`ssl_amd.losses.set_native_criteria(True)`.  Anything else -- CPU tensors, fp64, half, bf16, an input in a graph -- takes
the reference's torch lines and gives their bits.

`t` is an int64 tensor on the tensors' device and is never read on the host: the coefficients are gathered by the kernels.
The contract for its values is 0 <= t < T; a GPU sample whose t is outside gets NaN results (nothing is read outside a
table), a host `t` is checked and refused.  The reference's `self.logvar[t.cpu()].to(self.device)` is a host
synchronisation every training step; here logvar lives on the device and is gathered there.
"""
import numpy as np
import torch

from . import _gpu, _lib

__all__ = ["Schedule", "make_beta_schedule", "space_timesteps", "p_losses_criterion", "canvas_tiles", "gaussian_weights",
           "canvas_gather", "canvas_stitch", "p_sample_canvas_step", "ImageSpliterTh", "loss_sums"]

EPS, X0, V = (_lib.CONSTANTS["SSG_DIFF_" + k] for k in ("EPS", "X0", "V"))
_PARAM = {"eps": EPS, "x0": X0, "v": V}
_KIND = {"l1": _lib.CONSTANTS["SSG_PIX_L1"], "l2": _lib.CONSTANTS["SSG_PIX_MSE"]}
_BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
            "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
            "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
            "lvlb_weights")


# ---------------------------------------------------------------------------------------------------- schedule ---
def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """The betas of a named schedule as an fp64 numpy array (ldm/modules/diffusionmodules/util.py); torch's fp64 linspace
    and cosine on the CPU, as there, so that the bits are the reference's."""
    f64 = torch.float64
    if schedule == "linear":
        betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=f64) ** 2
    elif schedule == "cosine":
        steps = torch.arange(n_timestep + 1, dtype=f64) / n_timestep + cosine_s
        alphas = torch.cos(steps / (1 + cosine_s) * np.pi / 2).pow(2)
        alphas = alphas / alphas[0]
        betas = (1 - alphas[1:] / alphas[:-1]).clamp(min=0, max=0.999)
    elif schedule == "sqrt_linear":
        betas = torch.linspace(linear_start, linear_end, n_timestep, dtype=f64)
    elif schedule == "sqrt":
        betas = torch.linspace(linear_start, linear_end, n_timestep, dtype=f64) ** 0.5
    else:
        raise ValueError(f"schedule '{schedule}' unknown.")
    return betas.numpy()


def space_timesteps(num_timesteps, section_counts):
    """The set of steps of the original process that a respaced one keeps (ldm/models/respace.py): per section of equal
    size, `count` steps at a fractional stride, each rounded; "ddimN" is the integer stride that gives N steps."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            want = int(section_counts[4:])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    base, extra = divmod(num_timesteps, len(section_counts))
    start, steps = 0, []
    for i, count in enumerate(section_counts):
        size = base + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        at = 0.0
        for _ in range(count):
            steps.append(start + round(at))
            at += stride
        start += size
    return set(steps)


class Schedule:
    """The buffers of DDPM.register_schedule as fp32 tensors under the reference's names, on `device`.

    The arithmetic is numpy's, in the dtype of the betas (fp64 from make_beta_schedule; fp32 where `given_betas` is, as
    after a respacing), and every table is cast to float32 once.  `lvlb_weights` is formed from the float32 buffers in
    torch, as the reference forms it, for 'eps' / 'x0' / 'v', with lvlb_weights[0] = lvlb_weights[1].  Beside them:
        sigma   (0.5 * posterior_log_variance_clipped).exp(), taken with torch ON `device`: p_sample's exp is then the
                reference's own on that device
        p2      1 / (p2_k + snr) ** p2_gamma with snr = 1 / (1 - alphas_cumprod) - 1 (fp32, on `device`), or None
    """

    def __init__(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4, linear_end=2e-2,
                 cosine_s=8e-3, parameterization="eps", v_posterior=0., p2_gamma=None, p2_k=None, device=None):
        if parameterization not in _PARAM:
            raise NotImplementedError("mu not supported")
        if given_betas is None:
            betas = make_beta_schedule(beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end,
                                       cosine_s=cosine_s)
        else:
            betas = np.asarray(given_betas)
        alphas = 1. - betas
        ac = np.cumprod(alphas, axis=0)
        ac_prev = np.append(1., ac[:-1])
        self.num_timesteps = int(betas.shape[0])
        self.parameterization, self.v_posterior = parameterization, v_posterior
        self.p2_gamma, self.p2_k = p2_gamma, p2_k
        self.linear_start, self.linear_end = linear_start, linear_end
        f32 = lambda a: torch.tensor(a, dtype=torch.float32)
        tab = dict(betas=f32(betas), alphas_cumprod=f32(ac), alphas_cumprod_prev=f32(ac_prev),
                   sqrt_alphas_cumprod=f32(np.sqrt(ac)), sqrt_one_minus_alphas_cumprod=f32(np.sqrt(1. - ac)),
                   log_one_minus_alphas_cumprod=f32(np.log(1. - ac)), sqrt_recip_alphas_cumprod=f32(np.sqrt(1. / ac)),
                   sqrt_recipm1_alphas_cumprod=f32(np.sqrt(1. / ac - 1)))
        variance = (1 - v_posterior) * betas * (1. - ac_prev) / (1. - ac) + v_posterior * betas
        tab.update(posterior_variance=f32(variance),
                   posterior_log_variance_clipped=f32(np.log(np.maximum(variance, 1e-20))),
                   posterior_mean_coef1=f32(betas * np.sqrt(ac_prev) / (1. - ac)),
                   posterior_mean_coef2=f32((1. - ac_prev) * np.sqrt(alphas) / (1. - ac)))
        if parameterization == "x0":
            a32 = torch.Tensor(ac)
            lvlb = 0.5 * a32.sqrt() / (2. * 1 - a32)
        else:
            lvlb = tab["betas"] ** 2 / (2 * tab["posterior_variance"] * f32(alphas) * (1 - tab["alphas_cumprod"]))
            if parameterization == "v":
                lvlb = torch.ones_like(lvlb)
        if self.num_timesteps > 1:
            lvlb[0] = lvlb[1]
        tab["lvlb_weights"] = lvlb
        self._place(tab, torch.device("cpu") if device is None else torch.device(device))

    def _place(self, tab, device):
        self.device = device
        for name in _BUFFERS:
            setattr(self, name, tab[name].to(device).contiguous())
        self.sigma = (0.5 * self.posterior_log_variance_clipped).exp()
        self.p2 = None
        if self.p2_gamma is not None:
            assert self.p2_k is not None
            snr = 1.0 / (1 - self.alphas_cumprod) - 1
            self.p2 = 1 / (self.p2_k + snr) ** self.p2_gamma
        self._recon = {EPS: (self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod), X0: (None, None),
                       V: (self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)}[_PARAM[self.parameterization]]

    def to(self, device):
        """The same tables on another device (sigma and p2 are taken again there)."""
        other = object.__new__(Schedule)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k not in _BUFFERS})
        other._place({name: getattr(self, name) for name in _BUFFERS}, torch.device(device))
        return other

    def respaced(self, ddpm_steps):
        """test.py:277-292: keep space_timesteps(T, [ddpm_steps]), form the new betas 1 - a_i / a_last from the FLOAT32
        alphas_cumprod (the reference divides 0-dim float32 tensors) and register them again.  The kept steps, sorted,
        are `ori_timesteps` of the result."""
        keep = sorted(space_timesteps(self.num_timesteps, [ddpm_steps]))
        a = self.alphas_cumprod.cpu()[keep]
        last = torch.cat([torch.ones(1), a[:-1]])
        betas = (1 - a / last).numpy()
        out = Schedule(given_betas=betas, parameterization=self.parameterization, v_posterior=self.v_posterior,
                       p2_gamma=self.p2_gamma, p2_k=self.p2_k, device=self.device)
        out.ori_timesteps = keep
        return out

    # ---- the reference's methods ----
    def q_sample(self, x_start, t, noise=None):
        noise = torch.randn_like(x_start) if noise is None else noise
        return _combine(self.sqrt_alphas_cumprod, x_start, self.sqrt_one_minus_alphas_cumprod, noise, t, False)

    def get_v(self, x, noise, t):
        return _combine(self.sqrt_alphas_cumprod, noise, self.sqrt_one_minus_alphas_cumprod, x, t, True)

    def predict_start_from_noise(self, x_t, t, noise):
        return _combine(self.sqrt_recip_alphas_cumprod, x_t, self.sqrt_recipm1_alphas_cumprod, noise, t, True)

    def predict_start_from_z_and_v(self, x, v, t):
        return _combine(self.sqrt_alphas_cumprod, x, self.sqrt_one_minus_alphas_cumprod, v, t, True)

    def q_posterior(self, x_start, x_t, t):
        mean = _combine(self.posterior_mean_coef1, x_start, self.posterior_mean_coef2, x_t, t, False)
        return (mean, extract_into_tensor(self.posterior_variance, t, x_t.shape),
                extract_into_tensor(self.posterior_log_variance_clipped, t, x_t.shape))

    def p_sample(self, x, model_out, t, noise, clip_denoised=False, return_x0=False):
        """p_sample behind the network call: x_recon by parameterization, the optional clamp_(-1, 1), q_posterior's mean
        and mean + (t != 0) * sigma[t] * noise.  `noise` is the caller's (noise_like(...) * temperature, after its
        dropout).  Returns x_{t-1}, or (x_{t-1}, x_recon) with return_x0.  (For 'x0' with the clamp the reference's lines clamp
        `model_out` itself, in place; the kernel leaves its inputs alone.)"""
        _check_t(t, self.num_timesteps, x.shape[0])
        _table_on(self.sigma, x)
        B, n = _rows(x, model_out, noise)
        if not _native((x, model_out, noise), t):
            return _p_sample_torch(self, x, model_out, t, noise, clip_denoised, return_x0)
        x, model_out, noise, t = x.contiguous(), model_out.contiguous(), noise.contiguous(), t.contiguous()
        out = torch.empty_like(x)
        x0 = torch.empty_like(x) if return_x0 else None
        ra, rb = self._recon
        _gpu.launch(x.device, _lib.lib().ssg_diff_p_sample, x.data_ptr(), model_out.data_ptr(), noise.data_ptr(),
                    t.data_ptr(), _gpu.ptr(ra), _gpu.ptr(rb), self.posterior_mean_coef1.data_ptr(),
                    self.posterior_mean_coef2.data_ptr(), self.sigma.data_ptr(), self.num_timesteps, B, n,
                    _PARAM[self.parameterization], int(bool(clip_denoised)), out.data_ptr(), _gpu.ptr(x0))
        return (out, x0) if return_x0 else out


def extract_into_tensor(a, t, x_shape):
    """a[t] shaped (B, 1, ..., 1) for a tensor of x_shape (ldm/modules/diffusionmodules/util.py)."""
    return a.gather(-1, t).reshape(t.shape[0], *((1,) * (len(x_shape) - 1)))


def _native(tensors, t=None, no_grad=None):
    """Whether the kernels take the call: the package's rule (_gpu.native: the switch, fp32 tensors on one GPU), `t`, where
    the call has one, an int64 tensor on that GPU, and nothing in an autograd graph -- none of `no_grad` (None: of the
    tensors) requires grad while grad is enabled."""
    if not _gpu.native(*tensors) or (t is not None and (t.device != tensors[0].device or t.dtype != torch.int64)):
        return False
    return not (torch.is_grad_enabled() and any(x.requires_grad for x in (tensors if no_grad is None else no_grad)))


def _rows(*tensors):
    """(B, n) of tensors of one shape with a batch dimension; refuses empty ones and a mismatch."""
    shape = tensors[0].shape
    if len(shape) < 1 or any(x.shape != shape for x in tensors):
        raise ValueError(f"ssl_amd.diffusion: tensors of one shape with a batch dimension expected, got "
                         f"{[tuple(x.shape) for x in tensors]}")
    if tensors[0].numel() == 0:
        _lib.check(_lib.CONSTANTS["SSG_E_BADARG"])
    return shape[0], tensors[0].numel() // shape[0]


def _check_t(t, T, B):
    """t is (B,) int64; its values are checked where that costs no synchronisation: on a host tensor."""
    if t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"ssl_amd.diffusion: t must be an int64 tensor of shape ({B},), got {t.dtype} {tuple(t.shape)}")
    if not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) >= T):
        raise IndexError(f"ssl_amd.diffusion: t outside [0, {T})")


def _table_on(table, x):
    if table.device != x.device:
        raise RuntimeError(f"ssl_amd.diffusion: the schedule is on {table.device}, the tensors on {x.device}; "
                           "use Schedule.to(device)")
    return table


def _combine(A, x, Bt, y, t, subtract, clamp=None):
    """fl(fl(A[t] x) +- fl(Bt[t] y)), optionally clamped: one launch, or the reference's line."""
    _check_t(t, A.shape[0], x.shape[0])
    _table_on(A, x)
    B, n = _rows(x, y)
    if not _native((x, y), t):
        a, b = extract_into_tensor(A, t, x.shape) * x, extract_into_tensor(Bt, t, x.shape) * y
        out = a - b if subtract else a + b
        return out if clamp is None else out.clamp_(*clamp)
    x, y, t = x.contiguous(), y.contiguous(), t.contiguous()
    out = torch.empty_like(x)
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    _gpu.launch(x.device, _lib.lib().ssg_diff_combine, x.data_ptr(), y.data_ptr(), t.data_ptr(), A.data_ptr(),
                Bt.data_ptr(), A.shape[0], B, n, int(subtract), int(clamp is not None), lo, hi, out.data_ptr())
    return out


def _p_sample_torch(s, x, model_out, t, noise, clip_denoised, return_x0):
    """The reference's lines (p_mean_variance + p_sample) on any device and dtype."""
    if s.parameterization == "eps":
        x_recon = s.predict_start_from_noise(x, t=t, noise=model_out)
    elif s.parameterization == "x0":
        x_recon = model_out
    else:
        x_recon = s.predict_start_from_z_and_v(x, model_out, t)
    if clip_denoised:
        x_recon.clamp_(-1., 1.)
    mean, _, log_variance = s.q_posterior(x_start=x_recon, x_t=x, t=t)
    nonzero_mask = (1 - (t == 0).float()).reshape(x.shape[0], *((1,) * (len(x.shape) - 1)))
    out = mean + nonzero_mask * (0.5 * log_variance).exp() * noise
    return (out, x_recon) if return_x0 else out


# --------------------------------------------------------------------------------------------------- criterion ---
def _workspace(B, n, dev):
    nbytes = _lib.lib().ssg_diff_workspace_bytes(B, n)
    if nbytes == 0:
        _lib.check(_lib.CONSTANTS["SSG_E_TOOLARGE"])
    return _gpu.workspace(nbytes, dev)


def loss_sums(pred, target, loss_type="l2"):
    """S_b = sum_i l(target - pred) per sample as fp64 (B,), on the kernels: ssg_diff_loss_sums and the fold of
    ssg_diff_loss_finish (with neutral tables).  For tests and tools; p_losses_criterion is the API."""
    _gpu.need_gpu(pred, target)
    pred, target = pred.contiguous(), target.contiguous()
    B, n = _rows(pred, target)
    dev = pred.device
    with _gpu.on(dev):
        ws, nbytes = _workspace(B, n, dev)
        t = torch.zeros(B, dtype=torch.int64, device=dev)
        zero = torch.zeros(1, device=dev)
        out = torch.empty(2 * B + 4, dtype=torch.float64, device=dev)
        L = _lib.lib()
        _gpu.launch(dev, L.ssg_diff_loss_sums, pred.data_ptr(), target.data_ptr(), B, n, _KIND[loss_type], ws.data_ptr(),
                    nbytes)
        _gpu.launch(dev, L.ssg_diff_loss_finish, ws.data_ptr(), nbytes, t.data_ptr(), None, zero.data_ptr(),
                    zero.data_ptr(), 1, B, n, 1.0, 0.0, out.data_ptr(), out[B:].data_ptr(), out[B + 4:].data_ptr(), None)
    return out[:B]


class _Criterion(torch.autograd.Function):
    """(loss, x0, scalars) of (model_output, logvar); the rest are constants of the call."""

    @staticmethod
    def forward(ctx, model_output, logvar, target, x_noisy, t, schedule, kind, lsw, elbo, learn):
        dev = model_output.device
        pred, target, x_noisy, t = model_output.contiguous(), target.contiguous(), x_noisy.contiguous(), t.contiguous()
        ctx.set_materialize_grads(False)      # a gradient that does not arrive is None, not a tensor of zeros
        B, n = _rows(pred, target, x_noisy)
        T = schedule.num_timesteps
        L = _lib.lib()
        with _gpu.on(dev):
            ws, nbytes = _workspace(B, n, dev)
            # one allocation: S (B), the four scalars, coef (B), dlogvar (T)
            out = torch.empty(2 * B + 4 + T, dtype=torch.float64, device=dev)
            S, scalars, coef, dlv = out[:B], out[B:B + 4], out[B + 4:2 * B + 4], out[2 * B + 4:]
            lv = logvar.detach().contiguous()
            _gpu.launch(dev, L.ssg_diff_loss_sums, pred.data_ptr(), target.data_ptr(), B, n, kind, ws.data_ptr(), nbytes)
            _gpu.launch(dev, L.ssg_diff_loss_finish, ws.data_ptr(), nbytes, t.data_ptr(), _gpu.ptr(schedule.p2),
                        lv.data_ptr(), schedule.lvlb_weights.data_ptr(), T, B, n, lsw, elbo, S.data_ptr(),
                        scalars.data_ptr(), coef.data_ptr(), dlv.data_ptr() if learn else None)
            x0 = torch.empty_like(pred)
            _gpu.launch(dev, L.ssg_diff_combine, x_noisy.data_ptr(), pred.data_ptr(), t.data_ptr(),
                        schedule.sqrt_recip_alphas_cumprod.data_ptr(), schedule.sqrt_recipm1_alphas_cumprod.data_ptr(),
                        T, B, n, 1, 0, 0.0, 0.0, x0.data_ptr())
        ctx.save_for_backward(pred, target, t, coef, dlv)
        ctx.schedule, ctx.kind, ctx.learn, ctx.rows = schedule, kind, learn, (B, n)
        logged = scalars.to(torch.float32)
        ctx.mark_non_differentiable(logged)
        return logged[3].clone(), x0, logged

    @staticmethod
    def backward(ctx, g_loss, g_x0, _):
        pred, target, t, coef, dlv = ctx.saved_tensors
        dev, (B, n), s = pred.device, ctx.rows, ctx.schedule
        grad_pred = grad_logvar = None
        if g_loss is None and g_x0 is None:
            return (None,) * 10
        with _gpu.on(dev):
            g = torch.zeros(1, device=dev) if g_loss is None else g_loss.to(torch.float32).reshape(1)
            if ctx.needs_input_grad[0]:
                gx0 = None if g_x0 is None else g_x0.to(torch.float32).contiguous()
                grad_pred = torch.empty_like(pred)
                _gpu.launch(dev, _lib.lib().ssg_diff_loss_grad, pred.data_ptr(), target.data_ptr(), _gpu.ptr(gx0),
                            t.data_ptr(), s.sqrt_recipm1_alphas_cumprod.data_ptr(), s.num_timesteps, g.data_ptr(),
                            coef.data_ptr(), B, n, ctx.kind, grad_pred.data_ptr())
            if ctx.learn and ctx.needs_input_grad[1]:
                grad_logvar = (dlv * g.double()).to(torch.float32)
        return grad_pred, grad_logvar, None, None, None, None, None, None, None, None


def _criterion_torch(model_output, target, x_noisy, t, s, logvar, loss_type, lsw, elbo):
    """ddpmssl.py:391-417 (without the .cpu() round trip of t, which changes no value), the P2 line's broadcast included:
    with the weight on, `loss` is (B, 1, 1, B) and its mean weights every sample by the batch mean of the P2 weights."""
    diff = target - model_output
    per = (diff.abs() if loss_type == "l1" else diff * diff).mean([1, 2, 3]) if diff.dim() == 4 else \
        (diff.abs() if loss_type == "l1" else diff * diff).flatten(1).mean(1)
    loss_simple = per
    logged = [loss_simple.mean()]
    if s.p2 is not None:
        # the reference's line as it stands: a (B, 1, 1, 1) weight times the (B,) loss_simple is (B, 1, 1, B)
        loss_simple = extract_into_tensor(s.p2, t, target.shape) * loss_simple
    logvar_t = logvar[t]
    loss = loss_simple / torch.exp(logvar_t) + logvar_t
    logged.append(loss.mean())
    loss = lsw * loss.mean()
    loss_vlb = (s.lvlb_weights[t] * per).mean()
    logged.append(loss_vlb)
    loss = loss + elbo * loss_vlb
    logged.append(loss)
    x0 = (extract_into_tensor(s.sqrt_recip_alphas_cumprod, t, x_noisy.shape) * x_noisy -
          extract_into_tensor(s.sqrt_recipm1_alphas_cumprod, t, x_noisy.shape) * model_output)
    return loss, x0, logged


def p_losses_criterion(model_output, target, x_noisy, t, schedule, logvar, loss_type="l2", l_simple_weight=1.,
                       original_elbo_weight=0., learn_logvar=None, prefix="train"):
    """(loss, x0, loss_dict) of ddpmssl.py's p_losses between the network and the decoder.

    loss = l_simple_weight mean_b(wbar m_b / exp(logvar[t_b]) + logvar[t_b]) + original_elbo_weight mean_b(lvlb[t_b] m_b),
    m_b = mean_i l(target - model_output), wbar the BATCH MEAN of the P2 weights p2[t_b] of `schedule` (1 without) -- the
    reference multiplies its (B,) loss_simple by a (B, 1, 1, 1) weight and takes the mean of the (B, 1, 1, B) result
    (ddpmssl.py:397-401), which is this, not a per-sample weight; kept as the reference has it; x0 =
    predict_start_from_noise(x_noisy, t, model_output), differentiable: the pixel L1 and the SSG loss of the decoded x0
    send their gradient back through it, and the one backward launch adds both paths.  loss_dict holds the reference's
    four entries `{prefix}/loss_simple` (before the P2 weight), `/loss_gamma` and `logvar` (learnt logvar only),
    `/loss_vlb` (the unweighted per-sample mean) and `/loss`, detached.  `logvar` is (T,) fp32 on the device, an
    nn.Parameter where it is learnt (learn_logvar defaults to logvar.requires_grad)."""
    if loss_type not in _KIND:
        raise NotImplementedError(f"unknown loss type '{loss_type}'")
    learn = bool(logvar.requires_grad) if learn_logvar is None else bool(learn_logvar)
    _check_t(t, schedule.num_timesteps, model_output.shape[0])
    _table_on(schedule.lvlb_weights, model_output)
    if model_output.dim() < 2:
        raise ValueError("ssl_amd.diffusion: the criterion takes tensors of (B, ...) with at least two dimensions")
    if logvar.shape != (schedule.num_timesteps,):
        raise ValueError(f"ssl_amd.diffusion: logvar must have shape ({schedule.num_timesteps},), got {tuple(logvar.shape)}")
    # (the differentiable piece: model_output and logvar may require grad, target and x_noisy may not)
    if _native((model_output, target, x_noisy, logvar), t, no_grad=(target, x_noisy)):
        loss, x0, logged = _Criterion.apply(model_output, logvar, target, x_noisy, t, schedule, _KIND[loss_type],
                                            float(l_simple_weight), float(original_elbo_weight), learn)
    else:
        loss, x0, logged = _criterion_torch(model_output, target, x_noisy, t, schedule, logvar, loss_type,
                                            l_simple_weight, original_elbo_weight)
        logged = [v.detach() for v in logged]
    loss_dict = {f"{prefix}/loss_simple": logged[0]}
    if learn:
        loss_dict[f"{prefix}/loss_gamma"] = logged[1]
        loss_dict["logvar"] = logvar.data.mean()
    loss_dict[f"{prefix}/loss_vlb"] = logged[2]
    loss_dict[f"{prefix}/loss"] = logged[3]
    return loss, x0, loss_dict


# ------------------------------------------------------------------------------------------------------ canvas ---
def canvas_tiles(h, w, tile_size, tile_overlap):
    """[(ofs_y, ofs_x)] of p_mean_variance_canvas's tiles in its loop order (ddpm.py:2552-2583), and (grid_rows,
    grid_cols).  Its quirks are kept: `grid_rows` counts along the WIDTH and the x offset is keyed by `row`, `grid_cols`
    along the height with y keyed by `col`; the last row snaps to w - tile_size and the last column to h - tile_size, and
    the corner tile keeps both snaps.  h or w below tile_size is refused (the reference slices with a negative offset)."""
    if tile_size < 1 or not 0 <= tile_overlap < tile_size:
        raise ValueError(f"ssl_amd.diffusion: need tile_size >= 1 and 0 <= tile_overlap < tile_size, got {tile_size}, "
                         f"{tile_overlap}")
    if h < tile_size or w < tile_size:
        raise ValueError(f"ssl_amd.diffusion: a {h} x {w} canvas is smaller than the tile ({tile_size})")
    step = tile_size - tile_overlap

    def count(extent):
        k, end = 0, 0
        while end < extent:
            end = max(k * step, 0) + tile_size
            k += 1
        return k

    rows, cols = count(w), count(h)
    tiles = []
    for row in range(rows):
        for col in range(cols):
            ox = w - tile_size if row == rows - 1 else row * step
            oy = h - tile_size if col == cols - 1 else col * step
            tiles.append((oy, ox))
    return tiles, (rows, cols)


def gaussian_weights(tile_width, tile_height, nbatches=1, channels=4, device=None):
    """_gaussian_weights (ddpm.py:2890-2905) in fp64: exp(-(x - m)^2 / n^2 / (2 var)) / sqrt(2 pi var), var = 0.01, with the
    x midpoint (n - 1) / 2 and the y midpoint n / 2 (the reference's asymmetry), the outer product tiled to
    (nbatches, channels, tile_height, tile_width).  A float64 tensor, as numpy makes it there."""
    var = 0.01

    def probs(n, mid):
        return [np.exp(-(i - mid) * (i - mid) / (n * n) / (2 * var)) / np.sqrt(2 * np.pi * var) for i in range(n)]

    plane = np.outer(probs(tile_height, tile_height / 2), probs(tile_width, (tile_width - 1) / 2))
    return torch.tile(torch.tensor(plane, device=device), (nbatches, channels, 1, 1))


_TABLES = {}


def _tile_table(records, dev):
    """The device table of (oy, ox, src) records, cached per (records, device): a sampling loop uploads it once."""
    key = (tuple(records), str(dev))
    if key not in _TABLES:
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = torch.tensor(records, dtype=torch.int32).reshape(-1, 3).to(dev)
    return _TABLES[key]


def canvas_gather(x, tiles, tile_size):
    """Every tile of x (B, C, h, w) in one launch: (len(tiles) B, C, ts, ts), tile k's samples at [k B, (k + 1) B) -- the
    order in which the reference concatenates its `input_list`."""
    if x.dim() != 4 or x.numel() == 0 or not tiles:
        raise ValueError("ssl_amd.diffusion: canvas_gather takes a non-empty (B, C, h, w) tensor and at least one tile")
    B, C, h, w = x.shape
    ts = tile_size
    for oy, ox in tiles:
        if oy < 0 or ox < 0 or oy + ts > h or ox + ts > w:
            raise ValueError(f"ssl_amd.diffusion: tile at ({oy}, {ox}) of size {ts} leaves the {h} x {w} canvas")
    if not _native((x,)):
        return torch.cat([x[:, :, oy:oy + ts, ox:ox + ts] for oy, ox in tiles], dim=0)
    x = x.contiguous()
    with _gpu.on(x.device):
        table = _tile_table([(oy, ox, k * B) for k, (oy, ox) in enumerate(tiles)], x.device)
        out = torch.empty(len(tiles) * B, C, ts, ts, device=x.device)
        _gpu.launch(x.device, _lib.lib().ssg_diff_canvas_gather, x.data_ptr(), table.data_ptr(), len(tiles), B, C, h, w,
                    ts, out.data_ptr())
    return out


def _stitch_records(tiles, grid, B, per_sample):
    """(oy, ox, src) per tile and the batch step.  per_sample: tile k of sample b is preds[k B + b].  Otherwise the
    reference's own indexing for B > 1: it appends EVERY sample of a tile batch to the row's list and then reads entry
    `col` of it, so tile (row, col) takes entry row grid_cols B + col of the concatenated predictions, for all samples."""
    rows, cols = grid
    if per_sample or B == 1:
        return [(oy, ox, k * B) for k, (oy, ox) in enumerate(tiles)], 1
    return [(oy, ox, (k // cols) * cols * B + k % cols) for k, (oy, ox) in enumerate(tiles)], 0


def canvas_stitch(preds, tiles, shape, tile_weights=None, grid=None, per_sample=True):
    """The weighted average of overlapping tiles on a (B, C, h, w) canvas in one launch: per element, over the tiles in
    order, acc += pred * w and cnt += w as torch's in-place add of an fp64 product into an fp32 tensor rounds them
    ((float)((double)acc + (double)pred * w)), then acc / cnt.  preds is (len(tiles) B, C, ts, ts) in canvas_gather's
    order; tile_weights is fp64, (ts, ts) or broadcastable to (B, C, ts, ts); None is the unweighted average.
    per_sample=False with grid=(grid_rows, grid_cols) reproduces the reference's indexing of its prediction list for
    B > 1 (see _stitch_records); for B = 1 the two are the same."""
    B, C, h, w = shape
    ts = preds.shape[-1]
    if preds.dim() != 4 or preds.numel() == 0 or preds.shape[1:] != (C, ts, ts) or preds.shape[0] != len(tiles) * B:
        raise ValueError(f"ssl_amd.diffusion: predictions of shape ({len(tiles) * B}, {C}, ts, ts) expected, got "
                         f"{tuple(preds.shape)}")
    if not per_sample and grid is None:
        raise ValueError("ssl_amd.diffusion: per_sample=False needs the grid")
    records, bstep = _stitch_records(tiles, grid if grid is not None else (1, len(tiles)), B, per_sample)
    w4 = None
    if tile_weights is not None:
        if tile_weights.dtype != torch.float64:
            raise TypeError("ssl_amd.diffusion: tile_weights must be float64 (gaussian_weights), as the reference's are")
        w4 = tile_weights.expand(B, C, ts, ts)
    if not _native((preds,)) or (w4 is not None and w4.device != preds.device):
        out = torch.zeros(shape, device=preds.device, dtype=preds.dtype)
        cnt = torch.zeros(shape, device=preds.device, dtype=preds.dtype)
        for oy, ox, src in records:
            p = preds[src:src + B] if bstep else preds[src:src + 1]
            out[:, :, oy:oy + ts, ox:ox + ts] += p * w4 if w4 is not None else p
            cnt[:, :, oy:oy + ts, ox:ox + ts] += w4 if w4 is not None else 1
        return out.div_(cnt)
    preds = preds.contiguous()
    dev = preds.device
    wsb = wsc = 0
    if w4 is not None:
        if w4.stride(2) != ts or w4.stride(3) != 1:
            w4 = w4.contiguous()
        wsb, wsc = w4.stride(0), w4.stride(1)
    with _gpu.on(dev):
        table = _tile_table(records, dev)
        out = torch.empty(shape, device=dev)
        _gpu.launch(dev, _lib.lib().ssg_diff_canvas_stitch, preds.data_ptr(), preds.shape[0], bstep, table.data_ptr(),
                    len(tiles), _gpu.ptr(w4), wsb, wsc, B, C, h, w, ts, out.data_ptr())
    return out


def p_sample_canvas_step(schedule, network, x, struct_cond, t, noise, tile_size=64, tile_overlap=32, tile_weights=None,
                         clip_denoised=False, return_x0=False, per_sample=True):
    """One step of p_sample_canvas: gather the tiles of x and struct_cond (one launch each), `network(x_tiles,
    cond_tiles)` -> predictions of x_tiles' shape (the caller batches the network over the tiles however it likes),
    stitch (one launch), p_sample (one launch)."""
    assert tile_weights is not None
    B, _, h, w = x.shape
    tiles, grid = canvas_tiles(h, w, tile_size, tile_overlap)
    preds = network(canvas_gather(x, tiles, tile_size), canvas_gather(struct_cond, tiles, tile_size))
    model_out = canvas_stitch(preds, tiles, x.shape, tile_weights, grid, per_sample)
    return schedule.p_sample(x, model_out, t[:B], noise, clip_denoised=clip_denoised, return_x0=return_x0)


class ImageSpliterTh:
    """scripts/util_image.py's ImageSpliterTh: the same constructor, iteration order (the width index is the outer one),
    update and gather.  update keeps the patch; gather averages all of them in one launch, in the order of the update
    calls, with unit weights -- through fp64 that is the reference's fp32 `+=` bit for bit (a sum rounded to 53 bits
    and then to 24 is the sum rounded to 24: 53 >= 2 * 24 + 2).  The kernel takes square patches of one size that lie inside the image; an image
    with a side below the patch (whose windows the reference clips) takes the reference's lines."""

    def __init__(self, im, pch_size, stride, sf=1):
        assert stride <= pch_size
        self.stride, self.pch_size, self.sf = stride, pch_size, sf
        bs, chn, height, width = im.shape
        self.height_starts_list = self.extract_starts(height)
        self.width_starts_list = self.extract_starts(width)
        self.length = self.__len__()
        self.num_pchs = 0
        self.im_ori = im
        self._shape = (bs, chn, height * sf, width * sf)
        self._patches, self._at = [], []

    def extract_starts(self, length):
        if length <= self.pch_size:
            return [0]
        starts = [min(s, length - self.pch_size) for s in range(0, length, self.stride)]
        return sorted(set(starts), key=starts.index)

    def __len__(self):
        return len(self.height_starts_list) * len(self.width_starts_list)

    def __iter__(self):
        return self

    def __next__(self):
        if self.num_pchs >= self.length:
            raise StopIteration()
        nh = len(self.height_starts_list)
        w_start = self.width_starts_list[self.num_pchs // nh]
        h_start = self.height_starts_list[self.num_pchs % nh]
        pch = self.im_ori[:, :, h_start:h_start + self.pch_size, w_start:w_start + self.pch_size]
        self.h_start, self.h_end = h_start * self.sf, (h_start + self.pch_size) * self.sf
        self.w_start, self.w_end = w_start * self.sf, (w_start + self.pch_size) * self.sf
        self.num_pchs += 1
        return pch, (self.h_start, self.h_end, self.w_start, self.w_end)

    def update(self, pch_res, index_infos):
        h_start, h_end, w_start, w_end = (self.h_start, self.h_end, self.w_start, self.w_end) if index_infos is None \
            else index_infos
        self._patches.append(pch_res)
        self._at.append((h_start, w_start))

    def gather(self):
        bs, chn, H, W = self._shape
        if not self._patches:
            raise AssertionError("ssl_amd.diffusion: ImageSpliterTh.gather before any update")
        ph, pw = self._patches[0].shape[-2:]
        square = all(p.shape[-2:] == (ph, ph) for p in self._patches)
        first = self._patches[0]
        if not (square and _native(self._patches) and first.dtype == self.im_ori.dtype):
            res = torch.zeros(self._shape, dtype=self.im_ori.dtype, device=self.im_ori.device)
            cnt = torch.zeros(self._shape, dtype=self.im_ori.dtype, device=self.im_ori.device)
            for p, (y, x) in zip(self._patches, self._at):
                res[:, :, y:y + p.shape[-2], x:x + p.shape[-1]] += p
                cnt[:, :, y:y + p.shape[-2], x:x + p.shape[-1]] += 1
            assert torch.all(cnt != 0)
            return res.div(cnt)
        for y, x in self._at:
            if y < 0 or x < 0 or y + ph > H or x + ph > W:
                raise ValueError(f"ssl_amd.diffusion: the window at ({y}, {x}) leaves the {H} x {W} image")
        covered = np.zeros((H, W), dtype=bool)
        for y, x in self._at:
            covered[y:y + ph, x:x + ph] = True
        assert covered.all()
        return canvas_stitch(torch.cat(self._patches, dim=0), self._at, self._shape, None)
