#!/usr/bin/env python3
"""The Diffusion fork's pieces around its network timed on the MI355X: the native path (ssl_amd.diffusion on fp32 GPU
tensors -> ssg_diff_*) beside the reference's torch lines on the same GPU, on preallocated inputs.

    criterion     ddpmssl.py's p_losses between the network's output and the decoder, forward and backward, with a
                  gradient arriving through x0 (as the pixel L1 and the SSG loss send one): loss_simple, the P2 weight,
                  logvar (learnt), the VLB term, predict_start_from_noise.  The torch path keeps the reference's
                  `self.logvar[t.cpu()].to(device)`, a host synchronisation per call; the native path has none.
                  Shapes B x 4 x 64 x 64 (the config's latent), B = 4 and 16.
    canvas_step   one step of p_sample_canvas around the network at a 256 x 256 latent (2048^2 output), tile 64, overlap
                  32, B = 1: 49 tiles.  Natively gather (x and struct_cond), stitch, p_sample: four launches.  The torch
                  path is the reference's loops: per tile two slices, per batch of four tiles two concatenations, per tile
                  `noise_pred[...] += pred * tile_weights; contributors[...] += tile_weights`, the division,
                  predict_start_from_noise, clamp_, q_posterior and the noise line.  The network itself is left out of
                  both (the predictions are the gathered tiles of x): no U-Net can be run here without its weights, so
                  the share of a whole step is NOT measured; what is reported is the bare time and the device operations
                  that the network call is surrounded by.
A warm-up, then `--rounds` alternating windows of `--iters` calls each, device events around a window; the median window
and the min / max; the whole measurement `--runs` times (two runs are quoted).  `device_ops` is the number of device
activities (kernels, copies, memsets) torch's profiler records for one call after the warm-up (null if the profiler is not
available).  `differing_elements` compares the two paths' results element by element: for the canvas step it is the
check that torch ON THE GPU rounds its mixed-precision in-place add as the kernel does.

    python tools/diffusion_time.py [--iters N] [--rounds R] [--warmup W] [--runs K] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bbl_time import compare  # noqa: E402
from gan_time import device_ops  # noqa: E402


def differing(a, b):
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


def criterion_paths(B, dev, gen):
    from ssl_amd import diffusion
    s = diffusion.Schedule(linear_start=0.00085, linear_end=0.0120, p2_gamma=0.5, p2_k=1.0, device=dev)
    shape = (B, 4, 64, 64)
    out, target, x_noisy, gx0 = (torch.randn(shape, generator=gen).to(dev) for _ in range(4))
    gx0 *= 1e-3
    t = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    p = out.requires_grad_(True)
    logvar = torch.zeros(1000, device=dev).requires_grad_(True)
    ext = diffusion.extract_into_tensor
    keep = {}

    def clear():
        p.grad = logvar.grad = None

    def native():
        clear()
        loss, x0, _ = diffusion.p_losses_criterion(p, target, x_noisy, t, s, logvar, "l2", 1.0, 0.5)
        torch.autograd.backward([loss, x0], [None, gx0])
        keep["native"] = (loss.detach(), x0.detach())

    def reference():
        clear()
        loss_simple = torch.nn.functional.mse_loss(target, p, reduction="none").mean([1, 2, 3])
        logged = {"loss_simple": loss_simple.mean()}
        weight = ext(1 / (s.p2_k + (1.0 / (1 - s.alphas_cumprod) - 1)) ** s.p2_gamma, t, shape)
        loss_simple = weight * loss_simple
        logvar_t = logvar[t.cpu()].to(dev)
        loss = loss_simple / torch.exp(logvar_t) + logvar_t
        logged["loss_gamma"] = loss.mean()
        logged["logvar"] = logvar.data.mean()
        loss = 1.0 * loss.mean()
        loss_vlb = torch.nn.functional.mse_loss(target, p, reduction="none").mean(dim=(1, 2, 3))
        loss_vlb = (s.lvlb_weights[t] * loss_vlb).mean()
        loss = loss + 0.5 * loss_vlb
        x0 = ext(s.sqrt_recip_alphas_cumprod, t, shape) * x_noisy - ext(s.sqrt_recipm1_alphas_cumprod, t, shape) * p
        torch.autograd.backward([loss, x0], [None, gx0])
        keep["torch"] = (loss.detach(), x0.detach())

    def check():
        native()
        g_native = p.grad.clone()
        reference()
        (ln, xn), (lt, xt) = keep["native"], keep["torch"]
        return dict(loss_rel_diff=abs(float(ln) - float(lt)) / abs(float(lt)), x0_differing_elements=differing(xn, xt),
                    max_grad_diff_over_max_grad=float((g_native - p.grad).abs().max() / p.grad.abs().max()))

    return [("native", native), ("torch", reference)], check, dict(shape=list(shape))


def canvas_paths(dev, gen):
    from ssl_amd import diffusion
    s = diffusion.Schedule(linear_start=0.00085, linear_end=0.0120, device=dev)
    B, C, h, w, ts, overlap, batch = 1, 4, 256, 256, 64, 32, 4
    x, cond, noise = (torch.randn(B, C, h, w, generator=gen).to(dev) for _ in range(3))
    t = torch.full((B,), 417, dtype=torch.int64, device=dev)
    weights = diffusion.gaussian_weights(ts, ts, B, C, device=dev)
    tiles, grid = diffusion.canvas_tiles(h, w, ts, overlap)
    network = lambda xt, ct: xt
    ext = diffusion.extract_into_tensor
    keep = {}

    def native():
        keep["native"] = diffusion.p_sample_canvas_step(s, network, x, cond, t, noise, ts, overlap, weights,
                                                        clip_denoised=True)

    def reference():
        rows, cols = grid
        preds, xs, cs = [], [], []
        for k, (oy, ox) in enumerate(tiles):
            xs.append(x[:, :, oy:oy + ts, ox:ox + ts])
            cs.append(cond[:, :, oy:oy + ts, ox:ox + ts])
            if len(xs) == batch or k % cols == cols - 1:
                xin, cin = torch.cat(xs, dim=0), torch.cat(cs, dim=0)
                model_out = network(xin, cin)
                preds += [model_out[i].unsqueeze(0) for i in range(model_out.size(0))]
                xs, cs = [], []
        noise_pred = torch.zeros(x.shape, device=dev)
        contributors = torch.zeros(x.shape, device=dev)
        for k, (oy, ox) in enumerate(tiles):
            noise_pred[:, :, oy:oy + ts, ox:ox + ts] += preds[k] * weights
            contributors[:, :, oy:oy + ts, ox:ox + ts] += weights
        noise_pred /= contributors
        x_recon = (ext(s.sqrt_recip_alphas_cumprod, t, x.shape) * x -
                   ext(s.sqrt_recipm1_alphas_cumprod, t, x.shape) * noise_pred)
        x_recon.clamp_(-1., 1.)
        mean = ext(s.posterior_mean_coef1, t, x.shape) * x_recon + ext(s.posterior_mean_coef2, t, x.shape) * x
        log_variance = ext(s.posterior_log_variance_clipped, t, x.shape)
        nonzero_mask = (1 - (t == 0).float()).reshape(B, 1, 1, 1)
        keep["torch"] = mean + nonzero_mask * (0.5 * log_variance).exp() * noise

    def check():
        native()
        reference()
        return dict(differing_elements=differing(keep["native"], keep["torch"]), elements=keep["torch"].numel())

    return [("native", native), ("torch", reference)], check, dict(shape=[B, C, h, w], tile=ts, overlap=overlap,
                                                                  tiles=len(tiles))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffusion_time.py needs the MI355X")
    dev = torch.device("cuda:0")
    lines = []
    for run in range(1, args.runs + 1):
        gen = torch.Generator().manual_seed(36)
        cases = [("criterion", criterion_paths(4, dev, gen)), ("criterion", criterion_paths(16, dev, gen)),
                 ("canvas_step", canvas_paths(dev, gen))]
        for name, (paths, check, info) in cases:
            parity = check()
            res = compare(paths, args.iters, args.rounds, args.warmup)
            ops = {p: device_ops(fn) for p, fn in paths}          # (after the timing: a profiler session is not free)
            for path, (med, lo, hi, peak) in res.items():
                rec = dict(run=run, case=name, **info, path=path, ms_median=round(med, 4), ms_min=round(lo, 4),
                           ms_max=round(hi, 4), windows=args.rounds, iters=args.iters, device_ops=ops[path],
                           peak_MB=round(peak / 2 ** 20, 2))
                if path == "torch":
                    rec.update(torch_over_native=round(med / res["native"][0], 2), **parity)
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/diffusion_time.py: the training criterion (forward and backward, a gradient through x0) and one "
                "aggregation-sampling step around the network (gather, stitch, p_sample; the network left out of both "
                "paths), the native path beside the reference's torch lines, per call, on the MI355X; device_ops: device "
                "activities of one call.  The share of a whole step is not measured: no U-Net runs here without weights.\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
