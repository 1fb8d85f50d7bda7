#!/usr/bin/env python3
"""The GAN criteria timed, loss and gradient, per call form of a training iteration: the native path
(ssl_amd.losses.GANLoss on fp32 GPU tensors -> ssg_gan_sums / ssg_gan_grad) beside the torch expressions of the same
module on the same GPU (the reference's operations: the label tensor, the element-wise criterion, the means, the
subtraction and autograd's replay), and the bare C calls on preallocated buffers (what the kernels cost without the
Python around them).

Call forms, gan_type vanilla with loss_weight 0.1 as the reference's training files configure it:
    plain_generator        cri(fake, True).backward()
    plain_discriminator    cri(real, True, is_disc=True).backward(); cri(fake, False, is_disc=True).backward()
    relativistic_generator (cri(real - mean(fake), False) + cri(fake - mean(real), True)) / 2, real detached, .backward()
                           -- natively GANLoss.relativistic_generator(real, fake)
    relativistic_discriminator   the two 0.5 * cri(x - mean(other.detach()), ..., is_disc=True) lines, each .backward()
                           -- natively GANLoss.relativistic_term
Shapes: 16 x 1 x 256 x 256 (the U-Net discriminator's logits) and 16 x 1 (the VGG-style discriminator's), where only the
launch count differs.  A warm-up, then `--rounds` alternating windows of `--iters` calls each, device events around a
window; the median window and the min / max.  `device_ops` is the number of device activities (kernels, copies, memsets)
torch's profiler records for one call after the warm-up (null if the profiler is not available).  The byte floor at
8 TB/s: one read for the sums, one read and one store for the gradient, twelve bytes per element and tensor that gets a
gradient, four per tensor that does not (relativistic forms read each tensor once more for its mean).

    python tools/gan_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE]
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

HBM_BYTES_PER_S = 8e12   # MI355X


def device_ops(fn):
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    except Exception:       # noqa: BLE001 -- a count that cannot be taken is reported as null, the timings stand
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gan_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gan_time.py needs the MI355X")
    from ssl_amd import _lib
    from ssl_amd.losses import GANLoss
    from ssl_amd.losses import gan_loss as M
    dev = torch.device("cuda:0")
    L = _lib.lib()
    crit = GANLoss("vanilla", loss_weight=0.1)
    ref = crit._torch                        # the module's torch path: the reference's operations
    lines = []
    for shape in ((16, 1, 256, 256), (16, 1)):
        gen = torch.Generator().manual_seed(len(shape))
        real = (0.5 + 3 * torch.randn(shape, generator=gen)).to(dev).requires_grad_(True)
        fake = (-0.5 + 3 * torch.randn(shape, generator=gen)).to(dev).requires_grad_(True)
        n = real.numel()

        def clear():
            real.grad = fake.grad = None

        def n_plain_g():
            clear()
            crit(fake, True).backward()

        def t_plain_g():
            clear()
            ref(fake, True, False).backward()

        def n_plain_d():
            clear()
            crit(real, True, is_disc=True).backward()
            crit(fake, False, is_disc=True).backward()

        def t_plain_d():
            clear()
            ref(real, True, True).backward()
            ref(fake, False, True).backward()

        def n_rel_g():
            clear()
            crit.relativistic_generator(real.detach(), fake).backward()

        def t_rel_g():
            clear()
            r = real.detach()
            ((ref(r - torch.mean(fake), False, False) + ref(fake - torch.mean(r), True, False)) / 2).backward()

        def n_rel_d():
            clear()
            (crit.relativistic_term(real, fake.detach(), True, is_disc=True) * 0.5).backward()
            (crit.relativistic_term(fake, real.detach(), False, is_disc=True) * 0.5).backward()

        def t_rel_d():
            clear()
            (ref(real - torch.mean(fake.detach()), True, True) * 0.5).backward()
            (ref(fake - torch.mean(real.detach()), False, True) * 0.5).backward()

        # the bare C calls of the plain generator form: sums, then the gradient
        xd = fake.detach()
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        work = torch.empty(L.ssg_gan_workspace_bytes(), dtype=torch.uint8, device=dev)
        coef = torch.tensor([0.1 / n, 0.0], dtype=torch.float64, device=dev)
        grad = torch.empty_like(xd)
        stream = torch.cuda.current_stream().cuda_stream

        def c_calls():
            _lib.check(L.ssg_gan_sums(xd.data_ptr(), n, M.BCE, 1.0, 1.0, None, work.data_ptr(), sums.data_ptr(), stream))
            _lib.check(L.ssg_gan_grad(xd.data_ptr(), n, M.BCE, 1.0, 1.0, None, coef.data_ptr(), grad.data_ptr(), stream))

        # bytes: (tensors with a gradient, tensors read without one, extra reads for the means)
        forms = [("plain_generator", n_plain_g, t_plain_g, 12 * n),
                 ("plain_discriminator", n_plain_d, t_plain_d, 24 * n),
                 ("relativistic_generator", n_rel_g, t_rel_g, (12 + 4 + 8) * n),
                 ("relativistic_discriminator", n_rel_d, t_rel_d, (24 + 8) * n)]
        for name, native, reference, nbytes in forms:
            native()
            g_native = fake.grad.clone()
            reference()
            diff = float((g_native - fake.grad).abs().max() / fake.grad.abs().max())
            paths = [("native", native), ("torch", reference)] + ([("c_calls", c_calls)] if name == "plain_generator" else [])
            res = compare(paths, args.iters, args.rounds, args.warmup)
            ops = {p: device_ops(fn) for p, fn in paths}          # (after the timing: a profiler session is not free)
            floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
            for path, (med, lo, hi, peak) in res.items():
                rec = dict(form=name, shape=list(shape), path=path, ms_median=round(med, 4), ms_min=round(lo, 4),
                           ms_max=round(hi, 4), windows=args.rounds, iters=args.iters, device_ops=ops[path],
                           peak_MB=round(peak / 2 ** 20, 2), byte_floor_ms=round(floor_ms, 6),
                           floor_share=round(floor_ms / med, 4))
                if path == "torch":
                    rec.update(torch_over_native=round(med / res["native"][0], 2),
                               max_grad_diff_over_max_grad=diff)
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/gan_time.py: the GAN criterion (vanilla, loss_weight 0.1), loss and gradient, per call form: the "
                "native path, the module's torch expressions and (plain generator) the bare C calls, per call, all on the "
                "MI355X; device_ops: device activities of one call; byte_floor_ms: the form's bytes at 8 TB/s\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
