#!/usr/bin/env python3
"""SPSR's gradient-space terms of one generator step timed, loss and gradient, in four forms on the same GPU:

    torch     the four map calls (spsrssl_model.py:298-301) and the two criteria (:363 MSE, :368 L1) as the model writes
              them, in torch operations (ssl_amd.losses.spsr's torch path: the reference's operations), .backward()
    drop_in   the same lines on the native classes: Get_gradient, Get_gradient_nopadding, MSELoss, L1Loss
    fused     INTEGRATION.md's fused form: GradientLoss(...)(output, gt, return_map=True), one gradient_map(gt) under
              no_grad, GradientLoss('l1').branch(branch, gt)
    c_calls   the fused form's bare C calls on preallocated buffers: ssg_spsr_loss (map emitted), ssg_spsr_map,
              ssg_spsr_branch_loss, ssg_spsr_loss_backward, ssg_spsr_branch_grad

Shapes: 30 x 3 x 128 x 128 (the training file's batch and gt_size) and 16 x 3 x 256 x 256.  A warm-up, then `--rounds`
alternating windows of `--iters` calls each, device events around a window; the median window and the min / max.
`device_ops` is the number of device activities (kernels, copies, memsets) torch's profiler records for one call after
the warm-up (null if the profiler is not available).  The byte floor at 8 TB/s, fused form, four bytes per element and
access: forward reads output and gt and writes the SR map (3), the GT map reads gt and writes (2), the branch loss reads
branch and gt (2), the SR backward reads output and gt and writes the gradient (3), the branch gradient reads branch and
gt and writes (3): 52 bytes per element.

Then every C entry point alone on the same buffers (`path` "c:<name>", `accesses` = tensors read or written once, the
call's own byte floor beside it): windows of four times `--iters` back-to-back calls, alternating among the entry points.

    python tools/spsr_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE]
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
from gan_time import HBM_BYTES_PER_S, device_ops  # noqa: E402

W_GRADSR, W_BRANCH = 1e-2, 5e-1     # pixel_gradSR_opt, pixel_gradBranch_opt of train_SPSRSSL_bicubic_x4.yml


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spsr_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spsr_time.py needs the MI355X")
    from ssl_amd import _lib, engine
    from ssl_amd import losses as NL
    from ssl_amd.losses import spsr as M
    dev = torch.device("cuda:0")
    L = _lib.lib()
    MSE, L1 = engine.PIXEL_KINDS["mse"], engine.PIXEL_KINDS["l1"]
    get_grad, get_grad_nopadding = NL.Get_gradient(), NL.Get_gradient_nopadding()
    cri_sr, cri_br = NL.MSELoss(W_GRADSR), NL.L1Loss(W_BRANCH)
    fused_sr, fused_br = NL.GradientLoss("mse", W_GRADSR), NL.GradientLoss("l1", W_BRANCH)
    lines = []
    for shape in ((30, 3, 128, 128), (16, 3, 256, 256)):
        gen = torch.Generator().manual_seed(shape[0])
        gt = torch.rand(shape, generator=gen).to(dev)
        output = (gt + 0.1 * torch.randn(shape, generator=gen).to(dev)).requires_grad_(True)
        branch = (engine.gradient_map(gt) + 0.05 * torch.randn(shape, generator=gen).to(dev)).requires_grad_(True)
        n, planes, H, W = gt.numel(), shape[0] * shape[1], shape[2], shape[3]

        def clear():
            output.grad = branch.grad = None

        def t_model():
            clear()
            fake, var = M._torch_map(output), M._torch_map(gt)
            M._torch_map(gt), M._torch_map(gt)                  # var_ref_grad, var_H_grad_nopadding
            l_sr = M._torch_criterion("mse", fake, var, None, 0.0, W_GRADSR, "mean")
            l_br = M._torch_criterion("l1", branch, var, None, 0.0, W_BRANCH, "mean")
            (l_sr + l_br).backward()

        def n_drop_in():
            clear()
            fake, var = get_grad(output), get_grad(gt)
            get_grad(gt)
            nopad = get_grad_nopadding(gt)
            (cri_sr(fake, var) + cri_br(branch, nopad)).backward()

        def n_fused():
            clear()
            l_sr, fake = fused_sr(output, gt, return_map=True)
            with torch.no_grad():
                get_grad(gt)
            (l_sr + fused_br.branch(branch, gt)).backward()

        xd, bd = output.detach(), branch.detach()
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        work = torch.empty(2 * L.ssg_spsr_workspace_bytes(), dtype=torch.uint8, device=dev)
        coef = torch.tensor([W_GRADSR / n, W_BRANCH / n], dtype=torch.float64, device=dev)
        m_sr, m_gt, g_x, g_b = (torch.empty_like(gt) for _ in range(4))
        stream = torch.cuda.current_stream().cuda_stream
        half = L.ssg_spsr_workspace_bytes()

        def c_calls():
            p = lambda t, off=0: t.data_ptr() + off   # noqa: E731
            _lib.check(L.ssg_spsr_loss(p(xd), p(gt), planes, H, W, MSE, 0.0, p(m_sr), p(work), p(sums), stream))
            _lib.check(L.ssg_spsr_map(p(gt), planes, H, W, p(m_gt), stream))
            _lib.check(L.ssg_spsr_branch_loss(p(bd), p(gt), planes, H, W, L1, 0.0, p(work, half), p(sums, 8), stream))
            _lib.check(L.ssg_spsr_loss_backward(p(xd), p(gt), None, p(coef), planes, H, W, MSE, 0.0, p(g_x), stream))
            _lib.check(L.ssg_spsr_branch_grad(p(bd), p(gt), planes, H, W, L1, 0.0, p(coef, 8), p(g_b), stream))

        t_model()
        want = output.grad.clone()
        diffs = {}
        for name, fn in (("drop_in", n_drop_in), ("fused", n_fused)):
            fn()
            diffs[name] = float((output.grad - want).abs().max() / want.abs().max())
        c_calls()
        diffs["c_calls"] = float((g_x - want).abs().max() / want.abs().max())
        paths = [("torch", t_model), ("drop_in", n_drop_in), ("fused", n_fused), ("c_calls", c_calls)]
        res = compare(paths, args.iters, args.rounds, args.warmup)
        ops = {p: device_ops(fn) for p, fn in paths}          # (after the timing: a profiler session is not free)
        floor_ms = 52 * n / HBM_BYTES_PER_S * 1e3
        for path, (med, lo, hi, peak) in res.items():
            rec = dict(shape=list(shape), path=path, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                       windows=args.rounds, iters=args.iters, device_ops=ops[path], peak_MB=round(peak / 2 ** 20, 2),
                       byte_floor_ms=round(floor_ms, 6), floor_share=round(floor_ms / med, 4))
            if path != "torch":
                rec.update(torch_over_this=round(res["torch"][0] / med, 2), max_grad_diff_over_max_grad=diffs[path])
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        # every entry point alone: (call, tensors it reads or writes once)
        p = lambda t, off=0: t.data_ptr() + off   # noqa: E731
        one = lambda fn, *a: (lambda: _lib.check(fn(*a, stream)))   # noqa: E731
        dims = (planes, H, W)
        singles = [
            ("spsr_map", one(L.ssg_spsr_map, p(gt), *dims, p(m_gt)), 2),
            ("spsr_map_backward", one(L.ssg_spsr_map_backward, p(xd), p(bd), *dims, p(g_x)), 3),
            ("spsr_loss", one(L.ssg_spsr_loss, p(xd), p(gt), *dims, MSE, 0.0, None, p(work), p(sums)), 2),
            ("spsr_loss+map", one(L.ssg_spsr_loss, p(xd), p(gt), *dims, MSE, 0.0, p(m_sr), p(work), p(sums)), 3),
            ("spsr_loss_backward", one(L.ssg_spsr_loss_backward, p(xd), p(gt), None, p(coef), *dims, MSE, 0.0, p(g_x)), 3),
            ("spsr_loss_backward+grad_map",
             one(L.ssg_spsr_loss_backward, p(xd), p(gt), p(bd), p(coef), *dims, MSE, 0.0, p(g_x)), 4),
            ("spsr_branch_loss", one(L.ssg_spsr_branch_loss, p(bd), p(gt), *dims, L1, 0.0, p(work), p(sums)), 2),
            ("spsr_branch_grad", one(L.ssg_spsr_branch_grad, p(bd), p(gt), *dims, L1, 0.0, p(coef), p(g_b)), 3),
            ("pixel_sums", one(L.ssg_pixel_sums, p(xd), p(gt), n, MSE, 0.0, p(work), p(sums)), 2),
            ("pixel_grad", one(L.ssg_pixel_grad, p(xd), p(gt), n, MSE, 0.0, p(coef), p(g_x)), 3)]
        res = compare([(name, fn) for name, fn, _ in singles], 4 * args.iters, args.rounds, args.warmup)
        for name, _, accesses in singles:
            med, lo, hi, _ = res[name]
            floor_ms = 4 * accesses * n / HBM_BYTES_PER_S * 1e3
            line = json.dumps(dict(shape=list(shape), path="c:" + name, ms_median=round(med, 4), ms_min=round(lo, 4),
                                   ms_max=round(hi, 4), windows=args.rounds, iters=4 * args.iters, accesses=accesses,
                                   byte_floor_ms=round(floor_ms, 6), floor_share=round(floor_ms / med, 4)))
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/spsr_time.py: SPSR's gradient-space terms of a generator step (four maps, MSE on the SR map, L1 on "
                "the branch), loss and gradient, per call: the model's torch operations, the native drop-in classes, the "
                "fused form and its bare C calls, all on the MI355X; device_ops: device activities of one call; "
                "byte_floor_ms: the fused form's 52 bytes per element at 8 TB/s; then every C entry point alone (path "
                "c:<name>) with its own floor, four bytes per element and tensor it reads or writes\n"
                + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
