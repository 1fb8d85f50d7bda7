#!/usr/bin/env python3
"""SwinIR's window attention timed: torch's lines beside the fused call (ssl_amd.winattn -> ssg_winattn_forward /
ssg_winattn_backward), on the same GPU in the same run.

Paths, at the reference's training shape (options/train/SwinIRGANSSL/train_SwinIRGANSSL_bicubic_x4.yml: 4 images of
64 x 64 tokens, embed_dim 180, 6 heads of 30, window 8):
    c_forward_s0 / _s4, c_backward_s0 / _s4     the bare launches on preallocated tensors, shifts 0 and 4, against
                                                their byte floor: qkv read + out written (47.2 MB) and qkv + dout read +
                                                dqkv written (94.4 MB) at the 6.3 TB/s measured for streaming kernels
    block_fwd_torch / _fused                    one SwinTransformerBlock (shift 4) forward under no_grad
    block_fwd_bwd_torch / _fused                its forward + backward
    net_fwd_bwd_torch / _fused                  the whole SwinIR-M (depths 6 x 6, x4, pixelshuffle) forward + backward at
                                                4 x 3 x 64 x 64, eval() so that DropPath draws nothing
A warm-up, then `--rounds` alternating windows of `--iters` back-to-back calls each, device events around a window:
`ms_*` is the time per call of a window, so the larger of the host's and the device's time.  `host_ms` is the host's time
per call alone; `device_ops` and `device_busy_us` are the device activities torch's profiler records for one call and the
sum of their durations; `peak_MB` is the allocator's peak above the level before the call.

    python tools/winattn_time.py [--iters N] [--rounds R] [--warmup W] [--out FILE] [--append] [--no-net]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from ema_time import STREAM_BYTES_PER_S, record  # noqa: E402
from specnorm_time import report  # noqa: E402

B, H, W, HEADS, D = 4, 64, 64, 6, 30
C = HEADS * D


def time_bare(dev, args, lines):
    from ssl_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(1)
    qkv = torch.randn((B, H, W, 3 * C), generator=gen).to(dev)
    table = torch.randn((225, HEADS), generator=gen).to(dev)
    dout = torch.randn((B, H, W, C), generator=gen).to(dev)
    out, dqkv, dtable = torch.empty_like(dout), torch.empty_like(qkv), torch.empty_like(table)
    nbytes = L.ssg_winattn_workspace_bytes(B, H, W, HEADS, D)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    scale = D ** -0.5
    record(lines, what="bare", shape=[B, H, W], heads=HEADS, head_dim=D, units=B * (H // 8) * (W // 8) * HEADS,
           workgroups=nbytes // (8 * 225), grid_cap=L.ssg_winattn_grid_cap())

    def forward(shift):
        return lambda: _lib.check(L.ssg_winattn_forward(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W, HEADS,
                                                        D, shift, scale, stream))

    def backward(shift):
        return lambda: _lib.check(L.ssg_winattn_backward(qkv.data_ptr(), table.data_ptr(), dout.data_ptr(), dqkv.data_ptr(),
                                                         dtable.data_ptr(), ws.data_ptr(), nbytes, B, H, W, HEADS, D, shift,
                                                         scale, stream))

    floor = {"c_forward": 4 * (qkv.numel() + out.numel()) / STREAM_BYTES_PER_S * 1e3,
             "c_backward": 4 * (2 * qkv.numel() + dout.numel()) / STREAM_BYTES_PER_S * 1e3}

    def floors(path, med):
        ms = floor[path[:-3]]
        return dict(byte_floor_ms=round(ms, 5), floor_share=round(ms / med, 4))

    paths = [("c_forward_s0", forward(0)), ("c_forward_s4", forward(4)), ("c_backward_s0", backward(0)),
             ("c_backward_s4", backward(4))]
    report(lines, "bare", paths, args, floors)


def time_block(dev, args, lines):
    from ssl_amd import archs
    torch.manual_seed(2)
    blocks = {}
    for tag, fused in (("torch", False), ("fused", True)):
        blk = archs.SwinTransformerBlock(C, (H, W), HEADS, window_size=8, shift_size=4, mlp_ratio=2.0, fused=fused)
        if blocks:
            blk.load_state_dict(blocks["torch"].state_dict())
        blocks[tag] = blk.to(dev).eval()
    x = torch.randn(B, H * W, C, device=dev)
    xg = x.clone().requires_grad_(True)

    def fwd(blk):
        def run():
            with torch.no_grad():
                return blk(x, (H, W))
        return run

    def fwd_bwd(blk):
        def run():
            for p in blk.parameters():
                p.grad = None
            xg.grad = None
            blk(xg, (H, W)).mean().backward()
        return run

    paths = [("block_fwd_torch", fwd(blocks["torch"])), ("block_fwd_fused", fwd(blocks["fused"])),
             ("block_fwd_bwd_torch", fwd_bwd(blocks["torch"])), ("block_fwd_bwd_fused", fwd_bwd(blocks["fused"]))]
    res = report(lines, "block", paths, args)
    record(lines, what="block", fwd_torch_over_fused=round(res["block_fwd_torch"][0] / res["block_fwd_fused"][0], 3),
           fwd_bwd_torch_over_fused=round(res["block_fwd_bwd_torch"][0] / res["block_fwd_bwd_fused"][0], 3))


def time_net(dev, args, lines):
    from ssl_amd import archs
    cfg = dict(upscale=4, in_chans=3, img_size=64, window_size=8, img_range=1.0, depths=[6] * 6, embed_dim=C,
               num_heads=[HEADS] * 6, mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")
    torch.manual_seed(3)
    plain = archs.SwinIR(fused=False, **cfg)
    fused = archs.SwinIR(fused=True, **cfg)
    fused.load_state_dict(plain.state_dict())
    plain, fused = plain.to(dev).eval(), fused.to(dev).eval()
    x = torch.rand(B, 3, H, W, device=dev)

    def step(net):
        def run():
            for p in net.parameters():
                p.grad = None
            net(x).mean().backward()
        return run

    res = report(lines, "SwinIR-M 4x3x64x64", [("net_fwd_bwd_torch", step(plain)), ("net_fwd_bwd_fused", step(fused))], args)
    record(lines, what="SwinIR-M 4x3x64x64", torch_over_fused=round(res["net_fwd_bwd_torch"][0] / res["net_fwd_bwd_fused"][0], 3),
           saved_ms=round(res["net_fwd_bwd_torch"][0] - res["net_fwd_bwd_fused"][0], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winattn_time.txt"))
    ap.add_argument("--append", action="store_true", help="a further run of the tool into the same file")
    ap.add_argument("--no-net", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("winattn_time.py needs the MI355X")
    dev = torch.device("cuda:0")
    lines = []
    time_bare(dev, args, lines)
    time_block(dev, args, lines)
    if not args.no_net:
        net_args = argparse.Namespace(**dict(vars(args), iters=max(args.iters // 4, 3)))
        time_net(dev, net_args, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = ("# tools/winattn_time.py: SwinIR's window attention on the MI355X at the training shape (4 x 64 x 64 tokens, 6 "
            "heads of 30, window 8): the bare launches against their byte floor at 6.3 TB/s, one SwinTransformerBlock and "
            "the whole SwinIR-M forward + backward, torch's lines beside the fused call\n")
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("# a second run of the tool\n" if args.append else head) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
