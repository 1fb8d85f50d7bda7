#!/usr/bin/env python3
"""Bits of the streaming and ragged criteria and of the multi-tensor EMA, recorded per library and compared: what
profiles/chunked_refactor_bits.txt holds.  One process records one library (a fresh process per run):

    python tools/chunked_bits.py record OUT.npz [--csrc DIR]     DIR holds libssg_hip.so (default: ssl_amd/csrc)
    python tools/chunked_bits.py compare PARENT1.npz PARENT2.npz CHANGE.npz [--out FILE]

Items: every tensor of test_gpu_perceptual / test_gpu_gan / test_gpu_spsr .poison_cases(), and one EMA run over a set of
tensors of 0 .. 8,197 elements in which every alignment of dst and of src occurs (src shares dst's alignment in a
quarter of the pairs), SSG_MT_EMA, then _LIT, then _COPY on the same tensors, the set read back after each."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

EMA_SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 1023, 1027, 4093, 4095, 4096, 4097, 4099, 8191, 8192, 8193, 8197]


def ema_items(dev):
    import torch
    from ssl_amd import _lib, ema
    gen = torch.Generator().manual_seed(11)
    pairs = []
    for i, n in enumerate(EMA_SIZES * 4):                      # dst at i % 4 floats past a boundary, src at (i // 4 + i) % 4
        e, p = (torch.randn(n + 8, generator=gen).to(dev) for _ in range(2))
        pairs.append((e[i % 4:i % 4 + n], p[(i // 4 + i) % 4:(i // 4 + i) % 4 + n]))
    table, n_chunks, _ = ema.build_table([e.data_ptr() for e, _ in pairs], [p.data_ptr() for _, p in pairs],
                                         [e.numel() for e, _ in pairs], dev)
    w = torch.tensor([0.0123], dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, kind, d, a, wd in (("ema", ema.EMA, 0.999, 1 - 0.999, None), ("lit", ema.LIT, 0.0, 0.0, w.data_ptr()),
                                 ("copy", ema.COPY, 0.0, 0.0, None)):
        _lib.check(_lib.lib().ssg_multi_apply(table.data_ptr(), n_chunks, kind, d, a, wd, stream))
        torch.cuda.synchronize()
        out[f"ema/{name}"] = torch.cat([e for e, _ in pairs]).cpu().numpy()
    return out


def record(args):
    import torch
    from ssl_amd import _lib
    if args.csrc:
        _lib.SO_PATH = os.path.join(os.path.abspath(args.csrc), "libssg_hip.so")
        _lib.PROF_SO_PATH = os.path.join(os.path.abspath(args.csrc), "libssg_hip_prof.so")
    items = {}
    for mod in ("test_gpu_perceptual", "test_gpu_gan", "test_gpu_spsr"):
        for k, t in enumerate(__import__(mod).poison_cases()):
            items[f"{mod[9:]}/{k:03d}"] = t.detach().cpu().numpy()
    items.update(ema_items(torch.device("cuda:0")))
    np.savez(args.out, **items)
    print(f"{len(items)} items of {_lib.SO_PATH} -> {args.out}")


def compare(args):
    p1, p2, ch = (dict(np.load(f)) for f in (args.parent1, args.parent2, args.change))
    same = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()   # noqa: E731
    unstable = [k for k in p1 if not same(p1[k], p2[k])]
    lines = [f"items recorded: {len(p1)}", f"parent differs from itself on {len(unstable)} item(s): {unstable}"]
    different = 0
    assert sorted(p1) == sorted(p2) == sorted(ch)
    for k in sorted(p1):
        if k in unstable:
            lines.append(f"  {k:<22} {str(p1[k].shape):<14} not compared bit for bit (parent vs parent differs)")
            continue
        eq = same(p1[k], ch[k])
        different += not eq
        lines.append(f"  {k:<22} {str(p1[k].shape):<14} {p1[k].dtype} nan={int(np.isnan(p1[k]).sum())} "
                     + ("EQUAL" if eq else "DIFFERENT"))
    lines.append(f"compared {len(p1) - len(unstable)} items, {different} different")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if different or unstable else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("out")
    r.add_argument("--csrc", default="")
    c = sub.add_parser("compare")
    c.add_argument("parent1"), c.add_argument("parent2"), c.add_argument("change")
    c.add_argument("--out", default="")
    args = ap.parse_args()
    sys.exit(record(args) if args.cmd == "record" else compare(args))
