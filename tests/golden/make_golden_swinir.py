"""Generate f38_swinir.npz FROM THE REFERENCE ITSELF: its SwinIR class, on the CPU.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_swinir.py <reference root>

GAN-Based-SR/basicsr/archs/arch_util.py and swinir_arch.py are loaded as the two modules of a package made here, so
that `from .arch_util import ...` finds its neighbour without running basicsr/archs/__init__.py (which imports every
architecture).  They import packages that are not installed where the fixture is made or that pull the whole of
basicsr in (torchvision, distutils, basicsr.*); nothing of them is used by SwinIR, so while the two files load, a finder
in sys.meta_path answers those imports with stand-in modules whose attributes are inert classes (as
make_golden_diffusion.py does); `ARCH_REGISTRY.register()` returns the class unchanged.

The configuration is tests/test_cpu_winattn.py's SMALL_NET: embed_dim 12, heads [2, 2], depths [2, 2], window 8, img_size
16, upscale 2, upsampler 'pixelshuffle', eval().  Stored, numbers and key names only (no reference source text):
  keys                the state dict's keys, in order
  sd_<i>              the tensor of keys[i]
  x_a, x_b            inputs 1 x 3 x 16 x 16 and 1 x 3 x 16 x 24 (the second takes calculate_mask(x_size))
  y_a, y_b            the outputs
  attn_a_<k>, attn_b_<k>   block k's WindowAttention output (windows, 64, 12), k in forward order
"""
import importlib
import importlib.abc
import importlib.machinery
import os
import sys
import types
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f38_swinir.npz")

SMALL = dict(img_size=16, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=8, upscale=2,
             upsampler="pixelshuffle")


class _Inert:
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        return self


class _Registry:
    def register(self, *args, **kwargs):
        return lambda cls: cls


class _StandIn(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name.endswith("_REGISTRY"):
            return _Registry()
        return type(name, (_Inert,), {})


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, names):
        self.names = set(names)

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] not in self.names:
            return None
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _StandIn(spec.name)

    def exec_module(self, module):
        pass


STAND_INS = ("torchvision", "distutils", "basicsr")


def load_reference(root):
    package = types.ModuleType("reference_archs")
    package.__path__ = [os.path.join(root, "GAN-Based-SR", "basicsr", "archs")]
    sys.modules["reference_archs"] = package
    finder = _Finder(STAND_INS)
    sys.meta_path.insert(0, finder)
    try:
        return importlib.import_module("reference_archs.swinir_arch")
    finally:
        sys.meta_path.remove(finder)


def main(root):
    arch = load_reference(root)
    torch.manual_seed(38)
    net = arch.SwinIR(**SMALL).eval()
    # the tables and biases start at (nearly) zero: give every tensor of the state dict values that matter
    gen = torch.Generator().manual_seed(3838)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(torch.randn(p.shape, generator=gen))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            elif name.endswith("qkv.weight"):
                p.copy_(0.5 * torch.randn(p.shape, generator=gen))
    store = {}
    sd = net.state_dict()
    store["keys"] = np.array(list(sd.keys()))
    for i, key in enumerate(sd):
        store[f"sd_{i}"] = sd[key].numpy()
    taps = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: taps.append(out.detach().numpy().copy()))
             for m in net.modules() if isinstance(m, arch.WindowAttention)]
    for tag, shape in (("a", (1, 3, 16, 16)), ("b", (1, 3, 16, 24))):
        x = torch.rand(shape, generator=gen)
        del taps[:]
        with torch.no_grad():
            y = net(x)
        store[f"x_{tag}"], store[f"y_{tag}"] = x.numpy(), y.numpy()
        for k, tap in enumerate(taps):
            store[f"attn_{tag}_{k}"] = tap
    for h in hooks:
        h.remove()
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes;", len(sd), "keys")


if __name__ == "__main__":
    main(sys.argv[1])
