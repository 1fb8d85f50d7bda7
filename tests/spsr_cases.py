"""The shapes and contents of the GPU tests of SPSR's gradient map and its losses (tests/test_gpu_spsr.py), on the CPU:
the smallest at which the kernels of ssl_amd/csrc/ssg_spsr.hip can go wrong.  Every case is a pair (x, t) of fp32
(B,C,H,W) tensors: the image under the gradient and the target."""
import torch

import spsr_reference as R

WORKGROUP, PER_THREAD = 256, 4          # the forward kernels' threads and elements per thread and trip
TRIP_H, TRIP_W = 127, 131               # odd sides: groups of four straddle rows and planes


def trip_shape(cap):
    """(1, planes, H, W) with more than (2 cap - 1) workgroups' worth of elements -- every workgroup of the capped grid
    walks a second time -- and a count that is no multiple of four, so a scalar tail remains."""
    per = WORKGROUP * PER_THREAD
    planes = ((2 * cap - 1) * per + 5) // (TRIP_H * TRIP_W) + 1
    while planes * TRIP_H * TRIP_W % PER_THREAD == 0:
        planes += 1
    return (1, planes, TRIP_H, TRIP_W)


# name -> (B, C, H, W); 'view': 4-byte-aligned offset views of larger buffers; 'mixed': the target alone is such a view, so
# the two tensors of a call differ in alignment; 'strided': non-contiguous views; 'folded': more than one workgroup
SHAPES = {"1x1x1x1": (1, 1, 1, 1), "1x1x1x7": (1, 1, 1, 7), "1x1x7x1": (1, 1, 7, 1), "1x2x2x2": (1, 2, 2, 2),
          "2x3x9x11": (2, 3, 9, 11), "1x3x5x64": (1, 3, 5, 64), "1x3x5x65": (1, 3, 5, 65), "view": (2, 3, 9, 12),
          "mixed": (2, 3, 9, 12), "strided": (2, 3, 9, 11), "folded": (2, 3, 20, 23)}
CONTENTS = ("uniform", "flat", "step", "checker", "same")
# the layouts that start k floats into a buffer; HEADS_SHAPE's 11 elements at k = 1, 2, 3 leave a head of 3, 2, 1, two
# groups of four and a tail of 0, 1, 2
OFFSET_VIEWS = {"view": 1, "view2": 2, "view3": 3}
HEADS_SHAPE = (1, 1, 1, 11)


def content(name, shape, seed=0):
    """(x, t) fp32 on the CPU."""
    g = torch.Generator().manual_seed(3300 + seed)
    B, C, H, W = shape
    rand = lambda: torch.rand(shape, generator=g, dtype=torch.float64).to(torch.float32)   # noqa: E731
    if name == "uniform":
        return rand(), rand()
    if name == "flat":                  # m = sqrt(1e-6) in the interior, the gradient exactly 0 there
        return torch.full(shape, 0.5), torch.full(shape, 0.25)
    ii, jj = torch.arange(H).reshape(H, 1).expand(H, W), torch.arange(W).reshape(1, W).expand(H, W)
    if name == "step":                  # a vertical edge against a horizontal one
        return ((jj >= W // 2).float().expand(shape).contiguous(), (ii >= H // 2).float().expand(shape).contiguous())
    if name == "checker":
        return ((ii + jj) % 2).float().expand(shape).contiguous(), rand()
    if name == "same":                  # the map difference is exactly 0 everywhere: L1's sign(0)
        x = rand()
        return x, x.clone()
    raise KeyError(name)


def place(t, how, dev):
    """The CPU tensor t on the device as the case `how` wants it laid out."""
    if how in OFFSET_VIEWS:             # k floats behind a 16-byte boundary: a scalar head of 4 - k elements
        k = OFFSET_VIEWS[how]
        buf = torch.zeros(t.numel() + 5, dtype=torch.float32, device=dev)
        v = buf[k:k + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * k and v.is_contiguous()
        return v
    if how == "strided":                # every second column of a buffer twice as wide
        buf = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=torch.float32, device=dev)
        v = buf[..., ::2]
        v.copy_(t)
        assert not v.is_contiguous()
        return v
    return t.to(dev)


def isolation_batch(seed=0):
    """A (1, 3, 9, 11) batch whose planes differ by orders of magnitude, 1e-3, 1 and 1e3: a stencil that reads across a
    plane boundary changes a neighbour's map by far more than a rounding."""
    x, t = content("uniform", (1, 3, 9, 11), seed)
    s = torch.tensor([1e-3, 1.0, 1e3]).reshape(1, 3, 1, 1)
    return x * s, t * s


def cotangent(shape, seed=0):
    g = torch.Generator().manual_seed(4400 + seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(torch.float32)


def branch_for(t, seed=0):
    """What a gradient branch puts out for the target t: its map plus noise."""
    g = torch.Generator().manual_seed(5500 + seed)
    return (R.gmap(t) + 0.05 * torch.randn(t.shape, generator=g, dtype=torch.float64)).to(torch.float32)
