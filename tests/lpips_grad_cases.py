"""The inputs of the LPIPS gradient's tests (tests/test_cpu_lpips_grad.py, test_gpu_lpips_grad.py,
test_gpu_lpips_grad_poison.py): synthetic feature sets.  torch on the CPU; the unit and the grid cap are arguments.

The shapes are the smallest at which the kernel takes another path: a unit is px pixel lanes (the power of two at or
above min(HW, 256)) times 256 / px channel slices, so HW = 1 (256 slices of one pixel), 9 (16 slices), 255 and 256 (one
unit, the first with a dead lane), 257 (a second unit of one live lane); C = 1 and 3 leave most slices without a
channel, 64 and 512 give every slice several; one layer has one unit more than the grid cap (the second trip)."""
import torch

# between them every C of (1, 3, 64, 512) and every HW of (1, 9, 255, 256, 257)
LAYERS_A = [(1, 1, 1), (3, 3, 3), (64, 15, 17), (512, 16, 16), (3, 257, 1)]
LAYERS_B = [(512, 1, 1), (64, 3, 3), (1, 5, 51), (3, 16, 16), (64, 257, 1)]


def cases(unit, cap):
    """(name, N, [(C, H, W)], content)"""
    big = cap * unit + 5                              # cap + 1 units: the grid makes a second trip
    return [
        ("k5_n3_relu", 3, LAYERS_A, "relu"),
        ("k5_n1_relu", 1, LAYERS_B, "relu"),
        ("k1_n3_c512_hw9", 3, [(512, 3, 3)], "relu"),
        ("k1_n1_c64_hw256", 1, [(64, 16, 16)], "relu"),
        ("k5_n1_magnitudes", 1, LAYERS_B, "magnitudes"),
        ("k5_n3_identical", 3, LAYERS_A, "identical"),
        ("k5_n1_near_equal", 1, LAYERS_A, "near"),
        ("k1_n1_second_trip", 1, [(2, 1, big)], "relu"),
    ]


def maps(N, layers, content, seed=5):
    """(feats0, feats1, lins, coef): post-ReLU maps.  'relu' zeroes whole vectors on one side and on both at chosen
    pixels (and a one-channel layer's own zeros are zero vectors too); 'magnitudes' scales the layers from 1e-3 to
    1e2; 'identical' f1 = f0 > 0; 'near' f1 = f0 (1 + 1e-6 delta), f0 > 0."""
    gen = torch.Generator().manual_seed(seed)
    f0s, f1s, ws = [], [], []
    for k, (C, H, W) in enumerate(layers):
        scale = 10.0 ** (-3 + 5 * k / max(len(layers) - 1, 1)) if content == "magnitudes" else 1.0
        f0 = torch.relu(torch.randn(N, C, H, W, generator=gen) + 0.3) * scale
        if content in ("identical", "near"):
            f0 = f0 + 0.05
            f1 = f0.clone() if content == "identical" else f0 * (1 + 1e-6 * torch.randn(N, C, H, W, generator=gen))
        else:
            f1 = torch.relu(f0 + 0.4 * scale * torch.randn(N, C, H, W, generator=gen))
            pick = torch.rand(N, 1, H, W, generator=gen)
            f0 = torch.where(pick < 0.1, torch.zeros_like(f0), f0)                      # one side, and (< 0.05) both
            f1 = torch.where((pick < 0.05) | (pick > 0.95), torch.zeros_like(f1), f1)
        f0s.append(f0.contiguous()), f1s.append(f1.contiguous())
        ws.append(torch.rand(C, generator=gen) * 0.5)                                   # v0.1's weights are not negative
    coef = 0.5 + torch.rand(N, generator=gen)
    if N > 1:
        coef[1] = -coef[1]                                                              # an upstream gradient of either sign
    return f0s, f1s, ws, coef


def images(shape, seed=13):
    """(input, target) in [-1, 1]"""
    gen = torch.Generator().manual_seed(seed)
    target = torch.rand(shape, generator=gen) * 2 - 1
    return (target + 0.2 * torch.randn(shape, generator=gen)).clamp(-1, 1), target
