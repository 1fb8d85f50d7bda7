"""The inputs of the LPIPS / DISTS criteria's tests (tests/test_cpu_featmetric.py, test_gpu_featmetric.py,
test_gpu_featmetric_poison.py): synthetic feature sets, random weights in the packages' key layouts.  torch on the
CPU; the unit, the chunk and the grid cap are arguments."""
import torch

ALEX_CONVS = {0: (64, 3, 11), 3: (192, 64, 5), 6: (384, 192, 3), 8: (256, 384, 3), 10: (256, 256, 3)}
ALEX_SLICE = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}
ALEX_CHANNELS = (64, 192, 384, 256, 256)
VGG16_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG16_WIDTH = {0: 64, 2: 64, 5: 128, 7: 128, 10: 256, 12: 256, 14: 256, 17: 512, 19: 512, 21: 512, 24: 512, 26: 512, 28: 512}
VGG_CHANNELS = (64, 128, 256, 512, 512)
DISTS_CHANNELS = (3, 64, 128, 256, 512, 512)
IMAGE_SHAPES = ((2, 3, 64, 64), (1, 3, 67, 45))


def _slice_of_vgg(i):
    return 1 + sum(i > e for e in (3, 8, 15, 22))


# ---- LPIPS feature sets: (name, N, [(C, H, W)], content) ----
def lpips_cases(unit, cap):
    big = cap * unit + unit + 5                     # cap + 2 units: the grid makes a second trip
    assert big % 5 == 0
    cs = (1, 3, 64, 65, 192, 512)
    hw = ((1, 1), (3, 3), (7, 5), (unit + 1, 1))
    k16 = [(cs[i % 6], *hw[(i // 2) % 4]) for i in range(16)]
    return [
        ("k5_n3_relu", 3, [(1, 1, 1), (3, 3, 3), (64, 7, 5), (65, unit + 1, 1), (192, 3, 3)], "relu"),
        ("k16_n1_magnitudes", 1, k16, "magnitudes"),
        ("k1_n3_c512", 3, [(512, 3, 3)], "relu"),
        ("k1_n1_second_trip", 1, [(3, 5, big // 5)], "relu"),
        ("k5_n3_identical", 3, [(1, 1, 1), (3, 3, 3), (64, 7, 5), (65, unit + 1, 1), (192, 3, 3)], "identical"),
        ("k5_n1_near_equal", 1, [(3, 3, 3), (64, 7, 5), (65, unit + 1, 1), (192, 3, 3), (512, 1, 1)], "near"),
    ]


def lpips_maps(N, layers, content, seed=3):
    """(feats0, feats1, lins): post-ReLU maps; 'relu' zeroes whole vectors on one side and on both at some pixels;
    'magnitudes' scales the layers from 1e-3 to 1e2; 'identical' f1 = f0; 'near' f1 = f0 (1 + 1e-4 delta)."""
    gen = torch.Generator().manual_seed(seed)
    f0s, f1s, ws = [], [], []
    for k, (C, H, W) in enumerate(layers):
        scale = 10.0 ** (-3 + 5 * k / max(len(layers) - 1, 1)) if content == "magnitudes" else 1.0
        f0 = torch.relu(torch.randn(N, C, H, W, generator=gen) + 0.3) * scale
        if content == "identical":
            f1 = f0.clone()
        elif content == "near":
            f1 = f0 * (1 + 1e-4 * torch.randn(N, C, H, W, generator=gen))
        else:
            f1 = torch.relu(f0 + 0.4 * scale * torch.randn(N, C, H, W, generator=gen))
        if content in ("relu", "magnitudes"):
            pick = torch.rand(N, 1, H, W, generator=gen)
            f0 = torch.where(pick < 0.1, torch.zeros_like(f0), f0)                      # one side, and (< 0.05) both
            f1 = torch.where((pick < 0.05) | (pick > 0.95), torch.zeros_like(f1), f1)
        f0s.append(f0.contiguous()), f1s.append(f1.contiguous())
        ws.append(torch.rand(C, generator=gen) * 0.5)                                   # v0.1's weights are not negative
    return f0s, f1s, ws


# ---- DISTS feature sets ----
def dists_cases(chunk):
    edge = [(3, 1, 1), (5, 2, 1), (3, 15, 17), (2, 3, (chunk + 1) // 3), (2, 37, (2 * chunk + 7) // 37)]
    assert edge[3][1] * edge[3][2] == chunk + 1 and edge[4][1] * edge[4][2] == 2 * chunk + 7
    real = [(c, 2, 2) for c in DISTS_CHANNELS]
    return [
        ("edges_n3_noise", 3, edge, "noise"),
        ("edges_n1_constant", 1, edge, "constant"),
        ("edges_n2_offset", 2, edge, "offset"),
        ("edges_n2_same", 2, edge, "same"),
        ("edges_n1_negated", 1, edge, "negated"),
        ("real_channels_n2", 2, real, "noise"),
    ]


def dists_maps(N, layers, content, seed=7):
    """(xs, ys, alpha, beta): 'noise' post-ReLU maps; 'constant' planes; 'offset' 100 + 1e-3 noise; 'same' y = x;
    'negated' y = -x."""
    gen = torch.Generator().manual_seed(seed)
    xs, ys = [], []
    for C, H, W in layers:
        x = torch.relu(torch.randn(N, C, H, W, generator=gen) + 0.5)
        y = torch.relu(x + 0.3 * torch.randn(N, C, H, W, generator=gen))
        if content == "constant":
            x = torch.rand(N, C, 1, 1, generator=gen).expand(N, C, H, W)
            y = torch.rand(N, C, 1, 1, generator=gen).expand(N, C, H, W)
        elif content == "offset":
            x = 100 + 1e-3 * torch.randn(N, C, H, W, generator=gen)
            y = 100 + 1e-3 * torch.randn(N, C, H, W, generator=gen)
        elif content == "same":
            y = x.clone()
        elif content == "negated":
            y = -x
        xs.append(x.contiguous()), ys.append(y.contiguous())
    total = sum(c for c, _, _ in layers)
    return xs, ys, 0.05 + torch.rand(total, generator=gen), 0.05 + torch.rand(total, generator=gen)


# ---- random weights in the packages' own key layouts and as torchvision trunk + small file ----
def _conv(gen, out, cin, k):
    return (torch.randn(out, cin, k, k, generator=gen) * (2.0 / (k * k * cin)) ** 0.5, 0.1 * torch.randn(out, generator=gen))


def lpips_state(net, seed=0):
    """(package layout, torchvision trunk dict, the package's small lin file) of one random LPIPS network"""
    gen = torch.Generator().manual_seed(seed)
    package, trunk, small = {}, {}, {}
    if net == "alex":
        convs = [(i, *ALEX_CONVS[i], ALEX_SLICE[i]) for i in ALEX_CONVS]
        chans = ALEX_CHANNELS
    else:
        convs, width = [], 3
        for i in VGG16_CONVS:
            convs.append((i, VGG16_WIDTH[i], width, 3, _slice_of_vgg(i)))
            width = VGG16_WIDTH[i]
        chans = VGG_CHANNELS
    for i, out, cin, k, sl in convs:
        w, b = _conv(gen, out, cin, k)
        package[f"net.slice{sl}.{i}.weight"], package[f"net.slice{sl}.{i}.bias"] = w, b
        trunk[f"features.{i}.weight"], trunk[f"features.{i}.bias"] = w, b
    for k, c in enumerate(chans):
        lin = torch.rand(1, c, 1, 1, generator=gen) / c
        package[f"lin{k}.model.1.weight"] = package[f"lins.{k}.model.1.weight"] = small[f"lin{k}.model.1.weight"] = lin
    package["scaling_layer.shift"] = torch.Tensor([-.030, -.088, -.188])[None, :, None, None]
    package["scaling_layer.scale"] = torch.Tensor([.458, .448, .450])[None, :, None, None]
    return package, trunk, small


def dists_state(seed=1):
    """(package layout, torchvision trunk dict, the package's small alpha / beta file) of one random DISTS network"""
    gen = torch.Generator().manual_seed(seed)
    package, trunk, small, width = {}, {}, {}, 3
    for i in VGG16_CONVS:
        w, b = _conv(gen, VGG16_WIDTH[i], width, 3)
        width = VGG16_WIDTH[i]
        package[f"stage{_slice_of_vgg(i)}.{i}.weight"], package[f"stage{_slice_of_vgg(i)}.{i}.bias"] = w, b
        trunk[f"features.{i}.weight"], trunk[f"features.{i}.bias"] = w, b
    total = sum(DISTS_CHANNELS)
    small["alpha"] = package["alpha"] = 0.1 + 0.01 * torch.randn(1, total, 1, 1, generator=gen).abs()
    small["beta"] = package["beta"] = 0.1 + 0.01 * torch.randn(1, total, 1, 1, generator=gen).abs()
    return package, trunk, small


def images(shape, seed=11):
    """(sr, gt) in [0, 1]"""
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=gen)
    return (gt + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1), gt


def val_metrics_block():
    """the `val.metrics` block of the reference's options/train/*SSL/*.yml files, key for key (the options/test files
    have the same block without the two `better` entries)"""
    return {"psnr": dict(type="calculate_psnr", crop_border=4, test_y_channel=True),
            "ssim": dict(type="calculate_ssim", crop_border=4, test_y_channel=True),
            "lpips": dict(type="calculate_lpips", crop_border=4, better="lower"),
            "dists": dict(type="calculate_dists", crop_border=4, better="lower")}
