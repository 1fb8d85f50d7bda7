"""The inputs of the perceptual criterion's tests (tests/test_gpu_perceptual.py, test_gpu_perceptual_poison.py,
test_cpu_perceptual.py): pair sizes around the chunk, sets of K pairs, VGG's feature shapes, random torchvision-format
VGG weights.  torch on the CPU, nothing of ssl_amd; the chunk size and the grid cap are arguments."""
import torch

KINDS = ("l1", "mse", "charbonnier", "fro")
EPS = 1e-6
VGG19_TAPS = ("conv1_2", "conv2_2", "conv3_4", "conv4_4", "conv5_4")
VGG19_TAP_INDICES = (2, 7, 16, 25, 34)
KAIR_WEIGHTS = (0.1, 0.1, 1.0, 1.0, 1.0)
IMAGE_SHAPE = (2, 3, 32, 32)


def edge_sizes(chunk):
    """1, 3, 4, 5 (heads and tails alone), and one element either side of a chunk and of two"""
    return [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]


def second_trip_sizes(chunk, cap):
    """cap chunk + chunk + 5 elements in three pairs: cap + 2 chunks, so the grid of `cap` workgroups makes a second trip"""
    sizes = [(cap - 24) * chunk, 24 * chunk + 5, chunk]
    assert sum(sizes) == cap * chunk + chunk + 5
    return sizes


def vgg_feature_shapes(image=IMAGE_SHAPE):
    """the five tapped vgg19 features of an image batch: 32 : 16 : 8 : 4 : 1 in size"""
    b, _, h, w = image
    return [(b, c, h >> s, w >> s) for s, c in enumerate((64, 128, 256, 512, 512))]


def pair(shape, seed, spread=0.25):
    """(x, g): features after a ReLU-free conv are signed; g is x moved by a fraction of its spread, with a few exactly
    equal elements"""
    gen = torch.Generator().manual_seed(seed)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    g = torch.randn(shape, generator=gen)
    x = g + spread * torch.randn(shape, generator=gen)
    same = torch.rand(shape, generator=gen) < 0.05
    return torch.where(same, g, x), g


def pairs(shapes, seed):
    xs, gs = zip(*(pair(s, seed + 17 * i) for i, s in enumerate(shapes)))
    return list(xs), list(gs)


def weights(K, seed=5):
    """weights of both signs, one of them 0 (K >= 3)"""
    gen = torch.Generator().manual_seed(seed)
    w = (0.1 + torch.rand(K, generator=gen)).tolist()
    if K >= 3:
        w[1], w[2] = 0.0, -w[2]
    return w


def vgg_state_dict(vgg_type="vgg19", seed=0, names=None):
    """random weights in torchvision's format, `features.N.weight`: He-scaled convolutions so that the activations keep
    their size through the depth, batch-norm statistics near the identity"""
    from ssl_amd.losses.perceptual import vgg_layer_names
    gen = torch.Generator().manual_seed(seed)
    state, width = {}, 3
    for i, name in enumerate(names or vgg_layer_names(vgg_type)):
        if name.startswith("conv"):
            out = (64, 128, 256, 512, 512)[int(name[4]) - 1]
            state[f"features.{i}.weight"] = torch.randn(out, width, 3, 3, generator=gen) * (2.0 / (9 * width)) ** 0.5
            state[f"features.{i}.bias"] = 0.1 * torch.randn(out, generator=gen)
            width = out
        elif name.startswith("bn"):
            state[f"features.{i}.weight"] = 1 + 0.1 * torch.randn(width, generator=gen)
            state[f"features.{i}.bias"] = 0.1 * torch.randn(width, generator=gen)
            state[f"features.{i}.running_mean"] = 0.1 * torch.randn(width, generator=gen)
            state[f"features.{i}.running_var"] = 1 + 0.1 * torch.rand(width, generator=gen)
    return state


def images(seed=11):
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand(IMAGE_SHAPE, generator=gen)
    x = (gt + 0.1 * torch.randn(IMAGE_SHAPE, generator=gen)).clamp(0, 1)
    return x, gt
