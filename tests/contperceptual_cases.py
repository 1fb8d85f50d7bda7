"""The inputs, stand-in modules and cases of the autoencoder criterion's fixture (tests/golden/
make_golden_contperceptual.py records them through the reference's contperceptual.py; tests/test_cpu_lpips_grad.py and
test_gpu_lpips_grad.py run ssl_amd.losses.contperceptual on the same).  torch on the CPU.

The stand-ins replace what the reference takes from taming: a small fixed perceptual module (a 3x3 convolution, the
mean squared feature difference per image as (N,1,1,1)) and a small fixed discriminator (two convolutions around a
LeakyReLU).  Their weights, the inputs and the parameters of the `last_layer` construction come from one generator and
are stored in the fixture, so the tests never depend on the generator's stream."""
import torch
import torch.nn.functional as F
from torch import nn

N, H, W = 2, 16, 16
DISC_START = 100

# name -> (optimizer_idx, disc_loss, kl_weight, global_step, disc_factor, last_layer in the graph)
CASES = {
    "gen_hinge_kl_late": (0, "hinge", 1e-6, 150, 1.0, True),
    "gen_vanilla_nokl_early": (0, "vanilla", 0.0, 50, 1.0, True),
    "gen_hinge_kl_factor0": (0, "hinge", 1e-6, 150, 0.0, True),
    "gen_hinge_nokl_detached_layer": (0, "hinge", 0.0, 150, 1.0, False),
    "disc_hinge_kl_late": (1, "hinge", 1e-6, 150, 1.0, True),
    "disc_vanilla_nokl_late": (1, "vanilla", 0.0, 100, 1.0, True),
    "disc_hinge_nokl_early": (1, "hinge", 0.0, 99, 1.0, True),
}


class StandInPerceptual(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3, padding=1)

    def forward(self, input, target):
        return ((torch.tanh(self.conv(input)) - torch.tanh(self.conv(target))) ** 2).mean([1, 2, 3], keepdim=True)


class StandInDiscriminator(nn.Module):
    def __init__(self, input_nc=3, n_layers=3, use_actnorm=False):
        super().__init__()
        self.main = nn.Sequential(nn.Conv2d(input_nc, 4, 3, stride=2, padding=1), nn.LeakyReLU(0.2),
                                  nn.Conv2d(4, 1, 3, padding=1))

    def forward(self, x):
        return self.main(x)


def make_inputs(seed=37):
    """every tensor the cases share, as a dict of fp32 CPU tensors"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    inputs = torch.rand(N, 3, H, W, generator=gen) * 2 - 1
    out = dict(inputs=inputs, base=(inputs + 0.2 * r(N, 3, H, W)).clamp(-1, 1), hidden=0.3 * r(N, 3, H, W),
               last_layer=0.5 * r(1, 3, 1, 1), posterior=0.5 * r(N, 8, 4, 4),
               perc_weight=0.4 * r(4, 3, 3, 3), perc_bias=0.1 * r(4),
               disc_w0=0.4 * r(4, 3, 3, 3), disc_b0=0.1 * r(4), disc_w1=0.8 * r(1, 4, 3, 3), disc_b1=0.1 * r(1))
    return out


def plug(loss, t, dtype=torch.float32, device="cpu"):
    """the stand-ins with the stored weights in place of the module's perceptual loss and discriminator"""
    perc, disc = StandInPerceptual(), StandInDiscriminator()
    with torch.no_grad():
        perc.conv.weight.copy_(t["perc_weight"]), perc.conv.bias.copy_(t["perc_bias"])
        disc.main[0].weight.copy_(t["disc_w0"]), disc.main[0].bias.copy_(t["disc_b0"])
        disc.main[2].weight.copy_(t["disc_w1"]), disc.main[2].bias.copy_(t["disc_b1"])
    for p in perc.parameters():
        p.requires_grad = False
    loss.perceptual_loss, loss.discriminator = perc.eval(), disc
    return loss.to(device=device, dtype=dtype)


def reconstructions(t, in_graph, dtype=torch.float32, device="cpu"):
    """(reconstructions with retain_grad, last_layer): base + hidden * last_layer elementwise, so that last_layer is in
    the graph of both the nll and the generator's term; in_graph=False hands the criterion a parameter of the same
    shape that the reconstruction was not formed from (the reference's RuntimeError branch)."""
    to = lambda x: x.to(device=device, dtype=dtype)
    last = to(t["last_layer"]).clone().requires_grad_(True)
    rec = to(t["base"]) + to(t["hidden"]) * last
    rec.retain_grad()
    if not in_graph:
        return rec, to(t["last_layer"]).clone().requires_grad_(True), last
    return rec, last, last


def run_case(loss, make_posterior, t, name, dtype=torch.float32, device="cpu"):
    """One case through a criterion module (the reference's or the package's) with the stand-ins plugged in: a dict of
    the loss, every log value and the gradients, as tensors on `device`."""
    idx, _, _, step, _, in_graph = CASES[name]
    to = lambda x: x.to(device=device, dtype=dtype)
    rec, last_arg, last = reconstructions(t, in_graph, dtype, device)
    post = make_posterior(to(t["posterior"]))
    for p in loss.parameters():
        p.grad = None
    value, log = loss(to(t["inputs"]), rec, post, idx, step, last_layer=last_arg, split="train")
    out = {"loss": value.detach()}
    out.update({"log_" + k.split("/")[1]: torch.as_tensor(v).detach() for k, v in log.items()})
    if value.requires_grad:
        value.backward()
    if idx == 0:
        out["grad_reconstructions"], out["grad_last_layer"] = rec.grad, last.grad
        out["grad_logvar"] = loss.logvar.grad
    elif loss.discriminator.main[0].weight.grad is not None:
        out["grad_disc_w0"] = loss.discriminator.main[0].weight.grad
    return out


def build(cls, name, **extra):
    _, disc_loss, kl_weight, _, disc_factor, _ = CASES[name]
    return cls(disc_start=DISC_START, logvar_init=0.25, kl_weight=kl_weight, disc_weight=0.5, disc_factor=disc_factor,
               perceptual_weight=0.8, disc_loss=disc_loss, **extra)
