"""What the CPU and GPU tests of the ragged degradation chain share: the replay of recorded decisions, the mapping of a
program's stages onto the fixture's events, the case lists, and the live oracles with the share of the derived bound
that each one's own float32 result uses (profiles/blindsr_parity.txt)."""
import os

import numpy as np

import blindsr_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f35_blindsr.npz")
EVENT_KINDS = ["conv", "resize", "gaussian", "speckle", "poisson", "jpeg", "imresize"]

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = dict(np.load(GOLDEN))
    return _fixture


def scripted_draws(kinds, vals, lens, names, fields=None):
    """A BlindSRDraws that replays a recorded log: every call must be the method the log holds next (so the ORDER of the
    draws is checked too) and returns the recorded value.  `fields`: a numpy Generator the noise fields are taken from
    (as float32 tensors on the asked device); every field handed out is kept in `.given`."""
    import torch
    from ssl_amd.blindsr import BlindSRDraws
    starts = np.concatenate([[0], np.cumsum(lens)])

    class Scripted(BlindSRDraws):
        def __init__(self):
            self.at, self.given = 0, []

        def _next(self, kind):
            assert self.at < len(kinds), f"draw {self.at} ({kind}) is past the end of the recorded log"
            got = str(names[kinds[self.at]])
            assert got == kind, f"draw {self.at}: the reference called {got}, the builder {kind}"
            v = vals[starts[self.at]:starts[self.at + 1]]
            self.at += 1
            return v

        def random(self):
            return float(self._next("random")[0])

        def randint(self, lo, hi):
            v = int(self._next("randint")[0])
            assert lo <= v <= hi
            return v

        def py_uniform(self, lo, hi):
            return float(self._next("py_uniform")[0])

        def choice(self, seq):
            v = int(self._next("choice")[0])
            assert v in seq
            return v

        def sample(self, population, k):
            v = [int(q) for q in self._next("sample")]
            assert len(v) == k and sorted(v) == sorted(population)
            return v

        def np_rand(self, *shape):
            v = self._next("np_rand")
            return v.reshape(shape) if shape else float(v[0])

        def randn(self, shape, device):
            f = fields.standard_normal(shape).astype(np.float32)
            self.given.append(f)
            return torch.from_numpy(f).to(device)

        def poisson(self, rates):
            f = fields.poisson(rates.detach().cpu().numpy().astype(np.float64)).astype(np.float32)
            self.given.append(f)
            return torch.from_numpy(f).to(rates.device)

        def done(self):
            return self.at == len(kinds)

    return Scripted()


def chain_draws(i, fields=None):
    fx = fixture()
    return scripted_draws(fx[f"chain{i}_log_kind"], fx[f"chain{i}_log_val"], fx[f"chain{i}_log_len"], fx["log_kinds"], fields)


def events_of(stages):
    """a program's stages in the fixture's event rows (kind, h, w, h_out, w_out, extra); a strided convolution is recorded
    before its slice, so its row holds the input size twice and the NEXT row's input checks the slice"""
    rows = []
    for st in stages:
        p = st.params
        if st.kind == "conv":
            rows.append(("conv", st.h, st.w, st.h, st.w, np.asarray(p["kernel"]).shape[0]))
        elif st.kind == "resize":
            rows.append(("resize", st.h, st.w, st.oh, st.ow, p["interp"]))
        elif st.kind == "noise":
            rows.append(("speckle" if p["op"].startswith("SPECKLE") else "gaussian", st.h, st.w, st.oh, st.ow, 0))
        else:
            rows.append((st.kind, st.h, st.w, st.oh, st.ow, 0))
    return [(EVENT_KINDS.index(k),) + tuple(int(v) for v in rest) for k, *rest in rows]


# ------------------------------------------------------------------ case lists (GPU tests and the poison audit) ----
CONV_SIDES = [1, 2, 5, 9, 17, 33, 70]           # 9 = a tile's 8 rows + 1, 33 = its 32 columns + 1
CONV_KS = [3, 5, 7, 9]
RESIZE_RATIOS = [1 / 2, 1 / 3, 1 / 4, 0.53, 1 / 1.17, 1.0, 1.37, 2.0]


def asymmetric_kernel(rng, k):
    """positive, sum 1, heavier toward one corner: a missing flip moves the result by far more than any bound"""
    ramp = np.arange(1, k + 1, dtype=np.float64)
    kern = rng.random((k, k)) + 0.2 * np.outer(ramp, ramp ** 2)
    return kern / kern.sum()


def conv_cases(k, seed=0):
    """(images (C, h, w) float32, stages) for every pair of sides, channels 1 / 3, strides 1 / 2 / 4 and the clip by turns"""
    from ssl_amd.blindsr import Stage
    rng = np.random.default_rng(100 + k + seed)
    images, stages = [], []
    n = 0
    for h in CONV_SIDES:
        for w in CONV_SIDES:
            C, s = (1, 3)[n % 2], (1, 2, 4)[n % 3]
            images.append((rng.random((C, h, w), dtype=np.float32) * 1.4 - 0.2).astype(np.float32))
            stages.append(Stage("conv", h, w, -(-h // s), -(-w // s),
                                dict(kernel=asymmetric_kernel(rng, k), stride=s, clip=bool(n % 5 < 2))))
            n += 1
    return images, stages


def resize_cases(interp, seed=0):
    from ssl_amd.blindsr import Stage
    rng = np.random.default_rng(200 + interp + seed)
    shapes = []
    for r in RESIZE_RATIOS:
        for h, w in ((24, 36), (35, 41)):
            shapes.append((h, w, max(1, int(r * h)), max(1, int(r * w))))
    shapes += [(17, 23, 1, 1), (1, 1, 5, 7), (1, 1, 1, 1), (9, 40, 1, 13), (1, 30, 4, 11)]      # single pixels
    shapes += [(30, 44, 15, 31), (30, 44, 41, 22), (33, 65, 9, 90), (40, 20, 13, 27)]           # unequal / mixed ratios
    shapes += [(64, 96, 8, 12), (70, 66, 69, 65)]                                               # 8 x 8 boxes; ratio near 1
    images, stages = [], []
    for n, (h, w, oh, ow) in enumerate(shapes):
        C = (3, 1)[n % 2]
        images.append((rng.random((C, h, w), dtype=np.float32) * 1.4 - 0.2).astype(np.float32))
        stages.append(Stage("resize", h, w, oh, ow, dict(interp=interp, clip=bool(n % 3 == 0))))
    return images, stages


NOISE_MODES = [("GAUSS_COLOR", 3), ("GAUSS_COLOR", 1), ("GAUSS_GRAY", 3), ("GAUSS_GRAY", 1), ("GAUSS_CORR", 3),
               ("SPECKLE_COLOR", 3), ("SPECKLE_GRAY", 3), ("SPECKLE_CORR", 3), ("POISSON_RATES", 3), ("POISSON_RATES", 1),
               ("POISSON_COLOR", 3), ("POISSON_RATES_GRAY", 3), ("POISSON_GRAY", 3)]


def noise_cases(seed=0, nan=True):
    """(images, stages, fields) of every mode on 37 x 29 (two tiles of 1,024 pixels, the second partial); the first row
    holds values exactly at (k + 1/2) / 255 and one pixel is NaN"""
    from ssl_amd.blindsr import Stage, correlated_factor
    rng = np.random.default_rng(300 + seed)
    h, w = 37, 29
    images, stages, fields = [], [], []
    for op, C in NOISE_MODES:
        x = (rng.random((C, h, w), dtype=np.float32) * 1.3 - 0.15).astype(np.float32)
        x[:, 0, :] = ((np.arange(w) * 9 % 255 + 0.5) / 255.0).astype(np.float32)[None, :]
        if nan:
            x[0, 5, 7] = np.nan
        poisson = op.startswith("POISSON")
        planes = 0 if op.startswith("POISSON_RATES") else (1 if op.endswith("GRAY") else C)
        if poisson:
            f = rng.poisson(40.0, (planes, h, w)).astype(np.float32) if planes else None
            scale = 10 ** (2 * rng.random() + 2.0)
        else:
            f = rng.standard_normal((planes, h, w)).astype(np.float32)
            scale = 1.0 if op.endswith("CORR") else float(rng.integers(2, 26)) / 255.0
        matrix = correlated_factor(rng.random(3), np.linalg.qr(rng.random((3, 3)))[0], 25 / 255.) if op.endswith("CORR") else None
        images.append(x), fields.append(f)
        stages.append(Stage("noise", h, w, h, w, dict(op=op, scale=scale, matrix=matrix, clip=not op.startswith("POISSON_RATES"),
                                                       lead_clip=op.startswith("SPECKLE"))))
    return images, stages, fields


def noise_reference(x, st, f):
    """the restatement's float32 result of one noise case"""
    p, op = st.params, st.params["op"]
    if op.startswith("POISSON_RATES"):
        return R.poisson_rates(x, p["scale"], op.endswith("GRAY"))
    if op.startswith("POISSON"):
        return R.poisson(x, f, p["scale"], op.endswith("GRAY"), p["clip"])
    family, mode = op.split("_")
    return R.gaussian(x, f, p["scale"], mode.lower(), p["matrix"], family == "SPECKLE", p["clip"])


# ------------------------------------------------------------------ the live oracles and their shares ----
def oracle_shares():
    """name -> the largest |oracle's float32 result - restatement| / derived bound over the oracle's cases (each must be
    <= 1), for the oracles that evaluate in float32: scipy's convolve on a float32 image, torch's bilinear and bicubic
    interpolate and avg_pool2d on float32 tensors."""
    import torch
    import torch.nn.functional as F
    from scipy import ndimage
    rng = np.random.default_rng(7)
    shares = {}
    worst = 0.0
    for k in CONV_KS:
        for h, w in ((1, 1), (2, 5), (17, 33), (40, 23)):
            x = rng.random((3, h, w), dtype=np.float32)
            kern = asymmetric_kernel(rng, k)
            want, bound = R.conv(x, kern)
            got = ndimage.convolve(x.transpose(1, 2, 0), kern[:, :, None], mode='mirror').transpose(2, 0, 1)
            worst = max(worst, float((np.abs(got.astype(np.float64) - want) / bound).max()))
    shares["scipy.ndimage.convolve(mode='mirror') on float32"] = worst
    for interp, mode in ((R.LINEAR, "bilinear"), (R.CUBIC, "bicubic")):
        worst = 0.0
        for h, w, oh, ow in ((24, 36, 12, 18), (24, 36, 8, 12), (35, 41, 18, 21), (24, 36, 32, 49), (17, 23, 1, 1), (30, 44, 41, 22)):
            x = rng.random((3, h, w), dtype=np.float32)
            want, bound = R.resize(x, oh, ow, interp)
            # torch forms scale, coordinate and weights in float: three roundings of a value below the side each
            slack = R.coordinate_slack(x, oh, ow, interp, 4 * R.U * (h + 1), 4 * R.U * (w + 1))
            got = F.interpolate(torch.from_numpy(x)[None], size=(oh, ow), mode=mode, align_corners=False)[0].numpy()
            weights = 100 * R.U * np.abs(x).max() if interp == R.CUBIC else 0.0     # torch's cubic weights: another form
            worst = max(worst, float((np.abs(got.astype(np.float64) - want) / (bound + slack + weights)).max()))
        shares[f"torch interpolate {mode} on float32"] = worst
    worst = 0.0
    for h, w, q in ((24, 36, 2), (24, 36, 3), (24, 36, 4), (64, 96, 8)):
        x = rng.random((3, h, w), dtype=np.float32)
        want, bound = R.resize(x, h // q, w // q, R.AREA)
        got = F.avg_pool2d(torch.from_numpy(x)[None], q)[0].numpy()
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / bound).max()))
    shares["torch avg_pool2d on float32"] = worst
    return shares


# ------------------------------------------------------------------ the chain cases ----
def seeded_draws(seed):
    """A BlindSRDraws whose decisions come from generators of its own (python's Random and numpy's RandomState, seeded)
    and whose noise fields come from a numpy Generator; every field and every Poisson rate handed over is kept."""
    import random

    import torch
    from ssl_amd.blindsr import BlindSRDraws

    class Seeded(BlindSRDraws):
        def __init__(self):
            self.py, self.np, self.fields = random.Random(seed), np.random.RandomState(seed), np.random.default_rng(seed)
            self.given, self.rates = [], []

        def random(self):
            return self.py.random()

        def randint(self, lo, hi):
            return self.py.randint(lo, hi)

        def py_uniform(self, lo, hi):
            return self.py.uniform(lo, hi)

        def choice(self, seq):
            return self.py.choice(seq)

        def sample(self, population, k):
            return self.py.sample(population, k)

        def np_rand(self, *shape):
            return self.np.rand(*shape)

        def randn(self, shape, device):
            f = self.fields.standard_normal(shape).astype(np.float32)
            self.given.append(f)
            return torch.from_numpy(f).to(device)

        def poisson(self, rates):
            r = rates.detach().cpu().numpy()
            f = self.fields.poisson(r.astype(np.float64)).astype(np.float32)
            self.rates.append(r), self.given.append(f)
            return torch.from_numpy(f).to(rates.device)

    return Seeded()


# (variant, seed, the (h, w) of the three images): chosen so that the programs hold every stage kind but the MATLAB
# pre-scale (prep.imresize, which has tests of its own); test_gpu_blindsr checks that they do
CHAIN_CASES = [("plus", 21, ((80, 72), (76, 84), (69, 71))), ("bsrgan", 25, ((80, 72), (72, 88), (67, 70)))]
CHAIN_PATCH, CHAIN_SF = 16, 4


def chain_images(shapes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w]
        base = 0.5 + 0.35 * np.sin(yy / 5.0 + seed)[..., None] * np.cos(xx[..., None] / 7.0 + np.arange(3))
        out.append(np.clip(base + 0.1 * rng.standard_normal((h, w, 3)), 0, 1).astype(np.float32))
    return out
