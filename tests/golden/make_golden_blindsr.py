"""Generate f35_blindsr.npz FROM THE REFERENCE ITSELF: GAN-Based-SR/train_BSGRAN/utils/utils_blindsr.py run on the CPU.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_blindsr.py <reference root>

The reference imports OpenCV and torchvision, which are not installed where this runs, and `scipy.interpolate.interp2d`,
which no longer evaluates.  THIS SCRIPT ONLY (never a test) places stand-ins in `sys.modules` before it loads the
reference by file path:
  cv2          resize records its arguments and delegates to tests/blindsr_reference.py's restatement; cvtColor,
               imencode and imdecode pass the image through (the chain fixture holds decisions and SIZES, which no pixel
               value influences); GaussianBlur is absent (use_sharp is not exercised)
  torchvision  an empty module (utils_image.py imports make_grid and never calls it here)
  interp2d     the linear case on a regular grid, evaluated with numpy (what the removed function computed)
and wraps the reference module's `random`, `np.random`, `ndimage.filters.convolve` and its own stage functions so that
every decision, every intercepted field and every stage's sizes are recorded.  Only DATA is stored.

The fixture:
  kernels      every kernel the chains hand to ndimage.filters.convolve (add_blur's fspecial / anisotropic_Gaussian ones
               and downsample2's shifted one), padded to 9 x 9, with their sizes: `chain<i>_kernels`, `chain<i>_ksizes`
  noise        for add_Gaussian_noise, add_speckle_noise and add_Poisson_noise in each of their modes on a 24 x 20 x 3
               image: `noise_<tag>_in`, `_field` (the intercepted np.random.normal / multivariate_normal / poisson output),
               `_out`, `_log` (the decisions) and for the correlated modes `_cov`, `_D`, `_U`
  chains       twenty seeds of degradation_bsrgan and degradation_bsrgan_plus on 300 x 292 x 3 (and two sizes more):
               `chain<i>_log_kind` / `_log_val` / `_log_len` (every decision in call order: which generator method and
               what it returned), `chain<i>_events` (one row per stage: kind, h, w, h_out, w_out, extra), `chain<i>_meta`
               (variant, seed, H, W, sf, lq_patchsize, lq h, lq w, hq origin row, hq origin column)
The input's first two channels hold the row and the column of every pixel (over 1024), so the origin of the returned HQ
patch is read from its first pixel.
"""
import importlib.util
import os
import random as _random
import sys
import types
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import blindsr_reference as R  # noqa: E402

OUT = os.path.join(HERE, "f35_blindsr.npz")
LOG_KINDS = ["random", "randint", "py_uniform", "choice", "sample", "np_rand"]
EVENT_KINDS = ["conv", "resize", "gaussian", "speckle", "poisson", "jpeg", "imresize"]


class Recorder:
    def __init__(self):
        self.reset()

    def reset(self):
        self.log, self.events, self.kernels, self.fields, self.covs = [], [], [], [], []

    def note(self, kind, value):
        self.log.append((LOG_KINDS.index(kind), np.atleast_1d(np.asarray(value, dtype=np.float64)).reshape(-1)))
        return value


REC = Recorder()


class RandomProxy:
    """python's `random` as the reference module sees it"""

    def random(self):
        return REC.note("random", _random.random())

    def randint(self, a, b):
        return REC.note("randint", _random.randint(a, b))

    def uniform(self, a, b):
        return REC.note("py_uniform", _random.uniform(a, b))

    def choice(self, seq):
        return REC.note("choice", _random.choice(seq))

    def sample(self, population, k):
        return REC.note("sample", _random.sample(population, k))


class NpRandomProxy:
    def rand(self, *shape):
        return REC.note("np_rand", np.random.rand(*shape))

    def normal(self, *a, **k):
        REC.fields.append(np.random.normal(*a, **k))
        return REC.fields[-1]

    def multivariate_normal(self, mean, cov, size):
        REC.covs.append(np.array(cov))
        REC.fields.append(np.random.multivariate_normal(mean, cov, size))
        return REC.fields[-1]

    def poisson(self, lam):
        REC.fields.append(np.random.poisson(lam))
        return REC.fields[-1]


class NpProxy:
    random = NpRandomProxy()

    def __getattr__(self, name):
        return getattr(np, name)


class LinearInterp2d:
    """interp2d(x, y, z) (kind='linear') on a regular grid: z is (len(y), len(x))"""

    def __init__(self, x, y, z):
        self.x, self.y, self.z = np.asarray(x, float), np.asarray(y, float), np.asarray(z, float)

    def __call__(self, x1, y1):
        def split(grid, at):
            i = np.clip(np.searchsorted(grid, at, side="right") - 1, 0, max(len(grid) - 2, 0))
            j = np.minimum(i + 1, len(grid) - 1)
            span = np.where(j > i, grid[j] - grid[i], 1.0)
            return i, j, (at - grid[i]) / span
        ix, jx, fx = split(self.x, np.sort(np.asarray(x1, float)))
        iy, jy, fy = split(self.y, np.sort(np.asarray(y1, float)))
        z = self.z
        top = z[iy][:, ix] * (1 - fx) + z[iy][:, jx] * fx
        bot = z[jy][:, ix] * (1 - fx) + z[jy][:, jx] * fx
        return top * (1 - fy[:, None]) + bot * fy[:, None]


def install_stand_ins():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2RGB, cv2.IMWRITE_JPEG_QUALITY = 4, 4, 1

    def resize(img, dsize, interpolation=1):
        h, w = img.shape[:2]
        REC.events.append((EVENT_KINDS.index("resize"), h, w, dsize[1], dsize[0], interpolation))
        out, _ = R.resize(np.asarray(img, np.float32).transpose(2, 0, 1), dsize[1], dsize[0], interpolation)
        return out.transpose(1, 2, 0).astype(np.float32)

    cv2.resize = resize
    cv2.cvtColor = lambda img, code: img
    cv2.imencode = lambda ext, img, params: (True, img)
    cv2.imdecode = lambda buf, flag: buf
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")
    tv.utils = types.ModuleType("torchvision.utils")
    tv.utils.make_grid = None
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tv.utils
    import scipy.interpolate
    scipy.interpolate.interp2d = LinearInterp2d


def load_reference(root):
    base = os.path.join(root, "GAN-Based-SR", "train_BSGRAN", "utils")
    for name in ("train_BSGRAN", "train_BSGRAN.utils"):
        sys.modules[name] = types.ModuleType(name)

    def load(name, file):
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, file))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    util = load("train_BSGRAN.utils.utils_image", "utils_image.py")
    sys.modules["train_BSGRAN.utils"].utils_image = util
    ref = load("train_BSGRAN.utils.utils_blindsr", "utils_blindsr.py")
    ref.random, ref.np = RandomProxy(), NpProxy()
    real_convolve = ref.ndimage.filters.convolve

    class Filters:
        @staticmethod
        def convolve(img, k, mode):
            assert mode == "mirror"
            h, w = img.shape[:2]
            REC.events.append((EVENT_KINDS.index("conv"), h, w, h, w, k.shape[0]))
            REC.kernels.append(np.array(k[:, :, 0]))
            return real_convolve(img, k, mode=mode)

    class Ndimage:
        filters = Filters

    ref.ndimage = Ndimage

    def staged(name, kind):
        real = getattr(ref, name)

        def wrapped(img, *a, **k):
            REC.events.append((EVENT_KINDS.index(kind), img.shape[0], img.shape[1], img.shape[0], img.shape[1], 0))
            return real(img, *a, **k)
        setattr(ref, name, wrapped)

    for name, kind in (("add_Gaussian_noise", "gaussian"), ("add_speckle_noise", "speckle"), ("add_Poisson_noise", "poisson"),
                       ("add_JPEG_noise", "jpeg")):
        staged(name, kind)
    real_imresize = util.imresize_np

    def imresize_np(img, scale, antialiasing=True):
        out = real_imresize(img, scale, antialiasing)
        REC.events.append((EVENT_KINDS.index("imresize"), img.shape[0], img.shape[1], out.shape[0], out.shape[1], 0))
        return out
    util.imresize_np = imresize_np
    # add_JPEG_noise's own single2uint / uint2single round trip keeps the image as it is for the purposes of this fixture
    return ref


def position_image(h, w, rng):
    img = np.zeros((h, w, 3), np.float32)
    img[:, :, 0] = (np.arange(h, dtype=np.float32) / np.float32(1024))[:, None]
    img[:, :, 1] = (np.arange(w, dtype=np.float32) / np.float32(1024))[None, :]
    img[:, :, 2] = rng.random((h, w), dtype=np.float32)
    return img


def seed_all(seed):
    _random.seed(seed)
    np.random.seed(seed)


def pack_log(log):
    return (np.array([k for k, _ in log], np.int8), np.concatenate([v for _, v in log]),
            np.array([len(v) for _, v in log], np.int16))


def main(root):
    install_stand_ins()
    ref = load_reference(root)
    out = {"log_kinds": np.array(LOG_KINDS), "event_kinds": np.array(EVENT_KINDS)}
    rng = np.random.default_rng(35)

    # ---- the three noise functions, every mode ----
    base = (rng.random((24, 20, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
    wanted = {"gaussian": ("color", "gray", "corr"), "speckle": ("color", "gray", "corr"), "poisson": ("color", "gray")}
    calls = {"gaussian": lambda x: ref.add_Gaussian_noise(x, 2, 25), "speckle": lambda x: ref.add_speckle_noise(x),
             "poisson": lambda x: ref.add_Poisson_noise(x)}
    for fn, modes in wanted.items():
        seen = set()
        for seed in range(200):
            REC.reset()
            seed_all(1000 + seed)
            x = base.copy()
            y = calls[fn](x)
            field = REC.fields[-1]
            if fn == "poisson":
                mode = "color" if field.ndim == 3 else "gray"
            else:
                mode = "corr" if REC.covs else ("gray" if field.shape[-1] == 1 else "color")
            if mode in seen:
                continue
            seen.add(mode)
            tag = f"noise_{fn}_{mode}"
            kinds, vals, lens = pack_log(REC.log)
            out[tag + "_in"], out[tag + "_out"] = base, np.asarray(y, np.float32)
            out[tag + "_field"] = np.asarray(field, np.float32 if fn != "poisson" else np.float64)
            out[tag + "_log_kind"], out[tag + "_log_val"], out[tag + "_log_len"] = kinds, vals, lens
            if mode == "corr":
                out[tag + "_cov"] = REC.covs[-1]
            if seen == set(modes):
                break
        assert seen == set(modes), (fn, seen)

    # ---- the chains: decisions, stage order and sizes ----
    cases = [("bsrgan", s, 300, 292, 4, 72) for s in range(20)] + [("plus", s, 300, 292, 4, 64) for s in range(20)]
    cases += [("bsrgan", 100, 301, 295, 4, 72), ("plus", 101, 290, 310, 4, 64), ("bsrgan", 102, 150, 158, 2, 72)]
    for i, (variant, seed, H, W, sf, patch) in enumerate(cases):
        REC.reset()
        seed_all(seed)
        img = position_image(H, W, rng)
        if variant == "bsrgan":
            lq, hq = ref.degradation_bsrgan(img, sf=sf, lq_patchsize=patch)
        else:
            lq, hq = ref.degradation_bsrgan_plus(img, sf=sf, shuffle_prob=0.5, use_sharp=False, lq_patchsize=patch)
        kinds, vals, lens = pack_log(REC.log)
        origin = np.rint(hq[0, 0, :2].astype(np.float64) * 1024).astype(np.int64)
        out[f"chain{i}_log_kind"], out[f"chain{i}_log_val"], out[f"chain{i}_log_len"] = kinds, vals, lens
        out[f"chain{i}_events"] = np.array(REC.events, np.int32).reshape(-1, 6)
        out[f"chain{i}_meta"] = np.array([variant == "plus", seed, H, W, sf, patch, lq.shape[0], lq.shape[1], origin[0],
                                          origin[1], hq.shape[0], hq.shape[1]], np.int64)
        ks = np.zeros((len(REC.kernels), 9, 9))
        for j, k in enumerate(REC.kernels):
            ks[j, :k.shape[0], :k.shape[1]] = k
        out[f"chain{i}_kernels"], out[f"chain{i}_ksizes"] = ks, np.array([k.shape[0] for k in REC.kernels], np.int32)
    out["n_chains"] = np.array(len(cases))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(cases)} chains")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
