"""Generate f36_diffusion.npz FROM THE REFERENCE ITSELF: its schedule, per-sample combinations, Gaussian tile weights,
aggregation sampling and image splitter, on the CPU.

Needs the reference tree (which never travels with this repository):

    python tests/golden/make_golden_diffusion.py <reference root>

ldm/modules/diffusionmodules/util.py (make_beta_schedule) and ldm/models/respace.py (space_timesteps) import directly.
ldm/models/diffusion/ddpm.py and scripts/util_image.py import packages that are not installed where the fixture is made
(pytorch_lightning, torchvision, cv2, skimage, omegaconf ...); none of them is used by the methods recorded here, so
while those two files load, a finder in sys.meta_path answers the imports of those packages (STAND_INS, and any further
package whose import fails) with an empty stand-in module whose attributes are inert classes.  The methods are then
called UNBOUND on a small object of this file's own that has the attributes they read (`parameterization`,
`v_posterior`, `register_buffer`, the buffers, `configs`, the reference's own q_posterior and predict_start_* bound to
it, and for the canvas an `apply_model` that is tests/diffusion_cases.py's fixed elementwise function).

Stored, numbers only (no reference source text):
  sched_{name}_{buffer}         register_schedule's buffers for tests/diffusion_cases.py's SCHEDULES
  respaced_{steps}_{buffer}     the buffers after test.py:277-292's respacing of "linear_eps" (the loop over the float32
                                alphas_cumprod is restated here around the reference's space_timesteps and
                                register_schedule), and respaced_{steps}_steps, the kept steps
  combine_{q_sample, get_v, predict_start_from_noise, predict_start_from_z_and_v, q_posterior}
                                the methods' outputs on diffusion_cases.sample_inputs(3, 37, 0) under "linear_eps"
  weights_{8, 64}               _gaussian_weights(n, n, 1)[0, 0]: float64
  canvas_*_tiles                the tiles' (oy, ox) as p_mean_variance_canvas cut them, read off a canvas of indices
  canvas_*_stitched             its stitched model output (parameterization x0 returns it as x_recon)
  canvas_*_mean, _x0            its model_mean and x_recon under "linear_eps" (eps), clip_denoised, t = 17 (the large
                                case without _x0)
  split_*_windows, _out         ImageSpliterTh's index_infos in iteration order and gather()'s result
"""
import importlib
import importlib.abc
import importlib.machinery
import os
import sys
import types
sys.dont_write_bytecode = True

import numpy as np
import scipy.fft  # noqa: F401  (loaded before the stand-in finder exists)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f36_diffusion.npz")
sys.path.insert(0, os.path.dirname(HERE))
import diffusion_cases as C  # noqa: E402


class _Inert:
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        return self


class _StandIn(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (_Inert,), {})


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Answers the imports of the named top-level packages (and of everything below them) with stand-ins."""

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


# not installed where the fixture is made, or (the fork's own basicsr) a tree of further such imports; a package that is
# missing beside these is added when its import fails
STAND_INS = ("pytorch_lightning", "torchvision", "cv2", "skimage", "omegaconf", "basicsr")


def load_reference(root):
    fork = os.path.join(root, "Diffusion-Based-SR")
    sys.path.insert(0, fork)
    util = importlib.import_module("ldm.modules.diffusionmodules.util")
    respace = importlib.import_module("ldm.models.respace")
    finder = _Finder(STAND_INS)
    sys.meta_path.insert(0, finder)
    try:
        while True:
            try:
                ddpm = importlib.import_module("ldm.models.diffusion.ddpm")
                image = importlib.import_module("scripts.util_image")
                break
            except ModuleNotFoundError as err:
                missing = err.name.split(".")[0]
                if missing in finder.names or missing in ("ldm", "scripts"):
                    raise
                finder.names.add(missing)
    finally:
        sys.meta_path.remove(finder)
    print("stand-in modules:", ", ".join(sorted(finder.names)))
    return util, respace, ddpm, image


class Host:
    """What the recorded methods read of `self`."""

    def __init__(self, parameterization="eps", v_posterior=0.):
        self.parameterization, self.v_posterior = parameterization, v_posterior
        self.configs = types.SimpleNamespace(model=types.SimpleNamespace(params=types.SimpleNamespace(channels=C.CANVAS_C)))
        self.seen = []

    def register_buffer(self, name, tensor, persistent=True):
        setattr(self, name, tensor)

    def structcond_stage_model(self, cond, t):
        return cond

    def apply_model(self, x, t, c, struct_cond, return_ids=False):
        self.seen.append(x)
        return C.stand_in_network(x, struct_cond)


def registered(ddpm, kwargs):
    kwargs = dict(kwargs)
    host = Host(kwargs.pop("parameterization"), kwargs.pop("v_posterior"))
    ddpm.DDPM.register_schedule(host, **kwargs)
    for method in ("q_posterior", "predict_start_from_noise", "predict_start_from_z_and_v"):   # the reference's own
        setattr(host, method, types.MethodType(getattr(ddpm.DDPM, method), host))
    return host


def buffers(host, prefix):
    return {f"{prefix}_{b}": getattr(host, b).numpy() for b in C.BUFFERS}


def canvas_class(ddpm):
    for value in vars(ddpm).values():
        if isinstance(value, type) and "p_mean_variance_canvas" in vars(value) and "_gaussian_weights" in vars(value):
            return value
    raise RuntimeError("no class with p_mean_variance_canvas")


def main(root):
    util, respace, ddpm, image = load_reference(root)
    out = {}
    for name, kwargs in C.SCHEDULES.items():
        out.update(buffers(registered(ddpm, kwargs), "sched_" + name))
    base = registered(ddpm, C.SCHEDULES["linear_eps"])
    for steps in C.RESPACED:
        keep = respace.space_timesteps(1000, [steps])
        last, betas, kept = 1.0, [], []
        for i, a in enumerate(base.alphas_cumprod):        # 0-dim float32 tensors, as in test.py
            if i in keep:
                betas.append((1 - a / last).data.cpu().numpy())
                last = a
                kept.append(i)
        host = Host()
        ddpm.DDPM.register_schedule(host, given_betas=np.array(betas), timesteps=len(betas))
        out.update(buffers(host, f"respaced_{steps}"))
        out[f"respaced_{steps}_steps"] = np.asarray(kept, dtype=np.int64)
    # the per-sample combinations
    a, b, _ = (v.view(3, 1, 1, 37) for v in C.sample_inputs(3, 37, 0))
    t = C.timesteps(3, 1000)
    D = ddpm.DDPM
    out["combine_q_sample"] = D.q_sample(base, a, t, b).numpy()
    out["combine_get_v"] = D.get_v(base, a, b, t).numpy()
    out["combine_predict_start_from_noise"] = D.predict_start_from_noise(base, a, t, b).numpy()
    out["combine_predict_start_from_z_and_v"] = D.predict_start_from_z_and_v(base, a, b, t).numpy()
    out["combine_q_posterior"] = D.q_posterior(base, a, b, t)[0].numpy()
    # the canvas
    K = canvas_class(ddpm)
    for n in (8, 64):
        w = K._gaussian_weights(base, n, n, 1)
        assert w.dtype == torch.float64 and w.shape == (1, C.CANVAS_C, n, n)
        out[f"weights_{n}"] = w[0, 0].numpy()
    for case in C.CANVAS:
        ts, overlap, h, w = case
        for B in C.CANVAS_FIXTURE_B.get(case, C.CANVAS_BATCHES):
            name = C.canvas_name(case, B)
            weights = K._gaussian_weights(base, ts, ts, B)
            cond = torch.zeros(64, 1)
            tt = torch.full((B,), 17, dtype=torch.int64)
            # the tiles, read off a canvas whose elements are their own indices
            index = (torch.arange(h)[:, None] * w + torch.arange(w)[None, :]).float().expand(B, C.CANVAS_C, h, w).contiguous()
            host = registered(ddpm, dict(C.SCHEDULES["linear_eps"], parameterization="x0"))
            K.p_mean_variance_canvas(host, index, cond, index, tt, clip_denoised=False, tile_size=ts,
                                     tile_overlap=overlap, batch_size=4, tile_weights=weights)
            corners = torch.cat([s[::B, 0, 0, 0] for s in host.seen]).long()
            out[name + "_tiles"] = torch.stack([corners // w, corners % w], 1).numpy()
            x, sc = C.canvas_inputs(case, B)
            host = registered(ddpm, dict(C.SCHEDULES["linear_eps"], parameterization="x0"))
            got = K.p_mean_variance_canvas(host, x, cond, sc, tt, clip_denoised=False, return_x0=True, tile_size=ts,
                                           tile_overlap=overlap, batch_size=4, tile_weights=weights)
            out[name + "_stitched"] = got[3].numpy()
            got = K.p_mean_variance_canvas(base, x, cond, sc, tt, clip_denoised=True, return_x0=True, tile_size=ts,
                                           tile_overlap=overlap, batch_size=4, tile_weights=weights)
            out[name + "_mean"] = got[0].numpy()
            if case not in C.CANVAS_FIXTURE_B:             # (the large case's x_recon is left out: the file's size)
                out[name + "_x0"] = got[3].numpy()
    # the splitter
    for case in C.SPLITTER:
        h, w, patch, stride, sf = case
        im = C.splitter_input(case)
        sp = image.ImageSpliterTh(im, patch, stride, sf=sf)
        windows = []
        for k, (pch, info) in enumerate(sp):
            windows.append(info)
            sp.update(C.splitter_patch_result(pch, sf, k), info)
        out[C.splitter_name(case) + "_windows"] = np.asarray(windows, dtype=np.int64)
        out[C.splitter_name(case) + "_out"] = sp.gather().numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
