"""Generate f34_ema.npz FROM THE REFERENCE ITSELF: its LitEma on a small seeded model.

Needs the reference tree (which never travels with this repository) and runs on the CPU:

    python tests/golden/make_golden_ema.py <reference root>

It imports Diffusion-Based-SR/ldm/modules/ema.py by path (the file needs torch only) and runs LitEma on
ema_reference.fixture_model(): two convolutions, the first one's bias frozen.  Before each update the weights move by
ema_reference.fixture_perturbations().

Stored, from the reference on the CPU, numbers and names only:
  init_{name}            the model's initial parameters
  pert_{name}            (12, *shape) the perturbation added before update t
  shadow_{sname}         (12, *shape) LitEma's buffer after update t, decay 0.5 with the warm-up (which crosses 0.5 at
                         the 8th update)
  num_updates, decay     (12,) int32 and () fp32: the two scalar buffers after each update / as registered
  keys                   the state_dict's keys, in order
  fixed_shadow_{sname}   (3, *shape) the same with use_num_upates=False and decay 0.9999 (no warm-up), from the same start
  fixed_num_updates      () int32: -1
Only DATA is stored; no reference source text.
"""
import importlib.util
import os
import sys
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f34_ema.npz")
sys.path.insert(0, os.path.dirname(HERE))
import ema_reference as R  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "Diffusion-Based-SR", "ldm", "modules", "ema.py")
    spec = importlib.util.spec_from_file_location("reference_ema", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(LitEma, steps, **kwargs):
    net = R.fixture_model()
    ema = LitEma(net, **kwargs)
    pert = R.fixture_perturbations(R.FIXTURE_STEPS)
    shadows = {s: [] for s in ema.m_name2s_name.values()}
    counts = []
    for t in range(steps):
        R.perturb(net, pert, t)
        ema(net)
        for s in shadows:
            shadows[s].append(dict(ema.named_buffers())[s].clone().numpy())
        counts.append(int(ema.num_updates))
    return ema, {s: np.stack(v) for s, v in shadows.items()}, np.asarray(counts, dtype=np.int32)


def main(root):
    LitEma = load_reference(root).LitEma
    out = {"init_" + n: p.detach().numpy() for n, p in R.fixture_model().named_parameters()}
    out.update({"pert_" + n: v.numpy() for n, v in R.fixture_perturbations(R.FIXTURE_STEPS).items()})
    ema, shadows, counts = run(LitEma, R.FIXTURE_STEPS, decay=R.FIXTURE_DECAY)
    out.update({"shadow_" + s: v for s, v in shadows.items()})
    out["num_updates"], out["decay"] = counts, ema.decay.numpy()
    out["keys"] = np.asarray(list(ema.state_dict().keys()))
    ema, shadows, counts = run(LitEma, R.FIXED_STEPS, decay=R.FIXED_DECAY, use_num_upates=False)
    out.update({"fixed_shadow_" + s: v for s, v in shadows.items()})
    out["fixed_num_updates"] = counts[-1]
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
