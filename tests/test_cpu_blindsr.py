"""The ragged degradation chain without a GPU: the restatement (tests/blindsr_reference.py) against live oracles, the
kernel synthesis against SciPy, and the program builder and the restatement against what the reference itself did
(tests/golden/f35_blindsr.npz, recorded by tests/golden/make_golden_blindsr.py from utils_blindsr.py).

OpenCV is not available to these tests, so `cv2.resize` itself is not an oracle: LINEAR and CUBIC are held to torch's
interpolate (the formulas coincide), AREA to the exact integral of the piecewise-constant image over each cell and to
avg_pool2d.  Equality with cv2.resize is supposed, not verified."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blindsr_cases as cases
import blindsr_reference as R
from ssl_amd import blindsr

EVENT = {name: i for i, name in enumerate(cases.EVENT_KINDS)}


# ------------------------------------------------------------------ live oracles ----
@pytest.mark.parametrize("k", cases.CONV_KS)
def test_conv_restatement_is_scipys_mirror_convolve(k):
    from scipy import ndimage
    rng = np.random.default_rng(k)
    for h, w in ((1, 1), (1, 7), (2, 2), (3, 2), (5, 17), (33, 9)):          # axes shorter than the radius included
        x = rng.random((3, h, w))
        kern = cases.asymmetric_kernel(rng, k)
        want = ndimage.convolve(x.transpose(1, 2, 0), kern[:, :, None], mode='mirror').transpose(2, 0, 1)
        for s in (1, 2, 4):
            got, _ = R.conv(x, kern, s)
            assert np.abs(got - want[:, ::s, ::s]).max() <= 1e-14
    # the flip matters for this kernel: the correlation is far from the convolution
    assert np.abs(R.conv(x, kern[::-1, ::-1])[0] - want).max() > 1e-3


def test_kernel_synthesis_is_scipys_density():
    import scipy.stats as ss
    rng = np.random.default_rng(1)
    for size in (3, 5, 7, 9, 15):
        theta, l1, l2 = rng.random() * np.pi, 0.05 + rng.random(), 0.05 + rng.random()
        v = np.array([np.cos(theta), np.sin(theta)])
        V = np.array([[v[0], v[1]], [v[1], -v[0]]])
        Sigma = V @ np.diag([l1, l2]) @ np.linalg.inv(V)
        center = size / 2.0 + 0.5
        want = np.array([[ss.multivariate_normal.pdf([x - center + 1, y - center + 1], mean=[0, 0], cov=Sigma)
                          for x in range(size)] for y in range(size)])
        want /= want.sum()
        assert np.allclose(blindsr.gm_blur_kernel([0, 0], Sigma, size), want, rtol=1e-10, atol=1e-300)
        assert np.allclose(blindsr.anisotropic_Gaussian(size, theta, l1, l2), want, rtol=1e-10, atol=1e-300)
    g = blindsr.fspecial('gaussian', 7, 1.3)
    assert abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g.T) and np.array_equal(g, g[::-1])
    assert blindsr.fspecial('gaussian', 9, 0.1)[0, 0] == 0          # below eps * max: set to zero, as MATLAB does


@pytest.mark.parametrize("sf", [2, 3, 4])
def test_shift_pixel_is_the_linear_spline_on_the_clamped_grid(sf):
    from scipy.interpolate import RectBivariateSpline
    rng = np.random.default_rng(sf)
    for h, w in ((3, 3), (5, 7), (9, 9), (21, 4)):
        k = rng.random((h, w))
        xv, yv = np.arange(0, w, 1.0), np.arange(0, h, 1.0)
        shift = (sf - 1) * 0.5
        want = RectBivariateSpline(yv, xv, k, kx=1, ky=1)(np.clip(yv + shift, 0, h - 1), np.clip(xv + shift, 0, w - 1))
        assert np.abs(blindsr.shift_pixel(k, sf) - want).max() <= 1e-15
        both = blindsr.shift_pixel(np.stack([k, 2 * k], -1), sf)
        assert np.abs(both[..., 0] - want).max() <= 1e-15 and np.abs(both[..., 1] - 2 * want).max() <= 2e-15


@pytest.mark.parametrize("interp,mode", [(R.LINEAR, "bilinear"), (R.CUBIC, "bicubic")])
def test_linear_and_cubic_restatements_are_torchs_interpolate(interp, mode):
    """torch in fp64 forms coordinate and weights in fp64; the restatement casts the coordinate to float and forms float
    weights, as OpenCV does: one rounding of a coordinate below the side (df = u (side + 1)) and, for CUBIC, the
    roundings of the four weight polynomials (intermediates up to 7.5: 64 u, 16 u, 16 u and their sum + 3 u)."""
    rng = np.random.default_rng(interp)
    for h, w in ((24, 36), (35, 41), (1, 1), (1, 9)):
        x = rng.random((3, h, w))
        for r in cases.RESIZE_RATIOS + [3.3]:
            oh, ow = max(1, int(r * h)), max(1, int(r * w))
            got, bound = R.resize(x, oh, ow, interp)
            want = F.interpolate(torch.from_numpy(x)[None], size=(oh, ow), mode=mode, align_corners=False)[0].numpy()
            slack = R.coordinate_slack(x, oh, ow, interp, R.U * (h + 1), R.U * (w + 1))
            weights = 2 * 200 * R.U * np.abs(x).max() if interp == R.CUBIC else 2 * R.U * np.abs(x).max()
            assert (np.abs(got - want) <= bound + slack + weights).all(), (h, w, oh, ow)


def _cell_integral(x, oh, ow):
    """the exact mean of the piecewise-constant image over every destination cell, fp64"""
    def axis(n, m):
        s = n / m
        wts = np.zeros((m, n))
        for d in range(m):
            lo, hi = d * s, min(d * s + s, n)
            for i in range(int(np.floor(lo)), min(int(np.ceil(hi)), n)):
                wts[d, i] = max(0.0, min(hi, i + 1) - max(lo, i)) / (hi - lo)
        return wts
    return np.einsum("chw,yh,xw->cyx", x, axis(x.shape[1], oh), axis(x.shape[2], ow))


def test_area_table_is_the_cell_integral_up_to_the_dropped_slivers():
    rng = np.random.default_rng(3)
    for h, w, oh, ow in ((24, 36, 12, 19), (35, 41, 18, 21), (24, 36, 20, 30), (30, 44, 29, 43), (70, 66, 13, 66),
                         (17, 23, 1, 1), (24, 36, 8, 13)):
        x = rng.random((3, h, w))
        got, bound = R.resize(x, oh, ow, R.AREA)
        assert (np.abs(got - _cell_integral(x, oh, ow)) <= 2 * 1e-3 * np.abs(x).max() + bound).all(), (h, w, oh, ow)


def test_area_at_integer_ratios_is_avg_pool():
    rng = np.random.default_rng(4)
    for h, w, qy, qx in ((24, 36, 2, 2), (24, 36, 3, 4), (64, 96, 8, 8), (5, 7, 1, 1), (12, 7, 4, 1)):
        x = rng.random((3, h, w))
        got, bound = R.resize(x, h // qy, w // qx, R.AREA)
        want = F.avg_pool2d(torch.from_numpy(x)[None], (qy, qx))[0].numpy()
        assert (np.abs(got - want) <= bound).all()


def test_area_upscaling_rule():
    """sx = floor(d s), f = (d + 1) - (sx + 1) / s taken as 0 when <= 0 and as its fractional part otherwise: doubling a
    row repeats every sample (f = 0 for even d, and (d + 1) - (sx + 1) 2 = 0 for odd d)"""
    x = np.arange(12.0).reshape(1, 3, 4)
    got, _ = R.resize(x, 6, 8, R.AREA)
    assert np.array_equal(got, np.repeat(np.repeat(x, 2, 1), 2, 2))
    # one axis reduced, the other enlarged: both axes take the area-mode linear rule
    iy, wy = R.axis_taps(30, 41, "area_linear")
    assert wy.dtype == np.float32 and iy.max() == 29 and (wy.sum(1) == 1).all()


def test_every_float32_oracle_meets_the_derived_bound():
    shares = cases.oracle_shares()
    assert len(shares) == 4
    for name, share in shares.items():
        print(f"{name}: {share:.3f} of the bound")
        assert 0 < share <= 1.0, name


# ------------------------------------------------------------------ the reference's own record ----
def test_program_builder_replays_the_reference_chains():
    """Every recorded chain: the builder, fed the reference's decisions in the reference's call order, takes the same
    stages in the same order with the same sizes (int() truncation, the a, b captured at downsample2, the sf = 2 branch,
    the strided slice), hands the convolution the same kernels, and crops where the reference cropped."""
    fx = cases.fixture()
    n = int(fx["n_chains"])
    assert n >= 40
    seen = set()
    for i in range(n):
        plus, seed, H, W, sf, patch, lq_h, lq_w, org_y, org_x, hq_h, hq_w = (int(v) for v in fx[f"chain{i}_meta"])
        d = cases.chain_draws(i)
        prog = blindsr.build_program("plus" if plus else "bsrgan", H, W, d, sf=sf, lq_patchsize=patch, shuffle_prob=0.5)
        assert d.done(), f"chain {i}: the builder took {d.at} draws"
        events = fx[f"chain{i}_events"]
        assert cases.events_of(prog.stages) == [tuple(int(v) for v in row) for row in events], i
        ks, sizes = fx[f"chain{i}_kernels"], fx[f"chain{i}_ksizes"]
        convs = [s for s in prog.stages if s.kind == "conv"]
        assert [np.asarray(s.params["kernel"]).shape[0] for s in convs] == list(sizes)
        for s, k, size in zip(convs, ks, sizes):
            assert np.allclose(s.params["kernel"], k[:size, :size], rtol=1e-9, atol=1e-18), i
        for a, b in zip(prog.stages, prog.stages[1:]):
            assert (a.oh, a.ow) == (b.h, b.w)
        assert (lq_h, lq_w) == (patch, patch) and (hq_h, hq_w) == (patch * sf, patch * sf)
        assert (int(prog.crop[0] * sf), int(prog.crop[1] * sf)) == (org_y, org_x), i
        assert prog.crop[0] + patch <= prog.stages[-1].oh and prog.crop[1] + patch <= prog.stages[-1].ow
        seen |= {(s.kind, s.params.get("stride", 0) > 1) for s in prog.stages}
        seen |= {("sf2", prog.sf == 2 and sf == 4)}
    # the fixture reaches every branch the builder has
    for branch in (("conv", False), ("conv", True), ("resize", False), ("noise", False), ("jpeg", False), ("poisson", False),
                   ("imresize", False), ("sf2", True)):
        assert branch in seen, branch


def _noise_case(tag):
    fx = cases.fixture()
    d = cases.scripted_draws(fx[tag + "_log_kind"], fx[tag + "_log_val"], fx[tag + "_log_len"], fx["log_kinds"])
    x = fx[tag + "_in"].transpose(2, 0, 1)
    field = fx[tag + "_field"]
    field = field[None] if field.ndim == 2 else field.transpose(2, 0, 1)
    return d, x, field.astype(np.float32), fx[tag + "_out"].transpose(2, 0, 1)


@pytest.mark.parametrize("fn,mode", [("gaussian", "color"), ("gaussian", "gray"), ("gaussian", "corr"), ("speckle", "color"),
                                     ("speckle", "gray"), ("speckle", "corr")])
def test_noise_restatement_reproduces_the_reference_bit_for_bit(fn, mode):
    d, x, field, want = _noise_case(f"noise_{fn}_{mode}")
    st = (blindsr._gaussian_stage if fn == "gaussian" else blindsr._speckle_stage)(24, 20, 3, 2, 25, d)
    assert d.done() and st.params["op"] == ("GAUSS_" if fn == "gaussian" else "SPECKLE_") + mode.upper()
    # the recorded field is the noise itself (N(0, level / 255), or the multivariate draw): scale 1, and the correlated
    # draw goes in as a colour field
    got = R.gaussian(x, field, 1.0, "gray" if mode == "gray" else "color", None, fn == "speckle")
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    if mode == "corr":
        cov = cases.fixture()[f"noise_{fn}_{mode}_cov"]
        M = st.params["matrix"]
        assert np.allclose(M @ M.T, cov, rtol=1e-10, atol=1e-18)            # the factor reproduces the covariance
        _, s, v = np.linalg.svd(cov)
        assert np.allclose(M.T, np.sqrt(s)[:, None] * v, atol=1e-12)        # and is numpy's own (the SVD one)
    else:
        level = st.params["scale"] * 255.0
        assert abs(level - round(level)) < 1e-9 and 2 <= round(level) <= 25


@pytest.mark.parametrize("mode", ["color", "gray"])
def test_poisson_restatement_reproduces_the_reference_bit_for_bit(mode):
    d, x, field, want = _noise_case(f"noise_poisson_{mode}")
    st = blindsr._poisson_stage(24, 20, 3, d)
    assert d.done() and st.params["gray"] == (mode == "gray")
    got = R.poisson(x, field, st.params["vals"], st.params["gray"])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # numpy's own np.dot on the float32 image is the fused chain the kernel forms
    q = R.quantise(x)[:, :6]
    assert np.array_equal(R.luminance(q), R.luminance_fma(q))


def test_quantisation_rounds_half_to_even():
    x = ((np.arange(255) + 0.5) / 255.0).astype(np.float32)
    want = np.clip((x * 255.0).round(), 0, 255) / 255.
    assert want.dtype == np.float32 and np.array_equal(R.quantise(x), want)


def test_table_fill_refuses_what_would_leave_a_buffer():
    """the host side of a launch, which needs no GPU: ranges, overlaps, sizes and operations are checked before upload"""
    from ssl_amd import _lib
    K = _lib.CONSTANTS

    def rec(**kw):
        r = np.zeros(1, dtype=blindsr._REC)
        base = dict(C=3, h=8, w=8, oh=8, ow=8, op=3, stride=1)
        for key, v in dict(base, **kw).items():
            r[key] = v
        return r

    def status(family, recs, *sizes, same=False):
        try:
            blindsr.fill_table(family, recs, *sizes, same_buffer=same)
        except RuntimeError as e:
            return int(str(e).rsplit("status ", 1)[1].rstrip(")"))
        return 0

    assert status(blindsr.CONV, rec(), 192, 192, 0, 9) == 0
    assert status(blindsr.CONV, rec(), 191, 192, 0, 9) == K["SSG_E_WORKSPACE"]          # the input leaves its buffer
    assert status(blindsr.CONV, rec(), 192, 191, 0, 9) == K["SSG_E_WORKSPACE"]          # the output does
    assert status(blindsr.CONV, rec(), 192, 192, 0, 8) == K["SSG_E_WORKSPACE"]          # the taps do
    assert status(blindsr.CONV, rec(op=4), 192, 192, 0, 16) == K["SSG_E_BADARG"]        # an even kernel
    assert status(blindsr.CONV, rec(op=11), 192, 192, 0, 121) == K["SSG_E_BADARG"]
    assert status(blindsr.CONV, rec(stride=2), 192, 192, 0, 9) == K["SSG_E_BADARG"]     # oh is not ceil(h / stride)
    assert status(blindsr.CONV, rec(C=2), 192, 192, 0, 9) == K["SSG_E_BADARG"]
    assert status(blindsr.RESIZE, rec(op=0), 192, 192) == K["SSG_E_BADARG"]
    assert status(blindsr.RESIZE, rec(oh=0), 192, 192) == K["SSG_E_BADARG"]
    assert status(blindsr.NOISE, rec(op=0), 192, 192, 191, 0) == K["SSG_E_WORKSPACE"]   # the field leaves its buffer
    assert status(blindsr.NOISE, rec(op=2), 192, 192, 192, 8) == K["SSG_E_WORKSPACE"]   # the matrix does
    assert status(blindsr.NOISE, rec(op=2, C=1), 64, 64, 64, 9) == K["SSG_E_BADARG"]    # correlated noise needs colour
    two = np.concatenate([rec(), rec(out_off=100)])
    assert status(blindsr.RESIZE, two, 192, 400) == K["SSG_E_BADARG"]                   # two outputs overlap
    assert status(blindsr.RESIZE, rec(out_off=100), 400, 400, same=True) == K["SSG_E_BADARG"]   # an output on an input
    assert status(blindsr.RESIZE, rec(out_off=192), 400, 400, same=True) == 0
    table, n_tiles = blindsr.fill_table(blindsr.RESIZE, np.concatenate([rec(oh=9, ow=33), rec(out_off=1000)]), 192, 2000)
    words = table.view(np.int32)
    assert list(words[:7]) == [2, 5, blindsr.RESIZE, 0, 0, 4, 5] and n_tiles == 5      # 2 x 2 tiles, then one


def test_isp_model_must_be_none():
    with pytest.raises(NotImplementedError):
        blindsr.BlindSRDegradation(isp_model=object())
    with pytest.raises(ValueError):
        blindsr.build_program("bsrgan", 100, 100, blindsr.BlindSRDraws(), sf=4, lq_patchsize=72)


@pytest.mark.parametrize("variant,seed,shapes", cases.CHAIN_CASES)
def test_chain_cases_reach_every_stage_kind(variant, seed, shapes):
    """the programs the GPU chain test runs, built here: three images of three sizes whose stages differ slot by slot, with
    every kind of stage but the MATLAB pre-scale, consistent sizes and a crop inside the degraded image"""
    d = cases.seeded_draws(seed)
    progs = [blindsr.build_program(variant, h, w, d, sf=cases.CHAIN_SF, lq_patchsize=cases.CHAIN_PATCH) for h, w in shapes]
    kinds = {s.kind if s.kind != "noise" else s.params["op"].split("_")[0] for p in progs for s in p.stages}
    kinds |= {"strided" for p in progs for s in p.stages if s.kind == "conv" and s.params["stride"] > 1}
    want = {"conv", "resize", "GAUSS", "SPECKLE", "poisson", "jpeg"} if variant == "plus" else {"conv", "strided", "resize", "GAUSS", "jpeg"}
    assert kinds >= want and "imresize" not in kinds
    assert len({tuple(s.kind for s in p.stages) for p in progs}) == 3           # three different stage orders
    for p in progs:
        for a, b in zip(p.stages, p.stages[1:]):
            assert (a.oh, a.ow) == (b.h, b.w)
        assert p.crop[0] + cases.CHAIN_PATCH <= p.stages[-1].oh and p.crop[1] + cases.CHAIN_PATCH <= p.stages[-1].ow
    plan = blindsr._Plan([3] * 3, [p.stages for p in progs])
    image = plan.finish()
    n_stages = sum(len(p.stages) for p in progs)
    assert 0 < plan.launches < n_stages and image.size % 4 == 0 and plan.pool_at % 16 == 0
