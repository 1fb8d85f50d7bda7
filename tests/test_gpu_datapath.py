"""The data-path kernels (ssl_amd/csrc/ssg_datapath.hip, ssg_degrade.hip behind ssl_amd/datapath.py) held to
oracle/datapath_oracle.py beyond the fixture shapes of test_gpu_parity.py (F11-F17): non-square and per-sample
augment / crop, the byte-wide pool swap, every filter2D tap count, the generic USM pass up to 63 taps, resizes at
1-pixel / 1,025-plane / tile-edge shapes, and the noise stages at sizes where every grid-stride loop makes a second trip.

Bounds: the byte moves and the noise stages are bit exact; filter2D 3e-6, USM 2e-6 (no tie in the oracle's residual),
resize 3e-6 -- the project's bounds of F12, F13 and F15.  Inputs and their properties: tests/datapath_cases.py, pinned
by tests/test_cpu_datapath.py.  Every comparison prints one `DPSWEEP` line (pytest -s): kernel, case, worst error, bound.
"""
import random

import numpy as np
import pytest
import torch

import datapath_cases as dc
from oracle import datapath_oracle as dp

dorc = dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from ssl_amd import _lib
    _lib.lib()  # raises if libssg_hip.so is missing: no silent fallback
    return torch.device("cuda:0")


def T(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def report(kernel, case, err, bound):
    print(f"DPSWEEP {kernel:14s} {case:44s} err {err:.3e}  bound {bound:.1e}")


def same_bits(kernel, case, got, want):
    """Bit exact as the project's F11 / F16 tests mean it: equal dtype, shape and every element (np.array_equal); the
    count of differing elements goes to the DPSWEEP line."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (kernel, case, got.dtype, want.dtype, got.shape, want.shape)
    bad = int((got != want).sum())
    report(kernel, case, float(bad), 0.0)
    assert bad == 0, f"{kernel} {case}: {bad} of {got.size} elements differ"


# ------------------------------------------------------------------ 1. augment_crop ----
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("C", [1, 3])
def test_augment_crop_every_flip_on_a_non_square_source(dev, C, dtype):
    """All eight (hflip, vflip, rot90) in one batch of 8 on a 37 x 53 source of distinct values, per-sample origins that
    are all distinct within a batch and put every flip combination at each of the four corners of ITS augmented sample
    and at four interior origins; odd Wo.  Bit exact."""
    from ssl_amd import datapath
    Hs, Ws, Ho, Wo = 37, 53, 20, 23
    x = dc.distinct_source((8, C, Hs, Ws), dtype)
    xg = torch.as_tensor(x, device=dev)
    for shift in range(8):
        tl = dc.corner_origins(dc.FLIPS8, Hs, Ws, Ho, Wo, shift)
        y = datapath.augment_crop(xg, (Ho, Wo), tl, dc.FLIPS8).cpu().numpy()
        same_bits("augment_crop", f"8 flips 37x53 C{C} {np.dtype(dtype).name} shift{shift}", y,
                  dc.augment_crop_oracle(x, (Ho, Wo), tl, dc.FLIPS8))


@pytest.mark.parametrize("rot", [0, 1])
def test_augment_crop_whole_augmented_image(dev, rot):
    """Ho, Wo = Ha, Wa: the crop is the whole augmented sample, 53 x 37 for the rot90 samples of a 37 x 53 source."""
    from ssl_amd import datapath
    flips = [f for f in dc.FLIPS8 if f[2] == rot]
    x = dc.distinct_source((4, 3, 37, 53), np.float32)
    out_hw = (53, 37) if rot else (37, 53)
    tl = [(0, 0)] * 4
    y = datapath.augment_crop(T(x, dev), out_hw, tl, flips).cpu().numpy()
    same_bits("augment_crop", f"whole image rot{rot} -> {out_hw[0]}x{out_hw[1]}", y,
              dc.augment_crop_oracle(x, out_hw, tl, flips))
    with pytest.raises(ValueError):           # one row more than the augmented sample has
        datapath.augment_crop(T(x, dev), (out_hw[0] + 1, out_hw[1]), tl, flips)


def test_augment_crop_refuses_a_crop_that_fits_only_after_rot90(dev):
    """Source 20 x 40, Ho = 30: inside the rot90 sample (40 x 20), outside the unrotated one."""
    from ssl_amd import datapath
    x = dc.distinct_source((2, 3, 20, 40), np.float32)
    xg = T(x, dev)
    rot, tl = [(0, 0, 1), (1, 1, 1)], [(10, 0), (3, 2)]
    y = datapath.augment_crop(xg, (30, 18), tl, rot).cpu().numpy()
    same_bits("augment_crop", "20x40 -> 30x18 after rot90", y, dc.augment_crop_oracle(x, (30, 18), tl, rot))
    for flips in ([(0, 0, 0), (0, 0, 1)], [(0, 0, 1), (1, 1, 0)], None):
        with pytest.raises(ValueError):
            datapath.augment_crop(xg, (30, 18), [(0, 0), (0, 0)], flips)
    with pytest.raises(ValueError):           # left + Wo leaves the rotated sample's 20 columns
        datapath.augment_crop(xg, (30, 18), [(0, 3), (0, 0)], rot)


def test_paired_random_crop_non_square_all_rot(dev):
    """paired_random_crop_img_mask on a 40 x 56 GT / mask batch with all-rot flips (augmented 56 x 40) and its 14 x 10
    LQ, scale 4, seeded: the LQ patch at the drawn origin, GT and mask at 4 x that origin of the augmented samples."""
    from ssl_amd import datapath
    flips = [(0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
    gt = dc.distinct_source((4, 3, 40, 56), np.float32)
    mk = dc.distinct_source((4, 1, 40, 56), np.uint8)
    lq = dc.distinct_source((4, 3, 14, 10), np.float32) + 0.25
    seed = 3
    random.seed(seed)
    top, left = random.randint(0, 14 - 8), random.randint(0, 10 - 8)      # transforms.py:122-123
    assert top > 0 and left > 0
    random.seed(seed)
    g, l, m = datapath.paired_random_crop_img_mask(T(gt, dev), T(lq, dev), torch.as_tensor(mk, device=dev), 32, 4,
                                                   flips=flips)
    assert m.dtype == torch.uint8
    same_bits("augment_crop", "paired crop lq", l.cpu().numpy(), dp.crop_nchw(lq, top, left, 8))
    same_bits("augment_crop", "paired crop gt (rot, scale 4)", g.cpu().numpy(),
              dp.augment_crop_nchw(gt, 4 * top, 4 * left, (32, 32), flips))
    same_bits("augment_crop", "paired crop mask u8 (rot, scale 4)", m.cpu().numpy(),
              dp.augment_crop_nchw(mk, 4 * top, 4 * left, (32, 32), flips))
    with pytest.raises(ValueError):           # the same batch unrotated is 40 x 56, not 4 x (14 x 10)
        datapath.paired_random_crop_img_mask(T(gt, dev), T(lq, dev), torch.as_tensor(mk, device=dev), 32, 4,
                                             flips=[(0, 0, 0)] * 4)


def test_augment_crop_grid_stride_trip(dev):
    """2 x 3 x 1690 x 1710 uint8 cropped to 1680 x 1680: 16,934,400 outputs, more than the 65,536 x 256 of the grid, so
    the loop's `i += gridDim.x * 256` trip runs; mixed flips (one rot90) and origins on a non-square source."""
    from ssl_amd import datapath
    x = dc.distinct_source((2, 3, 1690, 1710), np.uint8)
    flips, tl = [(1, 0, 1), (0, 1, 0)], [(30, 7), (10, 29)]
    assert 2 * 3 * 1680 * 1680 > 65536 * 256
    y = datapath.augment_crop(torch.as_tensor(x, device=dev), (1680, 1680), tl, flips).cpu().numpy()
    same_bits("augment_crop", "2x3x1690x1710 u8 -> 1680x1680 (grid-stride)", y,
              dc.augment_crop_oracle(x, (1680, 1680), tl, flips))


# ------------------------------------------------------------------ 2. pair pool ----
@pytest.mark.parametrize("b", [1, 3, 4, 12])
def test_pair_pool_byte_wide_kernel(dev, b):
    """PairPool(12) with lq 300 B and mask 100 B per sample (no multiple of 16: pool_swap<uint8_t>) beside gt 1,200 B
    (pool_swap<uint4>), 40 exchanges against dp.PairPool with torch's CPU generator seeded alike; b = 12 swaps every
    slot.  Bit exact, every sample of the stream distinct."""
    from ssl_amd import datapath
    stream = dc.pool_stream(b)
    torch.manual_seed(200 + b)
    pool = datapath.PairPool(12)
    got = []
    for lq, gt, mk in stream:
        o = pool.exchange(T(lq, dev), T(gt, dev), torch.as_tensor(mk, device=dev))
        got.append([t.cpu().numpy() for t in o])
    torch.manual_seed(200 + b)
    ref = dp.PairPool(12)
    swapped = 0
    for t, (lq, gt, mk) in enumerate(stream):
        want = ref.exchange([lq, gt, mk], lambda: torch.randperm(12).numpy())
        swapped += int(not np.array_equal(want[0], lq))
        for name, a, w in zip(("lq", "gt", "mask"), got[t], want):
            assert a.dtype == w.dtype and np.array_equal(a, w), (b, t, name)
    assert swapped >= 40 - 12 // b - 1        # (after the fill every exchange hands out pooled samples)
    report("pool_swap", f"PairPool(12) b={b} 40 exchanges", 0.0, 0.0)


@pytest.mark.parametrize("off_q,off_b", [(4, 4), (4, 0), (0, 4), (1, 8)])
def test_pool_swap_alignment_fallback_through_the_c_abi(dev, off_q, off_b):
    """48-byte samples (a multiple of 16) with queue and / or batch pointers off a 16-byte boundary: the byte-wide
    kernel, whose result equals the aligned (wide-kernel) call on the same bytes and the numpy swap; bytes outside the
    samples stay."""
    from ssl_amd import _lib, engine
    L = _lib.lib()
    Q, b, sb, pad = 7, 3, 48, 32
    rng = np.random.default_rng(300 + off_q + 16 * off_b)
    qbuf = rng.integers(0, 256, off_q + Q * sb + pad, dtype=np.uint8)
    bbuf = rng.integers(0, 256, off_b + b * sb + pad, dtype=np.uint8)
    slots = np.array([5, 0, 3], np.int32)
    tq, tb, ts = torch.as_tensor(qbuf, device=dev), torch.as_tensor(bbuf, device=dev), torch.as_tensor(slots, device=dev)
    assert tq.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0
    _lib.check(L.ssg_pool_swap(tq.data_ptr() + off_q, tb.data_ptr() + off_b, sb, engine._ptr(ts), b, engine._stream()))
    # the same bytes on aligned bases: the 16-byte kernel
    aq, ab = torch.as_tensor(qbuf[off_q:off_q + Q * sb].copy(), device=dev), torch.as_tensor(bbuf[off_b:off_b + b * sb].copy(), device=dev)
    assert aq.data_ptr() % 16 == 0 and ab.data_ptr() % 16 == 0
    _lib.check(L.ssg_pool_swap(engine._ptr(aq), engine._ptr(ab), sb, engine._ptr(ts), b, engine._stream()))
    wq, wb = qbuf.copy(), bbuf.copy()
    for k, s in enumerate(slots):
        qs, bs = slice(off_q + s * sb, off_q + (s + 1) * sb), slice(off_b + k * sb, off_b + (k + 1) * sb)
        wq[qs], wb[bs] = bbuf[bs], qbuf[qs]
    gq, gb = tq.cpu().numpy(), tb.cpu().numpy()
    case = f"48 B samples, queue +{off_q} batch +{off_b}"
    same_bits("pool_swap", case + " queue", gq, wq)                       # (includes the bytes outside the samples)
    same_bits("pool_swap", case + " batch", gb, wb)
    assert np.array_equal(gq[off_q:off_q + Q * sb], aq.cpu().numpy()) and np.array_equal(gb[off_b:off_b + b * sb], ab.cpu().numpy())
    assert not np.array_equal(gq, qbuf)


# ------------------------------------------------------------------ 3. filter2D ----
@pytest.mark.parametrize("k", dc.FILTER_KS)
def test_filter2d_every_tap_count(dev, k):
    """Every odd k from 1 to 21 -- off = (K - k) / 2 = 4 .. 0 in filter2d_kernel<9> and 5 .. 0 in filter2d_kernel<21> --
    with per-sample signed kernels without symmetry (sum 1, sum|.| = 4) on 3 x 2 x 17 x 65 (one past the 16 x 64 tile both
    ways) and on the minimum legal side k // 2 + 1 in H and in W: 3e-6 against the fp64 oracle."""
    from ssl_amd import datapath
    kern = dc.filter_kernels(k)
    for tag, img in dc.filter_images(k):
        y = datapath.filter2D(T(img, dev), T(kern, dev)).cpu().numpy()
        err = maxerr(y, dp.filter2d(img, kern))
        report("filter2d", f"k={k} per-sample {tag} {img.shape[2]}x{img.shape[3]}", err, 3e-6)
        assert err <= 3e-6, (k, tag, err)
    # the one shared kernel (nk = 1) takes kernel 0 for every sample
    tag, img = dc.filter_images(k)[0]
    y = datapath.filter2D(T(img, dev), T(kern[1:2], dev)).cpu().numpy()
    err = maxerr(y, dp.filter2d(img, kern[1:2]))
    report("filter2d", f"k={k} shared {tag}", err, 3e-6)
    assert err <= 3e-6, (k, err)


# ------------------------------------------------------------------ 4. USMSharp ----
@pytest.mark.parametrize("tag", [c[0] for c in dc.USM_CASES])
def test_usm_sharp_generic_path(dev, tag):
    """usm_pass with the tap count at run time: the fixed OpenCV tables (1, 3, 5, 7 taps, sigma 0), 7 taps at sigma 1.1,
    31 taps, 63 taps (row tile 128 + 62 wide) at the minimum side 32 x 32 and at 70 x 131, and widths 127 / 128 / 129
    with heights 63 / 64 / 65; thresholds other than 10.  The oracle's residual has no tie on any case (asserted on the
    oracle alone), so the mask is decided: 2e-6 against the fp64 oracle, the bound of F12."""
    from ssl_amd import datapath
    img, kw, out, res = dc.usm_case(tag)
    assert dc.usm_ties(res, kw["threshold"]) == 0
    mod = datapath.USMSharp(radius=kw["radius"], sigma=kw["sigma"])
    assert mod.radius == kw["radius"]
    y = mod(T(img.copy(), dev), weight=kw["weight"], threshold=kw["threshold"]).cpu().numpy()
    err = maxerr(y, out)
    report("usm_sharp", f"{tag} thr {kw['threshold']} w {kw['weight']}", err, 2e-6)
    assert err <= 2e-6, (tag, err)


# ------------------------------------------------------------------ 5. interpolate ----
@pytest.mark.parametrize("mode", dc.RESIZE_MODES)
def test_interpolate_beyond_the_fixture_shapes(dev, mode):
    """ssg_resize at 1-pixel inputs and outputs, 1-row and 1-column sources (every bicubic tap clamps), a tuple
    scale_factor, 1,025 planes (the `p += gridDim.z` trip) and output widths 63 / 64 / 65 with heights 3 / 4 / 5: 3e-6
    against the fp32 oracle and against torch.nn.functional.interpolate on the CPU (the two agree to 1e-6 at these
    shapes, test_cpu_datapath.py)."""
    from ssl_amd import datapath
    for tag, shape, kw in dc.RESIZE_CASES:
        x = dc.resize_input(tag)
        o32, t32 = dc.resize_refs(tag, mode)
        y = datapath.interpolate(T(x.copy(), dev), mode=mode, **kw).cpu().numpy()
        assert y.shape == o32.shape == t32.shape, (tag, y.shape, o32.shape)
        eo, et = maxerr(y, o32), maxerr(y, t32)
        report("resize", f"{mode} {tag} vs oracle32", eo, 3e-6)
        report("resize", f"{mode} {tag} vs torch cpu", et, 3e-6)
        assert eo <= 3e-6 and et <= 3e-6, (mode, tag, eo, et)


# ------------------------------------------------------------------ 6. noise stages and clamp_round ----
BIG = 8192 * 256      # elements one trip of the element-wise grid-stride loops covers (blocks_for's cap x 256 threads)


@pytest.mark.parametrize("rounds", [False, True])
def test_gaussian_noise_beyond_one_grid_trip(dev, rounds):
    """4 x 3 x 419 x 421 = 2,116,788 elements (> 8,192 x 256; HW = 176,399 is odd), per-sample sigmas, gray flags
    (1, 0, 1, 0) with the shared gray field, all-zero flags with and without one: bit exact against the fp32 oracle."""
    from ssl_amd import datapath
    B, C, H, W = 4, 3, 419, 421
    assert B * C * H * W > BIG and (H * W) % 256
    rng = np.random.default_rng(1800)
    img = dc.q8(rng, B, C, H, W)
    fc, fg = rng.standard_normal((B, C, H, W)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32)
    sigma = np.array([1.0, 30.0, 7.3, 18.9], np.float32)
    gray, zero = np.array([1, 0, 1, 0], np.float32), np.zeros(4, np.float32)
    x, tfc, tfg, ts = T(img, dev), T(fc, dev), T(fg, dev), T(sigma, dev)
    y = datapath.add_gaussian_noise(x, ts, T(gray, dev), tfc, tfg, True, rounds).cpu().numpy()
    same_bits("gaussian_noise", f"4x3x419x421 gray 1010 rounds={rounds}", y,
              dorc.gaussian_noise(img, sigma, gray, fc, fg, True, rounds))
    want = dorc.gaussian_noise(img, sigma, zero, fc, None, True, rounds)
    y = datapath.add_gaussian_noise(x, ts, T(zero, dev), tfc, None, True, rounds).cpu().numpy()
    same_bits("gaussian_noise", f"4x3x419x421 gray 0000 no field rounds={rounds}", y, want)
    y = datapath.add_gaussian_noise(x, ts, T(zero, dev), tfc, tfg, True, rounds).cpu().numpy()
    same_bits("gaussian_noise", f"4x3x419x421 gray 0000 unused field rounds={rounds}", y, want)
    y = datapath.add_gaussian_noise(x, ts, T(gray, dev), tfc, tfg, False, rounds).cpu().numpy()
    same_bits("gaussian_noise", f"4x3x419x421 gray 1010 no clip rounds={rounds}", y,
              dorc.gaussian_noise(img, sigma, gray, fc, fg, False, rounds))


def test_clamp_round_beyond_one_grid_trip(dev):
    """2,097,152 + 4,321 values over [-0.2, 1.2] with the half-integer levels among them, all four (clip, rounds)."""
    from ssl_amd import datapath
    v = dc.clamp_round_input(BIG + 4321)
    x = T(v, dev)
    for clip in (True, False):
        for rounds in (True, False):
            same_bits("clamp_round", f"n={v.size} clip={clip} rounds={rounds}",
                      datapath.clamp_round(x, clip, rounds).cpu().numpy(), dorc.clip_round(v, clip, rounds))


def _poisson_check(dev, case, x, gray, scale, with_gray, settings=((True, False), (True, True), (False, False))):
    from ssl_amd import datapath
    B = x.shape[0]
    xg = T(x, dev)
    rate, rate_gray, vals = datapath.poisson_rates(xg, with_gray)
    r = dorc.poisson_rates(x, with_gray)
    same_bits("poisson_rates", case + " rate", rate.cpu().numpy(), r["rate"])
    same_bits("poisson_rates", case + " vals", vals[:, 0].cpu().numpy(), r["vals"].reshape(-1))
    dcol, dgray = dc.poisson_draws(r["rate"], 11), None
    if with_gray:
        same_bits("poisson_rates", case + " rate_gray", rate_gray.cpu().numpy(), r["rate_gray"])
        same_bits("poisson_rates", case + " vals_gray", vals[:, 1].cpu().numpy(), r["vals_gray"].reshape(-1))
        dgray = dc.poisson_draws(r["rate_gray"], 12)
    else:
        assert rate_gray is None
    for clip, rounds in settings:
        y = datapath.add_poisson_noise(xg, T(scale, dev), T(gray, dev), vals, T(dcol, dev),
                                       None if dgray is None else T(dgray, dev), clip, rounds).cpu().numpy()
        same_bits("poisson_noise", f"{case} clip={clip} rounds={rounds}", y,
                  dorc.poisson_noise(x, scale, gray, dcol, dgray, clip, rounds))
    return r


@pytest.mark.parametrize("perturb", [False, True])
def test_poisson_level_census_counts(dev, perturb):
    """Samples holding exactly 1, 2, 3, 4, 5, 128, 129, 256 distinct levels, so vals must be 1, 2, 4, 4, 8, 128, 256, 256
    (`vals_of`'s shift loop on both sides of every power of two): for the colour and the gray census alike on the
    gray-valued batch, for the gray census alone on the perturbed batch whose colour census holds more levels; inputs
    slightly outside [0, 1] (the level clamp), gray flags (1, 0, 1, 0, 1, 0, 0, 1).  Rates, vals and the noise
    arithmetic after the draw are bit exact against the fp32 oracle."""
    x = dc.poisson_level_batch(perturb)
    scale = np.linspace(0.05, 3.0, 8).astype(np.float32)
    r = _poisson_check(dev, f"levels perturb={perturb}", x, np.array(dc.POISSON_GRAY, np.float32), scale, True)
    want = np.array(dc.POISSON_VALS, np.float32)
    assert np.array_equal(r["vals_gray"].ravel(), want)
    assert np.array_equal(r["vals"].ravel(), want) != perturb


def test_poisson_one_channel_without_gray(dev):
    x = dc.poisson_level_batch(False)[:3, :1].copy()          # C = 1: 1, 2 and 3 levels
    _poisson_check(dev, "C=1 no gray", x, np.zeros(3, np.float32), np.array([0.5, 1.0, 2.5], np.float32), False)


def test_poisson_sample_beyond_one_grid_trip(dev):
    """1 x 1 x 1456 x 1456 = 2,119,936 pixels in one sample: the per-sample pixel loops of the census (64 blocks), the
    rates and the noise kernel (256 blocks each) run 130 and 33 trips; 200 levels -> vals 256."""
    rng = np.random.default_rng(1900)
    x = (rng.integers(28, 228, (1, 1, 1456, 1456)) / 255 + rng.uniform(-0.001, 0.001, (1, 1, 1456, 1456))).astype(np.float32)
    assert x.size > BIG
    r = _poisson_check(dev, "1x1x1456x1456", x, np.zeros(1, np.float32), np.array([1.7], np.float32), False,
                       settings=((True, False),))
    assert float(r["vals"].ravel()[0]) == 256.0


def test_poisson_gray_three_channels_beyond_the_census_grid(dev):
    """2 x 3 x 300 x 301 with gray flags (0, 1): HW = 90,300 is above the 64 x 256 pixels of one census trip and the
    256 x 256 of one rates / noise trip, with the gray path on."""
    rng = np.random.default_rng(1901)
    x = (dc.q8(rng, 2, 3, 300, 301) + rng.uniform(-0.001, 0.001, (2, 3, 300, 301))).astype(np.float32)
    _poisson_check(dev, "2x3x300x301 gray 01", x, np.array([0, 1], np.float32), np.array([0.3, 2.0], np.float32), True,
                   settings=((True, False), (True, True)))
