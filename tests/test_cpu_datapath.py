"""The reference side of tests/test_gpu_datapath.py, pinned on the CPU where no fixture reaches: the numpy oracle
(oracle/datapath_oracle.py) against torch's own CPU evaluation of the same calls at the sweep's shapes, and the
properties of the sweep's inputs (tests/datapath_cases.py) that the GPU comparisons take for granted; and the refusals
of the data path's C-ABI entry points, which are decided before anything is launched.  CPU only.
"""
import ctypes

import numpy as np
import pytest
import torch

import datapath_cases as dc
from oracle import datapath_oracle as dp


@pytest.mark.parametrize("mode", dc.RESIZE_MODES)
def test_resize_oracle_equals_torch_cpu_at_the_sweep_shapes(mode):
    """dp.interpolate(dtype=float32) and torch.nn.functional.interpolate on the CPU (the reference's own call) agree
    to 1e-6 with equal shapes at every shape of the sweep (measured: <= 9e-7, bicubic; both round the same fp32
    expression in slightly different orders) -- the GPU test's 3e-6 reference is then itself pinned there."""
    worst = 0.0
    for tag, shape, kw in dc.RESIZE_CASES:
        o, t = dc.resize_refs(tag, mode)
        assert o.shape == t.shape and o.dtype == np.float32, (tag, o.shape, t.shape)
        err = float(np.abs(o.astype(np.float64) - t).max())
        worst = max(worst, err)
        assert err <= 1e-6, (tag, mode, err)
    print(f"resize {mode}: oracle vs torch CPU worst {worst:.2e}")


def test_resize_sweep_reaches_the_paths_it_names():
    """The shapes the sweep is about, stated on the case table: more planes than the 1,024 of the grid's z extent, 1-pixel
    inputs and outputs, 1-row and 1-column sources, a tuple scale_factor, output widths on both sides of the 64-lane
    tile with output heights on both sides of the 4-row tile."""
    cases = {tag: (shape, kw) for tag, shape, kw in dc.RESIZE_CASES}
    assert max(s[0] * s[1] for s, _ in cases.values()) > 1024
    outs = {tag: dc.resize_refs(tag, "bilinear")[0].shape[-2:] for tag in cases}
    assert outs["1x1"] == (1, 1) and outs["5x130_to_1x1"] == (1, 1)
    assert any(s[2] == 1 and s[3] > 1 for s, _ in cases.values()) and any(s[3] == 1 and s[2] > 1 for s, _ in cases.values())
    assert any(isinstance(kw.get("scale_factor"), tuple) for _, kw in cases.values())
    assert {(h, w) for h in (3, 4, 5) for w in (63, 64, 65)} <= set(outs.values())
    assert outs["33x65_sf0.11"] == (3, 7) and outs["23x200_sf1/3"] == (7, 66) and outs["41x29_sf0.5x1.7"] == (20, 49)


@pytest.mark.parametrize("tag", [c[0] for c in dc.USM_CASES])
def test_usm_cases_have_no_tie_and_fp32_reaches_the_bound(tag):
    """On the oracle alone: no residual of the case lies within 1e-3 / 255 of its threshold, so the sharpening mask is
    decided at fp32; and the same separable expression in float32 numpy is within 1e-6 of the fp64 oracle (measured
    <= 2.1e-7), so the project's 2e-6 bound is one a right fp32 kernel meets on this case."""
    img, kw, out, res = dc.usm_case(tag)
    assert dc.usm_ties(res, kw["threshold"]) == 0
    assert float(np.abs(dc.usm_sharp_fp32(img, **kw) - out).max()) <= 1e-6
    r = kw["radius"] // 2
    assert img.shape[-2] > r and img.shape[-1] > r


def test_usm_cases_cover_the_generic_path():
    taps = {c[1] for c in dc.USM_CASES}
    assert {1, 3, 5, 7, 9, 31, 63} <= taps and 51 not in taps
    assert any(c[1] == 7 and c[2] > 0 for c in dc.USM_CASES) and any(c[1] == 63 and c[5][-2:] == (32, 32) for c in dc.USM_CASES)
    assert len({c[4] for c in dc.USM_CASES}) >= 4                # thresholds other than 10
    for k, tab in ((1, [1.0]), (3, [0.25, 0.5, 0.25])):
        assert np.array_equal(dp.gaussian_kernel_1d(k, 0.0), tab)
    # sigma > 0 leaves the fixed table: the two 7-tap cases use different taps
    assert np.abs(dp.gaussian_kernel_1d(7, 0.0) - dp.gaussian_kernel_1d(7, 1.1)).max() > 1e-3


@pytest.mark.parametrize("k", dc.FILTER_KS)
def test_filter_kernels_are_normalised_signed_and_asymmetric(k):
    K = dc.filter_kernels(k).astype(np.float64)
    assert K.shape == (3, k, k)
    assert np.abs(K.sum((1, 2)) - 1).max() <= 1e-6 and np.abs(K).sum((1, 2)).max() <= 4 + 1e-6
    for _, img in dc.filter_images(k):
        assert min(img.shape[-2:]) > k // 2
    if k == 1:
        return
    assert (K < 0).any() and np.abs(K[0] - K[1]).max() > 1e-3 and np.abs(K[1] - K[2]).max() > 1e-3
    for kb in K:   # no axis, transpose or point symmetry: a kernel read flipped, transposed or rotated is another kernel
        for other in (kb[::-1], kb[:, ::-1], kb.T, kb[::-1, ::-1], kb[::-1].T, kb[:, ::-1].T):
            assert np.abs(kb - other).max() > 1e-3


def test_filter2d_oracle_equals_torch_conv2d():
    """dp.filter2d against the reference's formulation (reflect pad + conv2d, img_process_util.py:7-31) in torch fp64, at
    k = 5 in a (3,2,17,65) batch with per-sample kernels."""
    k = 5
    img, kern = dc.filter_images(k)[0][1], dc.filter_kernels(k)
    x = torch.nn.functional.pad(torch.from_numpy(img).double(), (2, 2, 2, 2), mode="reflect")
    b, c, ph, pw = x.shape
    y = torch.nn.functional.conv2d(x.view(1, b * c, ph, pw),
                                   torch.from_numpy(kern).double().view(b, 1, k, k).repeat(1, c, 1, 1).view(b * c, 1, k, k),
                                   groups=b * c).view(b, c, 17, 65)
    assert np.abs(dp.filter2d(img, kern) - y.numpy()).max() <= 1e-14


def test_augment_oracle_on_non_square_sources_equals_torch_flips():
    """dp.augment_crop_nchw on a 37 x 53 source against torch.flip / transpose in the reference's order (hflip, vflip,
    transpose), all eight combinations, whole image and a crop at the far corner."""
    x = dc.distinct_source((8, 3, 37, 53), np.float32)
    for b, (h, v, r) in enumerate(dc.FLIPS8):
        t = torch.from_numpy(x[b])
        t = t.flip(-1) if h else t
        t = t.flip(-2) if v else t
        t = t.transpose(-1, -2) if r else t
        Ha, Wa = t.shape[-2:]
        assert (Ha, Wa) == ((53, 37) if r else (37, 53))
        assert np.array_equal(dp.augment_crop_nchw(x[b:b + 1], 0, 0, (Ha, Wa), [(h, v, r)])[0], t.numpy())
        assert np.array_equal(dp.augment_crop_nchw(x[b:b + 1], Ha - 20, Wa - 23, (20, 23), [(h, v, r)])[0],
                              t[:, Ha - 20:, Wa - 23:].numpy())
    tl = [dc.corner_origins(dc.FLIPS8, 37, 53, 20, 23, s) for s in range(8)]
    for i, (_, _, r) in enumerate(dc.FLIPS8):       # every sample meets the four corners of its augmented sample, always inside
        mt, ml = (53 - 20, 37 - 23) if r else (37 - 20, 53 - 23)
        assert {(0, 0), (mt, ml), (0, ml), (mt, 0)} <= {tl[s][i] for s in range(8)}
        assert all(0 <= tl[s][i][0] <= mt and 0 <= tl[s][i][1] <= ml for s in range(8))
    assert all(len(set(t)) == 8 for t in tl)        # per-sample origins, all distinct within a batch


def test_pool_stream_samples_are_distinct_and_reach_the_byte_wide_kernel():
    for b in (1, 3, 4, 12):
        st = dc.pool_stream(b)
        lq, gt, mk = (np.concatenate([s[i] for s in st]).reshape(40 * b, -1) for i in range(3))
        for a in (lq, gt, mk):
            assert len(np.unique(a, axis=0)) == 40 * b
        assert lq[0].nbytes == 300 and gt[0].nbytes == 1200 and mk[0].nbytes == 100
        assert lq[0].nbytes % 16 and mk[0].nbytes % 16 and gt[0].nbytes % 16 == 0
        assert 12 % b == 0


def test_poisson_level_batches_hold_the_level_counts_they_claim():
    """Colour and gray census of the constructed batches, by the oracle (np.unique): vals = 1, 2, 4, 4, 8, 128, 256, 256
    for both on the gray-valued batch, for the gray census alone on the perturbed batch (whose colour census differs
    wherever it can); some values lie outside [0, 1]."""
    want = np.array(dc.POISSON_VALS, np.float32)
    plain, pert = dp.poisson_rates(dc.poisson_level_batch(False), True), dp.poisson_rates(dc.poisson_level_batch(True), True)
    assert np.array_equal(plain["vals"].ravel(), want) and np.array_equal(plain["vals_gray"].ravel(), want)
    assert np.array_equal(pert["vals_gray"].ravel(), want)
    assert (pert["vals"].ravel() != want).sum() >= 5
    for p in (False, True):
        x = dc.poisson_level_batch(p)
        assert x.min() < -0.002 and x.max() > 1.002
        n = [len(np.unique(np.clip(np.rint(x[s] * np.float32(255)), 0, 255))) for s in range(8)]
        assert p or tuple(n) == dc.POISSON_LEVELS


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _torch_clip_round(out, clip, rounds):
    """degradations.py:501-507 / 668-674, literally."""
    if clip and rounds:
        return torch.clamp((out * 255.0).round(), 0, 255) / 255.
    if clip:
        return torch.clamp(out, 0, 1)
    if rounds:
        return (out * 255.0).round() / 255.
    return out


@pytest.mark.parametrize("clip,rounds", [(True, True), (True, False), (False, True), (False, False)])
def test_noise_oracles_equal_torch_fp32_bit_for_bit(clip, rounds):
    """The fp32 oracles of the noise stages against the reference's expressions (degradations.py:455-507, 601-674)
    evaluated by torch on the CPU in fp32, on the sweep's own inputs: bit exact.  This is what decides, should the GPU
    differ from the oracle in a bit, which of the two left the reference's expression."""
    v = dc.clamp_round_input(70001)
    assert np.array_equal(dp.clip_round(v, clip, rounds), _torch_clip_round(_t(v), clip, rounds).numpy())
    rng = np.random.default_rng(1700)
    B, C, H, W = 4, 3, 19, 23
    img = dc.q8(rng, B, C, H, W) + rng.uniform(-0.002, 0.002, (B, C, H, W)).astype(np.float32)
    sigma = rng.uniform(1, 30, B).astype(np.float32)
    gray = np.array([1, 0, 1, 0], np.float32)
    fc, fg = rng.standard_normal((B, C, H, W)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32)
    s4, g4 = _t(sigma).view(B, 1, 1, 1), _t(gray).view(B, 1, 1, 1)
    noise = _t(fc) * s4 / 255.
    noise_gray = _t(fg) * s4 / 255.
    ref = _torch_clip_round(_t(img) + (noise * (1 - g4) + noise_gray * g4), clip, rounds)
    assert np.array_equal(dp.gaussian_noise(img, sigma, gray, fc, fg, clip, rounds), ref.numpy())
    ref0 = _torch_clip_round(_t(img) + noise, clip, rounds)
    assert np.array_equal(dp.gaussian_noise(img, sigma, np.zeros(B, np.float32), fc, None, clip, rounds), ref0.numpy())
    # Poisson, on the perturbed level batch (colour and gray census differ)
    x = dc.poisson_level_batch(True)
    r = dp.poisson_rates(x, True)
    dcol, dgray = dc.poisson_draws(r["rate"], 1), dc.poisson_draws(r["rate_gray"], 2)
    scale = rng.uniform(0.05, 3, 8).astype(np.float32)
    g8 = np.array(dc.POISSON_GRAY, np.float32)
    tx = _t(x)
    tg = 0.2989 * tx[:, 0:1] + 0.587 * tx[:, 1:2] + 0.114 * tx[:, 2:3]
    tg = torch.clamp((tg * 255.0).round(), 0, 255) / 255.
    vg = torch.tensor([2 ** np.ceil(np.log2(len(torch.unique(tg[i])))) for i in range(8)], dtype=torch.float32).view(8, 1, 1, 1)
    ng = _t(dgray) / vg - tg
    tr = torch.clamp((tx * 255.0).round(), 0, 255) / 255.
    vc = torch.tensor([2 ** np.ceil(np.log2(len(torch.unique(tr[i])))) for i in range(8)], dtype=torch.float32).view(8, 1, 1, 1)
    assert np.array_equal(r["rate"], (tr * vc).numpy()) and np.array_equal(r["rate_gray"], (tg * vg).numpy())
    nz = _t(dcol) / vc - tr
    gg = _t(g8).view(8, 1, 1, 1)
    nz = (nz * (1 - gg) + ng * gg) * _t(scale).view(8, 1, 1, 1)
    ref = _torch_clip_round(tx + nz, clip, rounds)
    assert np.array_equal(dp.poisson_noise(x, scale, g8, dcol, dgray, clip, rounds), ref.numpy())


# ---- the C ABI's refusals, in the order include/ssg_hip.h documents them: decided before any launch ----
def _fake(k):
    return ctypes.c_void_p(k << 20)       # never dereferenced: every call below returns before anything reads it


def test_c_abi_augment_crop_and_pool_swap_refuse_before_any_launch():
    from ssl_amd import _lib
    L = _lib.lib()
    BAD = -1
    src, dst, par = _fake(1), _fake(2), _fake(3)
    ok = dict(src=src, dst=dst, eb=4, B=2, C=3, Hs=9, Ws=8, Ho=5, Wo=4, par=par)

    def crop(**kw):
        a = dict(ok, **kw)
        return L.ssg_augment_crop(a["src"], a["dst"], a["eb"], a["B"], a["C"], a["Hs"], a["Ws"], a["Ho"], a["Wo"], a["par"], None)

    for name in ("src", "dst", "par"):
        assert crop(**{name: None}) == BAD
    assert crop(B=-1) == BAD
    for name in ("C", "Hs", "Ws", "Ho", "Wo"):
        for v in (0, -3):
            assert crop(**{name: v}) == BAD
    for eb in (2, 0, 3, 8, -4):
        assert crop(eb=eb) == BAD
    assert crop(B=0) == 0                                   # nothing to move: no launch
    assert crop(B=0, eb=2) == BAD and crop(B=0, src=None) == BAD   # ... but the arguments are checked first

    q, b, s = _fake(4), _fake(5), _fake(6)
    assert L.ssg_pool_swap(None, b, 48, s, 2, None) == BAD
    assert L.ssg_pool_swap(q, None, 48, s, 2, None) == BAD
    assert L.ssg_pool_swap(q, b, 48, None, 2, None) == BAD
    assert L.ssg_pool_swap(q, b, 48, s, -1, None) == BAD
    assert L.ssg_pool_swap(q, b, 48, s, 0, None) == 0 and L.ssg_pool_swap(q, b, 0, s, 2, None) == 0   # nothing to move
    assert L.ssg_pool_swap(None, b, 0, s, 0, None) == BAD   # checked first


def test_c_abi_usm_sharp_refuses_before_any_launch():
    from ssl_amd import _lib
    L = _lib.lib()
    BAD, WS, SMALL = -1, -3, -4
    img, out, scr = _fake(1), _fake(2), _fake(3)
    ok = dict(img=img, out=out, B=2, C=3, H=40, W=37, radius=50, scr=scr, nb=None)

    def usm(**kw):
        a = dict(ok, **kw)
        nb = L.ssg_usm_scratch_bytes(a["B"], a["C"], a["H"], a["W"]) if a["nb"] is None else a["nb"]
        return L.ssg_usm_sharp(a["img"], a["out"], a["B"], a["C"], a["H"], a["W"], a["radius"], 0.0, 0.5, 10.0, a["scr"], nb, None)

    assert L.ssg_usm_scratch_bytes(2, 3, 40, 37) == 3 * 4 * 2 * 3 * 40 * 37
    # every call is refused by exactly what it names: the rest of `ok` would be served (H, W = 40, 37 > 51 / 2)
    assert usm(B=-1) == BAD and usm(radius=-1) == BAD
    for name in ("C", "H", "W"):
        for v in (0, -2):
            assert usm(**{name: v}) == BAD
    assert usm(B=0) == 0
    assert usm(B=0, img=None, out=None, scr=None, nb=0) == 0        # B == 0 is answered before the pointers are looked at
    assert usm(B=0, C=0) == BAD and usm(B=0, radius=-1) == BAD      # ... and after the sizes
    for name in ("img", "out", "scr"):
        assert usm(**{name: None}) == BAD
    assert usm(out=img) == BAD                                     # img == out
    full = L.ssg_usm_scratch_bytes(2, 3, 40, 37)
    assert usm(nb=full - 1) == WS and usm(nb=0) == WS
    assert usm(scr=None, nb=0) == BAD and usm(out=img, nb=0) == BAD  # pointers before the scratch size
    for radius in (64, 65, 1000):                                   # kernel sizes 65, 65, 1001: more than 63 taps
        assert usm(radius=radius) == BAD
        assert usm(radius=radius, nb=full - 1) == WS                # the scratch size before the kernel size
        assert usm(radius=radius, H=3) == BAD                       # the kernel size before the image size
    for radius, side in ((50, 25), (51, 25), (63, 31), (62, 31), (3, 1), (2, 1)):   # kernel size radius | 1; H, W <= R
        assert usm(radius=radius, H=side) == SMALL and usm(radius=radius, W=side) == SMALL
        assert usm(radius=radius, H=side, nb=12 * 2 * 3 * side * 37 - 1) == WS      # the scratch size before the image size
    assert usm(H=1, W=1) == SMALL


def test_c_abi_filter2d_and_diffjpeg_refuse_before_any_launch():
    from ssl_amd import _lib
    L = _lib.lib()
    BAD, SMALL = -1, -4
    img, ker, out = _fake(1), _fake(2), _fake(3)
    ok = dict(img=img, ker=ker, out=out, B=2, C=3, H=17, W=30, k=7, nk=2)

    def filt(**kw):
        a = dict(ok, **kw)
        return L.ssg_filter2d(a["img"], a["ker"], a["out"], a["B"], a["C"], a["H"], a["W"], a["k"], a["nk"], None)

    assert filt(B=-1) == BAD
    for name in ("C", "H", "W"):
        for v in (0, -2):
            assert filt(**{name: v}) == BAD
    assert filt(B=0) == 0
    assert filt(B=0, img=None, ker=None, out=None, k=4, nk=7) == 0   # B == 0 is answered before anything else but the sizes
    assert filt(B=0, W=0) == BAD
    for name in ("img", "ker", "out"):
        assert filt(**{name: None}) == BAD
    assert filt(out=img) == BAD
    for k in (0, -1, 2, 4, 20, 22, 23, 51):                          # even, non-positive, more than 21
        assert filt(k=k) == BAD
        assert filt(k=k, H=1, W=1) == BAD                            # the kernel size before the image size
    for nk in (0, 3, -1):                                            # neither 1 nor B
        assert filt(nk=nk) == BAD
        assert filt(nk=nk, k=21, H=10) == BAD                        # ... before the image size too
    for k, side in ((7, 3), (21, 10), (3, 1), (9, 4)):
        assert filt(k=k, H=side) == SMALL and filt(k=k, W=side) == SMALL and filt(k=k, H=side, nk=1) == SMALL
        assert filt(k=k, H=side, img=None) == BAD and filt(k=k, H=side, out=img) == BAD   # the pointers before the image size

    def jpeg(img=img, out=out, B=2, H=17, W=30, qdev=None, q=50.0):
        return L.ssg_diffjpeg(img, out, B, H, W, qdev, q, None)

    assert jpeg(B=-1) == BAD
    for v in (0, -2):
        assert jpeg(H=v) == BAD and jpeg(W=v) == BAD
    assert jpeg(B=0) == 0 and jpeg(B=0, img=None, out=None, q=0.0) == 0
    assert jpeg(B=0, H=0) == BAD
    assert jpeg(img=None) == BAD and jpeg(out=None) == BAD
    for q in (0.0, -5.0, float("nan"), -float("inf")):               # no device qualities and no positive host quality
        assert jpeg(q=q) == BAD
    assert jpeg(img=None, qdev=ker, q=0.0) == BAD
