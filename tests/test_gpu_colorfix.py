"""The colour-correction kernels (ssl_amd/csrc/ssg_colorfix.hip) on the GPU against the fp64 restatement of
tests/colorfix_reference.py, element by element within its bounds, and against the reference's recorded float32 outputs
(tests/golden/f27_colorfix.npz) within twice them (each side is within one bound of fp64).

The tile pass works on 64 x 64 tiles with a halo of up to 31: 200 x 197 has four tiles along each axis, so tiles with a
full halo inside the image on all sides; 70 x 90 has ragged tiles both ways; 33 x 17, 5 x 40 and 1 x 1 are smaller than
the larger radii, so both clamps act inside one tap.  No grid is capped.  The statistics fold chunks of 4,096 elements
with 256 threads: 300 x 301 has 23 chunks, 1030 x 1021 has 257 (a second trip of the fold).

Every check prints `PARITY <case> <largest error / bound>`; profiles/colorfix_parity.txt is that output."""
import functools
import os

import numpy as np
import pytest
import torch

import colorfix_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f27_colorfix.npz")

WAVELET_SHAPES = [(1, 1, 1, 1), (1, 3, 5, 40), (1, 3, 33, 17), (2, 3, 70, 90), (1, 2, 200, 197)]
ADAIN_SHAPES = [(1, 3, 1, 2), (2, 3, 70, 90), (1, 1, 300, 301), (1, 1, 1030, 1021)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def CF():
    from ssl_amd import colorfix
    return colorfix


@functools.lru_cache(maxsize=None)
def pair(shape, content="random"):
    """(content, style) float32: the content in [-1.2, 1.2] (a sample overshoots), the style in [-1, 1]."""
    B, C, H, W = shape
    rng = np.random.default_rng(1000 * H + W + 7 * C + B)
    s = rng.uniform(-1, 1, shape).astype(np.float32)
    if content == "random":
        c = rng.uniform(-1.2, 1.2, shape)
    elif content == "vstep":                                # a vertical edge: columns left of W / 2 low, the rest high
        c = np.where(np.arange(W)[None, None, None, :] < W // 2, -1.1, 0.9) + 0.0 * s
    elif content == "hstep":
        c = np.where(np.arange(H)[None, None, :, None] < H // 2, 0.8, -1.2) + 0.0 * s
    else:                                                   # impulses: the four corners and an interior pixel
        c = np.zeros(shape)
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3)):
            c[..., y, x] = 1.2
    c = c.astype(np.float32)
    c.setflags(write=False), s.setflags(write=False)
    return c, s


@functools.lru_cache(maxsize=None)
def recon64(shape, content, levels):
    c, s = pair(shape, content)
    out = R.wavelet_reconstruction(c, s, levels, np.float64)
    out.setflags(write=False)
    return out


def T(a, dev):
    return torch.as_tensor(np.array(a, order='C'), device=dev)      # (a copy: the cached inputs are read-only)


def _bits(t):
    return t if t.dtype == torch.uint8 else t.view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])


def within(name, got, want64, bound):
    """Every element of `got` within `bound` of `want64`; prints the largest share of the bound used."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    err = np.abs(got - want64)
    bound = np.broadcast_to(bound, err.shape)
    assert bool(np.isfinite(got).all()), name
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"PARITY {name} {frac:.4f}")
    assert bool((err <= bound).all()), (name, frac)


# ---------------------------------------------------------------------------------------------- wavelet kernels ---
@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("shape", WAVELET_SHAPES)
def test_wavelet_reconstruction_random(dev, CF, shape, levels):
    c, s = pair(shape)
    got = CF.color_fix(T(c, dev), T(s, dev), kind="wavelet", out="raw", levels=levels)
    assert got.dtype == torch.float32
    within(f"wavelet {shape} levels {levels} random", got, recon64(shape, "random", levels), R.wavelet_bound(c, s))


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["vstep", "hstep", "impulse"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 40), (2, 3, 70, 90), (1, 2, 200, 197)])
def test_wavelet_reconstruction_edges_and_impulses(dev, CF, shape, content):
    c, s = pair(shape, content)
    got = CF.wavelet_reconstruction(T(c, dev), T(s, dev))
    within(f"wavelet {shape} {content}", got, recon64(shape, content, 5), R.wavelet_bound(c, s))
    # the same impulse content decomposed: a corner's doubled weights and the interior's spread, against the restatement
    if content == "impulse":
        high, low = CF.wavelet_decomposition(T(c, dev))
        h64, l64 = R.wavelet_decomposition(c, dtype=np.float64)
        within(f"decompose low {shape} impulse", low, l64, R.wavelet_bound(c))
        within(f"decompose high {shape} impulse", high, h64, R.wavelet_bound(c))


@pytest.mark.gpu
def test_one_pixel_image_gives_the_style(dev, CF):
    c, s = pair((1, 1, 1, 1))
    got = CF.wavelet_reconstruction(T(c, dev), T(s, dev)).cpu().numpy()
    assert abs(float(got[0, 0, 0, 0]) - float(s[0, 0, 0, 0])) <= float(R.wavelet_bound(c, s)[0, 0, 0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("shape", WAVELET_SHAPES)
def test_wavelet_decomposition_either_output_and_both(dev, CF, shape, levels):
    c, _ = pair(shape)
    x = T(c, dev)
    h64, l64 = R.wavelet_decomposition(c, levels, np.float64)
    bound = R.wavelet_bound(c)
    high, low = CF.wavelet_decomposition(x, levels)
    within(f"decompose high {shape} levels {levels}", high, h64, bound)
    within(f"decompose low {shape} levels {levels}", low, l64, bound)
    h_only, none = CF.wavelet_decomposition(x, levels, want=("high",))
    assert none is None and torch.equal(_bits(h_only), _bits(high))
    none, l_only = CF.wavelet_decomposition(x, levels, want=("low",))
    assert none is None and torch.equal(_bits(l_only), _bits(low))


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 3, 16, 100])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 5, 40), (2, 3, 70, 90)])
def test_wavelet_blur(dev, CF, shape, radius):
    assert radius != 100 or radius > max(shape[2:])         # one radius larger than both sides
    c, _ = pair(shape)
    got = CF.wavelet_blur(T(c, dev), radius)
    within(f"blur {shape} radius {radius}", got, R.wavelet_blur(c, radius, np.float64), R.wavelet_bound(c))


@pytest.mark.gpu
def test_wavelet_blur_huge_radius_does_not_overflow(dev, CF):
    c, _ = pair((1, 3, 5, 40))
    a, b = CF.wavelet_blur(T(c, dev), 2 ** 31 - 1), CF.wavelet_blur(T(c, dev), 100)
    assert torch.equal(_bits(a), _bits(b))                  # both clamp every outer tap onto the border


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_inputs_are_computed_in_fp32(dev, CF, dtype):
    shape = (2, 3, 70, 90)
    c, s = (T(a, dev).to(dtype) for a in pair(shape))
    cu, su = c.float(), s.float()
    for kind in ("wavelet", "adain"):
        for out in ("raw", "unit"):
            got = CF.color_fix(c, s, kind=kind, out=out)
            assert got.dtype == dtype
            assert torch.equal(_bits(got), _bits(CF.color_fix(cu, su, kind=kind, out=out).to(dtype)))
        assert torch.equal(CF.color_fix(c, s, kind=kind, out="uint8"), CF.color_fix(cu, su, kind=kind, out="uint8"))
    cn, sn = cu.cpu().numpy(), su.cpu().numpy()
    within(f"wavelet {shape} {dtype} upcast", CF.color_fix(cu, su, out="raw"),
           R.wavelet_reconstruction(cn, sn, dtype=np.float64), R.wavelet_bound(cn, sn))
    mixed = CF.wavelet_reconstruction(c, su)                # the promoted dtype of the two inputs
    assert mixed.dtype == torch.float32 and torch.equal(_bits(mixed), _bits(CF.wavelet_reconstruction(cu, su)))
    high, low = CF.wavelet_decomposition(c)
    assert high.dtype == low.dtype == dtype
    m, sd = CF.calc_mean_std(c)
    assert m.dtype == sd.dtype == dtype and m.shape == sd.shape == (2, 3, 1, 1)


@pytest.mark.gpu
def test_non_contiguous_inputs(dev, CF):
    shape = (2, 3, 70, 90)
    c, s = pair(shape)
    ct = T(c.transpose(0, 1, 3, 2), dev).permute(0, 1, 3, 2)        # (2,3,70,90) with strides of (2,3,90,70)
    st = T(np.concatenate([s, s], 3), dev)[..., ::2]                # every other column of a wider tensor
    sn = np.concatenate([s, s], 3)[..., ::2]
    assert not ct.is_contiguous() and not st.is_contiguous() and ct.shape == st.shape == shape
    within("wavelet non-contiguous", CF.wavelet_reconstruction(ct, st), R.wavelet_reconstruction(c, sn, dtype=np.float64),
           R.wavelet_bound(c, sn))
    within("adain non-contiguous", CF.adaptive_instance_normalization(ct, st),
           R.adaptive_instance_normalization(c, sn, np.float64), R.adain_bound(c, sn))


# ------------------------------------------------------------------------------------------------ AdaIN kernels ---
def _stats_close(name, stats, c, s):
    """The device's (2, B C, 2) statistics against numpy's fp64 ones, 1e-12 relative each."""
    got = stats.cpu().numpy()
    worst = 0.0
    for i, img in enumerate((c, s)):
        m, sd = R.calc_mean_std(img, dtype=np.float64)
        for j, want in enumerate((m.reshape(-1), sd.reshape(-1))):
            rel = np.abs(got[i, :, j] - want) / np.abs(want)
            worst = max(worst, float(rel.max()))
    print(f"PARITY {name} statistics {worst / R.STATS_RTOL:.4f}")
    assert worst <= R.STATS_RTOL, (name, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ADAIN_SHAPES)
def test_adain_against_fp64(dev, CF, shape):
    c, s = pair(shape)
    ct, st = T(c, dev), T(s, dev)
    stats = CF._stats(ct, st)
    assert stats.shape == (2, shape[0] * shape[1], 2) and stats.dtype == torch.float64
    _stats_close(f"adain {shape}", stats, c, s)
    got = CF.adaptive_instance_normalization(ct, st)
    within(f"adain {shape}", got, R.adaptive_instance_normalization(c, s, np.float64), R.adain_bound(c, s))
    m, sd = CF.calc_mean_std(ct)
    assert m.shape == sd.shape == (shape[0], shape[1], 1, 1) and m.dtype == torch.float32
    assert torch.equal(m.reshape(-1), stats[0, :, 0].float()) and torch.equal(sd.reshape(-1), stats[0, :, 1].float())
    # the fixed-order fold: the same bits again, and for a plane alone as inside its batch
    assert torch.equal(_bits(CF._stats(ct, st)), _bits(stats))
    alone = CF._stats(ct[-1:, -1:].contiguous(), st[-1:, -1:].contiguous())
    assert torch.equal(_bits(alone[:, 0]), _bits(stats[:, -1]))
    one = CF._stats(st, None)
    assert one.shape == (1, shape[0] * shape[1], 2) and torch.equal(_bits(one[0]), _bits(stats[1]))


@pytest.mark.gpu
def test_adain_plane_of_one_element_is_nan(dev, CF):
    c, s = pair((1, 3, 1, 1))
    stats = CF._stats(T(c, dev), T(s, dev)).cpu().numpy()
    assert np.array_equal(stats[0, :, 0], c.reshape(-1).astype(np.float64)) and bool(np.isnan(stats[:, :, 1]).all())
    got = CF.adaptive_instance_normalization(T(c, dev), T(s, dev))
    assert got.shape == (1, 3, 1, 1) and bool(torch.isnan(got).all())
    unit = CF.color_fix(T(c, dev), T(s, dev), kind="adain", out="unit")
    assert bool(torch.isnan(unit).all())                    # torch's clamp keeps a NaN
    assert torch.equal(_bits(CF._stats(T(c, dev), T(s, dev))), _bits(CF._stats(T(c, dev), T(s, dev))))


@pytest.mark.gpu
def test_adain_flat_content_plane(dev, CF):
    shape = (1, 2, 20, 30)
    c, s = (a.copy() for a in pair(shape))
    c[0, 0] = np.float32(0.37)
    stats = CF._stats(T(c, dev), T(s, dev))
    got = stats.cpu().numpy()
    # the shifted sums of a flat plane are exactly 0 (the square root within two units in the last place)
    assert got[0, 0, 0] == float(np.float32(0.37)) and abs(got[0, 0, 1] - np.sqrt(1e-5)) <= 1e-18
    _stats_close("adain flat plane", stats, c, s)
    within("adain flat plane", CF.adaptive_instance_normalization(T(c, dev), T(s, dev)),
           R.adaptive_instance_normalization(c, s, np.float64), R.adain_bound(c, s))


# ---------------------------------------------------------------------------------------------------- epilogues ---
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wavelet", "adain", "nofix"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 40), (2, 3, 70, 90), (1, 2, 200, 197)])
def test_epilogues(dev, CF, shape, kind):
    c, s = pair(shape)
    ct, st = T(c, dev), T(s, dev)
    raw = CF.color_fix(ct, st, kind=kind, out="raw")
    unit = CF.color_fix(ct, st, kind=kind, out="unit")
    assert torch.equal(_bits(unit), _bits(torch.clamp((raw + 1) / 2, 0, 1)))       # bit for bit
    if kind != "adain":                                     # the content overshoots [-1, 1] both ways: both clamps act
        assert float(unit.min()) == 0.0 and float(unit.max()) == 1.0
    u8 = CF.color_fix(ct, st, kind=kind, out="uint8")
    B, C, H, W = shape
    assert u8.dtype == torch.uint8 and u8.shape == (B, H, W, C) and u8.is_contiguous()
    if kind == "wavelet":
        v64, bound = recon64(shape, "random", 5), R.wavelet_bound(c, s)
    elif kind == "adain":
        v64, bound = R.adaptive_instance_normalization(c, s, np.float64), R.adain_bound(c, s)
    else:
        v64, bound = c.astype(np.float64), np.zeros((1, 1, 1, 1))
        assert torch.equal(_bits(raw), _bits(ct))
    ok, decided = R.byte_check(u8.cpu().numpy(), v64, bound)
    print(f"PARITY bytes {kind} {shape} decided {decided:.5f}")
    assert ok and decided >= 0.99
    # the bytes are the truncation of 255 times the kernel's own unit output, in NHWC
    assert torch.equal(u8, (unit * 255.0).to(torch.uint8).permute(0, 2, 3, 1))


@pytest.mark.gpu
def test_nofix_needs_no_init_image(dev, CF):
    c, _ = pair((1, 3, 5, 40))
    assert torch.equal(CF.color_fix(T(c, dev), None, kind="nofix"), torch.clamp((T(c, dev) + 1) / 2, 0, 1))


# ------------------------------------------------------------------------------------------------------ fixture ---
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
def test_against_the_recorded_reference(dev, CF, n):
    with np.load(GOLDEN) as z:
        g = {k[3:]: z[k] for k in z.files if k.startswith(f"c{n}_")}
    c, s = g["content"], g["style"]
    ct, st = T(c, dev), T(s, dev)
    wb, wb2 = 2 * R.wavelet_bound(c), 2 * R.wavelet_bound(c, s)
    high, low = CF.wavelet_decomposition(ct)
    for name, got, bound in (("blur1", CF.wavelet_blur(ct, 1), wb), ("blur16", CF.wavelet_blur(ct, 16), wb),
                             ("high", high, wb), ("low", low, wb), ("recon", CF.wavelet_reconstruction(ct, st), wb2),
                             ("adain", CF.adaptive_instance_normalization(ct, st), 2 * R.adain_bound(c, s))):
        within(f"fixture {n} {name} (of twice the bound)", got, g[name].astype(np.float64), bound)
    for img, t, tag in ((c, ct, "c"), (s, st, "s")):
        m, sd = CF.calc_mean_std(t)
        # the reference's float32 reduction of a few thousand values: 2^-20 of the plane's magnitude, as the fixture's
        # own script holds it to fp64; the kernel's statistics are fp64 rounded once
        tol = 2.0 ** -20 * float(np.abs(img).max()) + 2.0 ** -24 * 1.2
        assert float(np.abs(m.cpu().numpy() - g["mean_" + tag]).max()) <= tol
        assert float(np.abs(sd.cpu().numpy() - g["std_" + tag]).max()) <= tol


# ----------------------------------------------------------------------------------------------------- PIL pair ---
@pytest.mark.gpu
def test_pil_pair(dev, CF):
    from PIL import Image
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:24, 0:20]
    base = 128 + 90 * np.sin(0.3 * x[..., None] + np.arange(3)) * np.cos(0.2 * y[..., None])
    tgt = np.clip(base + rng.normal(0, 20, base.shape), 0, 255).astype(np.uint8)
    src = np.clip(0.6 * base + 70 + rng.normal(0, 10, base.shape), 0, 255).astype(np.uint8)
    for fn, ref in ((CF.adain_color_fix, R.adain_color_fix), (CF.wavelet_color_fix, R.wavelet_color_fix)):
        out = fn(Image.fromarray(tgt), Image.fromarray(src))
        assert isinstance(out, Image.Image) and out.mode == "RGB" and out.size == (20, 24)
        got, want = np.asarray(out).astype(int), ref(tgt, src).astype(int)
        # a truncation may fall either way where the float32 evaluations straddle an integer: rarely, and by one
        assert int(np.abs(got - want).max()) <= 1 and float((got == want).mean()) >= 0.99
    grey = CF.wavelet_color_fix(Image.fromarray(np.ascontiguousarray(tgt[..., 0])),
                                Image.fromarray(np.ascontiguousarray(src[..., 0])))
    assert grey.mode == "L" and grey.size == (20, 24)


# ------------------------------------------------------------------------------------------------------- poison ---
def poison_cases():
    """Outputs of every kernel of the file, for test_gpu_colorfix_poison.py: the tile pass at three level counts and its
    three epilogues, both decomposition outputs over interior tiles, the blur, the statistics over 23 chunks, the apply
    pass, and the NaN plane."""
    from ssl_amd import colorfix as CF
    dev = torch.device("cuda:0")
    out = []
    c, s = (T(a, dev) for a in pair((2, 3, 70, 90)))
    out += [CF.color_fix(c, s, out=o) for o in ("raw", "unit", "uint8")]                    # 0 1 2
    out += [CF.color_fix(c, s, out="raw", levels=l) for l in (1, 3)]                        # 3 4
    out += [CF.color_fix(c, s, kind="adain", out=o) for o in ("raw", "uint8")]              # 5 6
    out.append(CF.wavelet_blur(c, 16))                                                      # 7
    c, s = (T(a, dev) for a in pair((1, 2, 200, 197)))
    out += list(CF.wavelet_decomposition(c))                                                # 8 9
    out.append(CF.wavelet_reconstruction(c, s))                                             # 10
    c, s = (T(a, dev) for a in pair((1, 3, 5, 40)))
    out.append(CF.wavelet_reconstruction(c, s))                                             # 11
    c, s = (T(a, dev) for a in pair((1, 1, 300, 301)))
    out.append(CF._stats(c, s))                                                             # 12
    c, s = (T(a, dev) for a in pair((1, 3, 1, 1)))
    out += [CF._stats(c, s), CF.adaptive_instance_normalization(c, s)]                      # 13 14: the NaN plane
    torch.cuda.synchronize()
    return out
