"""The colour correction's restatement (tests/colorfix_reference.py) against the reference's recorded outputs
(tests/golden/f27_colorfix.npz, written by make_golden_colorfix.py) and against constructions of its own, and what of
ssl_amd.colorfix and its C ABI can be checked without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import colorfix_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f27_colorfix.npz")
CASES = (0, 1)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(golden, n):
    return {k[len(f"c{n}_"):]: v for k, v in golden.items() if k.startswith(f"c{n}_")}


def test_fixture_shapes_and_ranges(golden):
    shapes = {0: (1, 3, 40, 56), 1: (1, 3, 5, 40)}
    for n in CASES:
        g = _case(golden, n)
        assert g["content"].shape == g["style"].shape == shapes[n]
        assert g["content"].dtype == g["style"].dtype == np.float32
        assert abs(float(np.abs(g["content"]).max()) - 1.2) < 1e-6 and abs(float(np.abs(g["style"]).max()) - 1.0) < 1e-6
        # textured, not flat: every plane has contrast
        assert float(g["content"].std(axis=(2, 3)).min()) > 0.1 and float(g["style"].std(axis=(2, 3)).min()) > 0.1
    assert os.path.getsize(GOLDEN) < 256 * 1024


@pytest.mark.parametrize("n", CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_against_the_recorded_reference(golden, n, dtype):
    """fp64: the reference's float32 result lies within one bound of it; fp32: both are float32 evaluations, each within
    one bound of fp64, so within two of each other."""
    g = _case(golden, n)
    c, s = g["content"], g["style"]
    k = 1 if dtype == np.float64 else 2
    wb, wb2 = k * R.wavelet_bound(c), k * R.wavelet_bound(c, s)
    high, low = R.wavelet_decomposition(c, dtype=dtype)
    assert high.dtype == dtype
    for name, got, bound in (("blur1", R.wavelet_blur(c, 1, dtype), wb), ("blur16", R.wavelet_blur(c, 16, dtype), wb),
                             ("high", high, wb), ("low", low, wb),
                             ("recon", R.wavelet_reconstruction(c, s, dtype=dtype), wb2),
                             ("adain", R.adaptive_instance_normalization(c, s, dtype), k * R.adain_bound(c, s))):
        assert got.shape == g[name].shape, name
        assert bool((np.abs(got.astype(np.float64) - g[name]) <= bound).all()), name
    for img, tag in ((c, "c"), (s, "s")):
        m, sd = R.calc_mean_std(img, dtype=dtype)
        assert m.shape == g["mean_" + tag].shape == (1, 3, 1, 1)
        # a float32 reduction of a few thousand values: 2^-20 of the plane's magnitude (make_golden_colorfix.py)
        tol = 2.0 ** -20 * float(np.abs(img).max()) * k
        assert float(np.abs(m - g["mean_" + tag]).max()) <= tol and float(np.abs(sd - g["std_" + tag]).max()) <= tol


@pytest.mark.parametrize("shape", [(2, 3, 40, 56), (1, 3, 5, 40), (1, 2, 1, 1), (1, 1, 70, 90)])
@pytest.mark.parametrize("levels", [1, 3, 5])
def test_linear_form_equals_two_decompositions(shape, levels):
    rng = np.random.default_rng(sum(shape) + levels)
    c, s = rng.uniform(-1.2, 1.2, shape), rng.uniform(-1, 1, shape)
    a = R.wavelet_reconstruction(c, s, levels)
    b = R.wavelet_reconstruction_linear(c, s, levels)
    assert float(np.abs(a - b).max()) <= 1e-14
    high, low = R.wavelet_decomposition(c, levels)
    assert float(np.abs(high - (c - low)).max()) <= 1e-14          # the per-level differences telescope


def _operator(n, radius):
    """The 1-D blur as a matrix, built from its definition: row j gathers 1/4, 1/2, 1/4 at clamp(j - r), j, clamp(j + r)."""
    m = np.zeros((n, n))
    for j in range(n):
        for d, w in ((-radius, 0.25), (0, 0.5), (radius, 0.25)):
            m[j, min(max(j + d, 0), n - 1)] += w
    return m


@pytest.mark.parametrize("H,W", [(5, 40), (40, 56)])
@pytest.mark.parametrize("where", ["corner", "interior"])
def test_impulse_responses(H, W, where):
    y, x = (0, 0) if where == "corner" else (H // 2, W // 2)
    img = np.zeros((1, 1, H, W))
    img[0, 0, y, x] = 1.0
    # one level: the separable outer product of the clamped 1-D operators' columns
    for r in (1, 2, 16):
        want = np.outer(_operator(H, r)[:, y], _operator(W, r)[:, x])
        assert float(np.abs(R.wavelet_blur(img, r)[0, 0] - want).max()) <= 1e-15
    # five levels: the product of the five operators per axis
    my, mx = np.eye(H), np.eye(W)
    for i in range(5):
        my, mx = _operator(H, 2 ** i) @ my, _operator(W, 2 ** i) @ mx
    high, low = R.wavelet_decomposition(img)
    assert float(np.abs(low[0, 0] - np.outer(my[:, y], mx[:, x])).max()) <= 1e-15
    assert float(np.abs(high + low - img).max()) <= 1e-15
    b1 = R.wavelet_blur(img, 1)[0, 0]
    if where == "corner":
        # the taps at -1 are clamped onto the corner: 1/4 + 1/2 per axis there, 1/4 next to it
        assert b1[0, 0] == 0.75 * 0.75 and b1[0, 1] == 0.75 * 0.25 and b1[1, 0] == 0.25 * 0.75 and b1[1, 1] == 0.0625
        assert b1.sum() == 1.0                                    # (a row of the operator sums to 1, a column need not)
        b16 = R.wavelet_blur(img, 16)[0, 0]
        # radius 16 from the corner: every pixel up to 16 away (or to the far side) has its -16 tap clamped onto it
        assert b16[0, 0] == 0.5625 and np.all(b16[0, 1:min(16, W - 1) + 1] == 0.1875)
        assert np.all(b16[1:min(16, H - 1) + 1, 1:min(16, W - 1) + 1] == 0.0625)
    else:
        assert b1[y, x] == 0.25 and b1[y, x + 1] == 0.125 and b1[y + 1, x + 1] == 0.0625 and b1.sum() == 1.0
        # no tap of an interior impulse is clamped while the support 2^levels - 1 fits: the mass stays 1
        levels = max(l for l in range(1, 6) if 2 ** l - 1 <= min(y, x, H - 1 - y, W - 1 - x))
        assert levels == (1 if H == 5 else 4)
        assert abs(R.wavelet_decomposition(img, levels)[1].sum() - 1.0) <= 1e-15


def test_interior_impulse_mass_through_five_levels():
    img = np.zeros((1, 1, 70, 90))
    img[0, 0, 35, 45] = 1.0
    low = R.wavelet_decomposition(img)[1]
    assert abs(low.sum() - 1.0) <= 1e-15 and low[0, 0, 35 - 31, 45 - 31] == 0.0625 ** 5 and low[0, 0, 3, 45] == 0.0


def test_one_pixel_image_gives_the_style():
    c, s = np.array([[[[0.3]], [[-1.1]]]]), np.array([[[[-0.7]], [[0.25]]]])
    # every tap is the one pixel: low = the image, high = 0, up to the fp64 roundings of the nine-term sums
    assert float(np.abs(R.wavelet_reconstruction(c, s) - s).max()) <= 1e-15
    assert float(np.abs(R.wavelet_reconstruction_linear(c, s) - s).max()) <= 1e-15


def test_adain_edge_planes():
    c = np.array([[[[0.3]], [[-1.1]]]])
    m, s = R.calc_mean_std(c)
    assert np.array_equal(m, c) and bool(np.isnan(s).all())
    assert bool(np.isnan(R.adaptive_instance_normalization(c, c)).all())
    flat = np.full((1, 2, 4, 5), 0.37)
    m, s = R.calc_mean_std(flat)
    assert float(np.abs(s - np.sqrt(1e-5)).max()) <= 1e-17 and float(np.abs(m - 0.37).max()) <= 1e-16
    x = np.random.default_rng(3).uniform(-1, 1, (1, 2, 1, 2))
    m, s = R.calc_mean_std(x)                               # two elements: var = (a - b)^2 / 2
    assert float(np.abs(s[0, :, 0, 0] - np.sqrt((x[0, :, 0, 0] - x[0, :, 0, 1]) ** 2 / 2 + 1e-5)).max()) <= 1e-16


def test_byte_check_decides_and_forgives_only_near_an_integer():
    v = np.array([[[[-1.5, 1.5, 0.0, 2 * 100.25 / 255 - 1, 2 * 100.0 / 255 - 1]]]])
    good = np.array([0, 255, 127, 100, 99], np.uint8).reshape(1, 1, 5, 1)
    ok, decided = R.byte_check(good, v, 1e-6)
    assert ok and decided == 0.8                             # only the last value sits on an integer
    for bad in ([1, 255, 127, 100, 99], [0, 254, 127, 100, 99], [0, 255, 127, 101, 99], [0, 255, 127, 100, 98]):
        assert not R.byte_check(np.array(bad, np.uint8).reshape(1, 1, 5, 1), v, 1e-6)[0]
    assert R.byte_check(np.array([0, 255, 127, 100, 100], np.uint8).reshape(1, 1, 5, 1), v, 1e-6)[0]


# -------------------------------------------------------------------------------------------------- host checks ---
NAMES = ("ssg_wavelet_blur", "ssg_wavelet_decompose", "ssg_colorfix_wavelet", "ssg_colorfix_stats", "ssg_colorfix_adain",
         "ssg_colorfix_workspace_bytes")
PY_NAMES = ("wavelet_blur", "wavelet_decomposition", "wavelet_reconstruction", "calc_mean_std",
            "adaptive_instance_normalization", "adain_color_fix", "wavelet_color_fix", "color_fix")
FAKE = ctypes.c_void_p(1 << 20)        # a non-null, 16-byte aligned address that a refused call never touches
FAKE2 = ctypes.c_void_p(2 << 20)
FAKE3 = ctypes.c_void_p(3 << 20)


def _declaration(hdr, name):
    m = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_symbols_exported_declared_and_bound():
    from ssl_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.HEADER).read()
    kinds = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    for name in NAMES:
        assert hasattr(L, name)
        res, args = _lib.PROTOTYPES[name]
        decl = _declaration(hdr, name)
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):
            want = ctypes.c_void_p if ("*" in d or d.startswith("ssg_stream_t")) else kinds[d.split()[0]]
            assert a is want, (name, d)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
    for i, k in enumerate(("RAW", "UNIT", "U8_NHWC")):
        assert re.search(rf"#define SSG_COLORFIX_{k} {i}\b", hdr)
    assert L.ssg_abi_version() == 6
    import ssl_amd
    from ssl_amd import colorfix as CF
    assert ssl_amd.colorfix is CF and "colorfix" in ssl_amd.__all__
    for name in PY_NAMES:
        assert callable(getattr(CF, name)) and name in CF.__all__
    assert (CF.OUT_RAW, CF.OUT_UNIT, CF.OUT_UINT8) == (0, 1, 2)


def test_c_abi_refuses_before_any_launch():
    from ssl_amd import _lib
    L = _lib.lib()
    BAD, BIG, WS, ALIGN = -1, -2, -3, -5
    ok = (1, 3, 40, 56)
    assert L.ssg_wavelet_blur(None, *ok, 1, FAKE, None) == BAD
    assert L.ssg_wavelet_blur(FAKE, *ok, 1, None, None) == BAD
    assert L.ssg_wavelet_blur(FAKE, *ok, 1, FAKE, None) == BAD          # in place
    assert L.ssg_wavelet_blur(FAKE, *ok, 0, FAKE2, None) == BAD
    for shape in ((0, 3, 40, 56), (1, 0, 40, 56), (1, 3, 0, 56), (1, 3, 40, -1)):
        assert L.ssg_wavelet_blur(FAKE, *shape, 1, FAKE2, None) == BAD
        assert L.ssg_colorfix_wavelet(FAKE, FAKE2, *shape, 5, 0, FAKE3, None) == BAD
        assert L.ssg_colorfix_adain(FAKE, None, *shape, 0, FAKE3, None) == BAD
        assert L.ssg_colorfix_workspace_bytes(*shape) == 0
    big = (4, 3, 16384, 16384)                                         # 2^31 elements and more
    assert L.ssg_wavelet_blur(FAKE, *big, 1, FAKE2, None) == BIG
    assert L.ssg_colorfix_wavelet(FAKE, FAKE2, *big, 5, 0, FAKE3, None) == BIG
    assert L.ssg_colorfix_workspace_bytes(*big) == 0
    assert L.ssg_wavelet_decompose(FAKE, *ok, 5, None, None, None) == BAD
    assert L.ssg_wavelet_decompose(FAKE, *ok, 5, FAKE, None, None) == BAD
    assert L.ssg_wavelet_decompose(FAKE, *ok, 5, FAKE2, FAKE2, None) == BAD
    assert L.ssg_wavelet_decompose(FAKE, *ok, 0, FAKE2, FAKE3, None) == BAD
    assert L.ssg_wavelet_decompose(FAKE, *ok, 6, FAKE2, FAKE3, None) == BIG
    assert L.ssg_colorfix_wavelet(FAKE, None, *ok, 5, 0, FAKE3, None) == BAD
    assert L.ssg_colorfix_wavelet(FAKE, FAKE2, *ok, 5, 0, FAKE, None) == BAD
    assert L.ssg_colorfix_wavelet(FAKE, FAKE2, *ok, 5, 3, FAKE3, None) == BAD
    assert L.ssg_colorfix_wavelet(FAKE, FAKE2, *ok, 6, 0, FAKE3, None) == BIG
    nb = L.ssg_colorfix_workspace_bytes(*ok)
    assert nb == 256                                                    # 2 images x 3 planes x 1 chunk x 3 doubles, padded
    assert L.ssg_colorfix_workspace_bytes(1, 1, 300, 301) == 1280       # 23 chunks x 48 bytes, padded to 256
    assert L.ssg_colorfix_stats(FAKE, FAKE2, *ok, 1e-5, None, FAKE3, nb, None) == BAD
    assert L.ssg_colorfix_stats(FAKE, FAKE2, *ok, -1.0, FAKE3, FAKE3, nb, None) == BAD
    assert L.ssg_colorfix_stats(FAKE, FAKE2, *ok, float("nan"), FAKE3, FAKE3, nb, None) == BAD
    assert L.ssg_colorfix_stats(FAKE, FAKE2, *ok, 1e-5, FAKE2, FAKE3, nb - 1, None) == WS
    assert L.ssg_colorfix_stats(FAKE, FAKE2, *ok, 1e-5, FAKE2, ctypes.c_void_p((3 << 20) + 8), nb, None) == ALIGN
    assert L.ssg_colorfix_adain(FAKE, None, *ok, 5, FAKE3, None) == BAD
    assert L.ssg_colorfix_adain(FAKE, None, *ok, 2, FAKE, None) == BAD  # bytes over their own input


def test_python_argument_errors_without_a_device():
    from ssl_amd import colorfix as CF
    a, b = torch.zeros(1, 3, 8, 9), torch.zeros(1, 3, 8, 10)
    with pytest.raises(ValueError, match="differ in shape"):
        CF.wavelet_reconstruction(a, b)
    with pytest.raises(ValueError, match="differ in shape"):
        CF.adaptive_instance_normalization(a, b)
    with pytest.raises(ValueError, match="differ in shape"):
        CF.color_fix(a, b)
    with pytest.raises(ValueError, match="4D"):
        CF.calc_mean_std(a[0])
    with pytest.raises(TypeError):
        CF.wavelet_blur(a.to(torch.uint8), 1)
    with pytest.raises(ValueError, match="radius"):
        CF.wavelet_blur(a, 0)
    for levels in (0, 6, 2.0):
        with pytest.raises(NotImplementedError):
            CF.wavelet_decomposition(a, levels)
        with pytest.raises(NotImplementedError):
            CF.color_fix(a, a, levels=levels)
    with pytest.raises(ValueError, match="kind"):
        CF.color_fix(a, a, kind="histogram")
    with pytest.raises(ValueError, match="out"):
        CF.color_fix(a, a, out="png")
    with pytest.raises(ValueError, match="init_image"):
        CF.color_fix(a, None, kind="adain")
    g = a.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no backward"):
        CF.color_fix(g, a)
    with pytest.raises(RuntimeError, match="no backward"):
        CF.wavelet_reconstruction(a, g)
    # the package has no CPU path
    for call in (lambda: CF.wavelet_reconstruction(a, a), lambda: CF.calc_mean_std(a), lambda: CF.wavelet_blur(a, 1),
                 lambda: CF.color_fix(a, None, kind="nofix"), lambda: CF.color_fix(g.detach(), a, kind="adain", out="uint8")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        CF.color_fix(g, a)                                              # without grad mode only the device is wrong
