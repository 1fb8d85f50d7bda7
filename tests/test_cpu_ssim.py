"""The SSIM criterion's restatement and bound (tests/ssim_reference.py) against the reference's recorded results
(tests/golden/f28_ssim.npz, written by make_golden_ssim.py) and against autograd, and what of ssl_amd.losses.ssim and its
C ABI can be checked without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ssim_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f28_ssim.npz")
N_CASES = 12


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(golden, n):
    g = {k[len(f"c{n}_"):]: torch.from_numpy(np.asarray(v)) for k, v in golden.items() if k.startswith(f"c{n}_")}
    g["ws"], g["avg"] = int(g["ws"]), bool(g["avg"])
    x = g["x"]
    g["coef"] = g["gout"].double() / (x.numel() if g["avg"] else x[0].numel())
    return g


def test_fixture_holds_numbers_only_and_stays_small(golden):
    assert sum(1 for k in golden if k.endswith("_x")) == N_CASES
    for k, v in golden.items():
        assert v.dtype in (np.float32, np.float64, np.int64), k
    assert float(max(np.abs(v).max() for k, v in golden.items() if k.endswith(("_x", "_y")))) <= 1.0
    largest = max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
                  if f.endswith(".npz") and f != "f28_ssim.npz")
    assert os.path.getsize(GOLDEN) <= min(largest, 1 << 20)
    shapes = {tuple(golden[f"c{n}_x"].shape) for n in range(N_CASES)}
    assert {(1, 1, 1, 1), (1, 1, 7, 5), (1, 3, 11, 11), (2, 2, 20, 23), (1, 2, 36, 40)} == shapes
    assert [int(golden[f"c{n}_ws"]) for n in range(5)] == [11, 11, 3, 7, 11] and not int(golden["c4_avg"])


@pytest.mark.parametrize("n", range(N_CASES))
def test_restatement_equals_fp64_autograd_through_the_reference(golden, n):
    """1e-11 of max|grad| (where x == y the gradient's terms cancel to zero, max|grad| is rounding noise and the gap is
    measured against the terms' size)."""
    g = _case(golden, n)
    assert torch.equal(g["window"].double(), R.window(g["ws"]))
    assert float((R.ssim(g["x"], g["y"], g["ws"], g["avg"]) - g["loss64"]).abs().max()) <= 1e-13
    rx, ry = R.gradients(g["x"], g["y"], g["ws"], g["coef"])
    scale = max(float(g["gx64"].abs().max()), float(g["gy64"].abs().max()))
    if torch.equal(g["x"], g["y"]):
        scale = R.term_scale(g["x"], g["y"], g["ws"], g["coef"])
    gap = max(float((rx - g["gx64"]).abs().max()), float((ry - g["gy64"]).abs().max()))
    print(f"case {n}: gap {gap:.3e}, scale {scale:.3e}")
    assert gap <= 1e-11 * scale


@pytest.mark.parametrize("n", range(N_CASES))
def test_analytic_gradient_equals_autograd_of_the_restatement(golden, n):
    g = _case(golden, n)
    a = g["x"].double().requires_grad_(True)
    b = g["y"].double().requires_grad_(True)
    w = R.window(g["ws"])
    m = R.moments(a, b, w)
    S = R.point(m, R.nodes(m))[0]
    (S * R._coef(g["coef"], a.shape)).sum().backward()
    rx, ry = R.gradients(g["x"], g["y"], g["ws"], g["coef"])
    scale = max(R.term_scale(g["x"], g["y"], g["ws"], g["coef"]), 1e-300)
    assert float((rx - a.grad).abs().max()) <= 1e-11 * scale and float((ry - b.grad).abs().max()) <= 1e-11 * scale


@pytest.mark.parametrize("n", range(N_CASES))
def test_the_reference_itself_meets_the_bound(golden, n):
    """The reference's own fp32 loss and gradients lie within the derived bound of the fp64 restatement: the bound the
    kernels are held to on the GPU is one the reference meets."""
    g = _case(golden, n)
    lb, bx, by = R.bounds(g["x"], g["y"], g["ws"], g["coef"])
    lb = lb.mean() if g["avg"] else lb
    rx, ry = R.gradients(g["x"], g["y"], g["ws"], g["coef"])
    shares = (R.share(g["loss"], R.ssim(g["x"], g["y"], g["ws"], g["avg"]), lb), R.share(g["gx"], rx, bx),
              R.share(g["gy"], ry, by))
    print(f"case {n}: the reference uses {shares[0]:.3e} / {shares[1]:.3e} / {shares[2]:.3e} of the bounds")
    assert max(shares) <= 1.0


def test_bound_is_linear_in_the_coefficient_and_symmetric():
    x, y = R.content("smooth", (2, 2, 20, 17), seed=3)
    l1, bx1, by1 = R.bounds(x, y, 11, torch.tensor([1.0, 1.0]))
    l2, bx2, by2 = R.bounds(x, y, 11, torch.tensor([0.5, -3.0]))
    s = torch.tensor([0.5, 3.0]).reshape(2, 1, 1, 1)
    assert torch.allclose(bx2, bx1 * s, rtol=1e-12, atol=0) and torch.equal(l1, l2)
    l3, bx3, by3 = R.bounds(y, x, 11, torch.tensor([1.0, 1.0]))
    assert torch.allclose(bx3, by1, rtol=1e-9, atol=0) and torch.allclose(l3, l1, rtol=1e-9, atol=0)
    gx, gy = R.gradients(x, y, 11)
    hx, hy = R.gradients(y, x, 11)
    assert torch.allclose(gx, hy, rtol=1e-9, atol=1e-18) and torch.allclose(gy, hx, rtol=1e-9, atol=1e-18)


def test_zero_images_give_one_and_no_gradient():
    z = torch.zeros(1, 2, 9, 13)
    assert bool((R.ssim_map(z, z) == 1.0).all())
    gx, gy = R.gradients(z, z)
    assert not bool(gx.any()) and not bool(gy.any())


def test_smaller_window_is_the_eleven_tap_kernel_with_zero_taps():
    x, y = R.content("uniform01", (1, 2, 13, 9), seed=5)
    for ws in (1, 3, 7):
        w = torch.zeros(11, 11, dtype=torch.float64)
        h = ws // 2
        w[5 - h:6 + h, 5 - h:6 + h] = R.window(ws)
        m_small, m_big = R.moments(x.double(), y.double(), R.window(ws)), R.moments(x.double(), y.double(), w)
        for a, b in zip(m_small, m_big):
            assert float((a - b).abs().max()) <= 1e-15


# -------------------------------------------------------------------------------------------------- host checks ---
NAMES = ("ssg_ssim_workspace_bytes", "ssg_ssim_grid_cap", "ssg_ssim_taps", "ssg_ssim_loss")
FAKE = ctypes.c_void_p(1 << 20)        # non-null, 16-byte aligned addresses that a refused call never touches
FAKE2 = ctypes.c_void_p(2 << 20)
FAKE3 = ctypes.c_void_p(3 << 20)
FAKE4 = ctypes.c_void_p(4 << 20)
FAKE5 = ctypes.c_void_p(5 << 20)


def _declaration(hdr, name):
    m = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
    assert m, name
    text = re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " "))
    return [a.strip() for a in text.split(",") if a.strip() != "void"]


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
    assert L.ssg_abi_version() == 6
    from ssl_amd import losses
    import importlib
    M = importlib.import_module("ssl_amd.losses.ssim")     # (the package attribute `ssim` is the function)
    for name in ("gaussian", "create_window", "ssim", "SSIMLoss"):
        assert getattr(losses, name) is getattr(M, name) and name in M.__all__


def test_taps_are_the_reference_taps_bit_for_bit(golden):
    from ssl_amd import _lib
    from ssl_amd.losses import create_window, gaussian
    L = _lib.lib()
    buf = (ctypes.c_float * 11)()
    for ws in (1, 3, 5, 7, 9, 11):
        assert L.ssg_ssim_taps(ws, buf) == 0
        t = torch.tensor(list(buf), dtype=torch.float32)
        h = ws // 2
        assert torch.equal(t[5 - h:6 + h], R.gaussian(ws)) and torch.equal(gaussian(ws, 1.5), R.gaussian(ws))
        assert not bool(t[:5 - h].any()) and not bool(t[6 + h:].any())
        assert torch.equal(create_window(ws, 3).double(), R.window(ws).expand(3, 1, ws, ws))
    for n in range(N_CASES):       # ... and the reference's recorded window is the table of those taps
        ws = int(golden[f"c{n}_ws"])
        assert torch.equal(torch.from_numpy(golden[f"c{n}_window"]), create_window(ws, 1)[0, 0])
    for ws in (0, -1, 2, 4, 12, 13):
        assert L.ssg_ssim_taps(ws, buf) == -1
    assert L.ssg_ssim_taps(11, None) == -1


def test_trip_shape_is_tied_to_the_grid_cap():
    """test_gpu_ssim.py's second-trip shape: more tiles than the cap, fewer than two grids -- raising the cap fails here
    instead of quietly returning that test to one trip."""
    from ssl_amd import _lib
    import test_gpu_ssim as tg
    L = _lib.lib()
    cap = L.ssg_ssim_grid_cap()
    B, C, H, W = tg.TRIP_SHAPE
    rows, cols = (lambda n: -(-n // tg.TH)), (lambda n: -(-n // tg.TW))
    tiles = C * rows(H) * cols(W)
    assert B == 1 and cap < tiles < 2 * cap
    B, C, H, W = tg.INTERIOR_TRIP_SHAPE
    tiles, per = C * rows(H) * cols(W), rows(H) * cols(W)
    assert B == 1 and cap < tiles < 2 * cap and per < cap                      # ... and a plane alone makes one trip
    assert (cap - 2 * per) // cols(W) + 1 < rows(H) - 1                        # interior tile rows lie on the second trip
    assert L.ssg_ssim_workspace_bytes(*tg.TRIP_SHAPE) == 8 * cap               # one double per workgroup: capped
    assert L.ssg_ssim_workspace_bytes(1, 1, tg.TH, tg.TW) == 256               # one tile, padded
    assert L.ssg_ssim_workspace_bytes(1, 1, tg.TH + 1, tg.TW) == 256           # two tiles
    assert L.ssg_ssim_workspace_bytes(2, 3, 40, 37) == 256                     # 2 x 6 doubles, padded
    assert L.ssg_ssim_workspace_bytes(3, 1, 4 * tg.TH, 3 * tg.TW + 1) == 512   # 3 x 16 doubles


def test_c_abi_refuses_before_any_launch():
    from ssl_amd import _lib
    L = _lib.lib()
    BAD, BIG, WS, ALIGN = -1, -2, -3, -5
    ok = (2, 3, 40, 37)
    nb = L.ssg_ssim_workspace_bytes(*ok)
    call = lambda x, y, shape, ws, g, s, w, n: L.ssg_ssim_loss(x, y, *shape, ws, g, s, w, n, None)   # noqa: E731
    assert call(None, FAKE2, ok, 11, FAKE3, FAKE4, FAKE5, nb) == BAD
    assert call(FAKE, None, ok, 11, FAKE3, FAKE4, FAKE5, nb) == BAD
    assert call(FAKE, FAKE2, ok, 11, FAKE3, None, FAKE5, nb) == BAD
    assert call(FAKE, FAKE2, ok, 11, FAKE3, FAKE4, None, nb) == BAD
    assert call(FAKE, FAKE2, ok, 11, FAKE, FAKE4, FAKE5, nb) == BAD            # the gradient over its input
    assert call(FAKE, FAKE2, ok, 11, FAKE2, FAKE4, FAKE5, nb) == BAD
    for shape in ((0, 3, 40, 37), (2, 0, 40, 37), (2, 3, 0, 37), (2, 3, 40, -1)):
        assert call(FAKE, FAKE2, shape, 11, FAKE3, FAKE4, FAKE5, nb) == BAD
        assert L.ssg_ssim_workspace_bytes(*shape) == 0
    for ws in (0, 4, 12, 13, -3):
        assert call(FAKE, FAKE2, ok, ws, FAKE3, FAKE4, FAKE5, nb) == BAD
    for big in ((4, 3, 16384, 16384), (65536, 1, 2, 2)):                       # 2^31 elements; more images than grid rows
        assert call(FAKE, FAKE2, big, 11, FAKE3, FAKE4, FAKE5, 1 << 30) == BIG
        assert L.ssg_ssim_workspace_bytes(*big) == 0
    assert call(FAKE, FAKE2, ok, 11, FAKE3, FAKE4, FAKE5, nb - 1) == WS
    assert call(FAKE, FAKE2, ok, 11, None, FAKE4, FAKE5, nb - 1) == WS         # the loss-only entry too
    assert call(FAKE, FAKE2, ok, 11, FAKE3, FAKE4, ctypes.c_void_p((5 << 20) + 8), nb) == ALIGN
    # two things wrong at once: the pointers, then the shape, then the window, then the workspace's size, then its alignment
    big, odd = (4, 3, 16384, 16384), ctypes.c_void_p((5 << 20) + 8)
    assert call(None, FAKE2, big, 11, FAKE3, FAKE4, FAKE5, 1 << 30) == BAD
    assert call(FAKE, FAKE2, big, 11, FAKE, FAKE4, FAKE5, 1 << 30) == BAD
    assert call(FAKE, FAKE2, big, 4, FAKE3, FAKE4, FAKE5, 0) == BIG
    assert call(FAKE, FAKE2, (0, 3, 40, 37), 4, FAKE3, FAKE4, odd, 0) == BAD
    assert call(FAKE, FAKE2, ok, 4, FAKE3, FAKE4, odd, nb - 1) == BAD
    assert call(FAKE, FAKE2, ok, 11, FAKE3, FAKE4, odd, nb - 1) == WS


def test_python_argument_errors_without_a_device():
    from ssl_amd.losses import SSIMLoss, ssim
    a = torch.zeros(1, 3, 8, 9)
    for ws in (4, 13):
        with pytest.raises(ValueError, match="odd window sizes up to 11"):
            SSIMLoss(window_size=ws)
    with pytest.raises(ValueError, match="positive integer"):
        SSIMLoss(window_size=0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ssim(a, a)
    crit = SSIMLoss(7, size_average=False)
    assert (crit.window_size, crit.size_average, crit.channel) == (7, False, 1)
    assert crit.window.shape == (1, 1, 7, 7) and crit.window.dtype == torch.float32
