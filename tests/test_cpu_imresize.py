"""What of the MATLAB-style bicubic imresize (ssl_amd/prep.py:imresize, ssl_amd/csrc/ssg_imresize.hip) can be checked
without a device: the fp64 restatement (tests/imresize_reference.py) against the reference's recorded float32 outputs
(tests/golden/f30_imresize*.npz, made by make_golden_imresize.py) within the bound derived in the restatement's header,
the library's host tables against the restatement's bit for bit, the integer restatement at dyadic scales, the tie
images of the GPU byte test, and the refusals the host decides."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import imresize_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_BADARG, E_TOOLARGE, E_IMAGESMALL = -1, -2, -4
# every (scale, antialiasing) of the fixture's list
MODES = [(s, True) for s in R.SCALES.values()] + [(1 / 2, False), (1 / 3, False)]


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(GOLDEN)


def lib_table(L, n, s, aa):
    """(status, first, weights) of ssg_imresize_table; the arrays keep their fill where the call is refused"""
    m = L.ssg_imresize_out_size(n, s)
    T = L.ssg_imresize_taps(s, int(aa))
    assert m > 0 and T > 0
    first = np.full(m, -77, np.int32)
    w = np.full((m, T), -77.0, np.float64)
    return L.ssg_imresize_table(n, m, s, int(aa), first.ctypes.data, w.ctypes.data), first, w


def min_side(s, aa):
    """the smallest n whose axis lies in the mirror domain, by the restatement"""
    for n in range(1, 200):
        try:
            R.axis_table(n, s, aa)
            return n
        except ValueError:
            pass
    raise AssertionError((s, aa))


def test_fixture_holds_the_cases_and_records_what_the_reference_refused(fixture):
    cases, skipped = fixture
    assert sorted(cases) == sorted(R.FIXTURE_CASE_TAGS) and len(cases) == 26
    # 1 / 4 without antialiasing on 64 x 48 needs no padding at the far end: the reference raises, this package computes
    assert len(skipped) == 1 and skipped[0].startswith("far@1_4@noaa: RuntimeError")
    R.resize_planes(np.zeros((64, 48)), 1 / 4, False)


def test_restatement_against_the_reference_within_the_derived_bound(fixture):
    """Per element.  With SSL_AMD_WRITE_PROFILES naming a folder, the share of the bound each case uses is written there
    (profiles/imresize_parity.txt is that output, followed by the GPU test's)."""
    lines = []
    for tag in R.FIXTURE_CASE_TAGS:
        x, s, aa, ref = fixture[0][tag]
        y = R.resize_planes(x, s, aa)
        assert y.shape == ref.shape, tag
        b = R.reference_bound(x, s, aa)
        diff = np.abs(ref.astype(np.float64) - y)
        share = float((diff / b["total"]).max())
        at = np.unravel_index(np.argmax(diff), diff.shape)
        lines.append(f"{tag:18s} max |ref - fp64| {diff.max():.3e}  bound there {b['total'][at]:.3e} (coordinate "
                     f"{b['coordinate'][at]:.2e}, weights {b['weights'][at]:.2e}, dot {b['dot'][at]:.2e})  "
                     f"largest share of the bound {share:.3f}")
        print(lines[-1])
        assert share <= 1.0, lines[-1]
    out = os.environ.get("SSL_AMD_WRITE_PROFILES")
    if out:
        with open(os.path.join(out, "imresize_parity_cpu.txt"), "w") as f:
            f.write("reference (float32 Python) against the fp64 restatement, per fixture case "
                    "(tests/test_cpu_imresize.py)\n" + "\n".join(lines) + "\n")


def test_bound_grows_with_the_side_only_through_the_coordinate(fixture):
    """at 0.7 the coordinate term dominates on 300 x 255 and is the only one that grew from 19 x 23"""
    small = R.reference_bound(fixture[0]["small@0.7@aa"][0], 0.7)
    big = R.reference_bound(fixture[0]["big@0.7@aa"][0], 0.7)
    assert big["coordinate"].max() > 5 * small["coordinate"].max()
    assert big["coordinate"].max() > big["weights"].max() + big["dot"].max()
    assert big["dot"].max() < 2 * small["dot"].max()


@pytest.mark.parametrize("s,aa", MODES)
def test_library_tables_equal_the_restatement_bit_for_bit(L, s, aa):
    sides = set(range(1, 41)) | {h for hw in R.FIXTURE_INPUTS.values() for h in hw}
    accepted = 0
    for n in sorted(sides):
        status, first, w = lib_table(L, n, s, aa)
        try:
            rf, rw = R.axis_table(n, s, aa)
        except ValueError:
            assert status == E_IMAGESMALL, (n, s, aa)
            assert (first == -77).all() and (w == -77.0).all()
            continue
        accepted += 1
        assert status == 0, (n, s, aa)
        assert np.array_equal(first, rf), (n, s, aa)
        assert w.shape == rw.shape and np.array_equal(w.view(np.uint64), rw.view(np.uint64)), (n, s, aa)
        assert L.ssg_imresize_taps(s, int(aa)) == R.taps(s, aa) == w.shape[1]
    assert accepted >= 30


def test_out_size_is_the_host_s_ceil_of_the_double_product(L):
    # the product is formed in doubles and not repaired: 50 * 1.1 is 55.00000000000001 and gives 56, as in the
    # reference; 30 * 0.1 is exactly 3.0 in doubles and gives 3
    assert L.ssg_imresize_out_size(50, 1.1) == 56 == math.ceil(50 * 1.1)
    assert L.ssg_imresize_out_size(30, 0.1) == 3 == math.ceil(30 * 0.1)
    for s, _ in MODES:
        for n in list(range(1, 61)) + [255, 300, 1356, 2040]:
            assert L.ssg_imresize_out_size(n, s) == math.ceil(n * s) == R.out_size(n, s), (n, s)
    assert L.ssg_imresize_out_size(0, 0.5) == E_BADARG
    assert L.ssg_imresize_out_size(2 ** 30, 4.0) == E_TOOLARGE


@pytest.mark.parametrize("s", [1 / 8, 1 / 4, 1 / 2, 2.0, 4.0, 8.0])
def test_integer_restatement_equals_the_fp64_one_at_dyadic_scales(s):
    rng = np.random.default_rng(int(s * 64))
    for shape in ((40, 56), (33, 47, 3), (2, 24, 31, 3)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        b, y = R.imresize_bytes(a, s)
        assert np.array_equal(R.imresize_bytes_int(a, s), b), (s, shape)
        p = a if a.ndim == 2 else np.moveaxis(a, -1, -3)
        num, Q = R.resize_planes_int(p, s)
        yi = num.astype(np.float64) / float(2 ** Q)
        assert np.array_equal(yi if a.ndim == 2 else np.moveaxis(yi, -3, -1), y)      # the fp64 sums are exact


def test_integer_restatement_without_antialiasing():
    a = np.random.default_rng(5).integers(0, 256, (36, 52), dtype=np.uint8)
    assert np.array_equal(R.imresize_bytes_int(a, 0.5, False), R.imresize_bytes(a, 0.5, False)[0])


@pytest.mark.parametrize("s", [1 / 2, 1 / 4])
def test_tie_image_has_exact_ties(s):
    a, n = R.tie_image(s)
    assert n >= 32 and a.dtype == np.uint8 and a.shape == (64, 64)
    num, Q = R.resize_planes_int(a, s)
    ties = R.int_ties(num, Q)
    assert int(ties.sum()) == n
    y = R.resize_planes(a, s)
    assert (y[ties] - np.floor(y[ties]) == 0.5).all()
    # MATLAB's round-half-away: every tie goes up
    assert np.array_equal(R.imresize_bytes_int(a, s)[ties], (np.floor(y[ties]) + 1).astype(np.uint8))


def test_clear_of_ties_condition_can_be_met():
    """the inputs of the GPU byte test at non-dyadic scales: no y within 1e-9 of k + 1 / 2"""
    for s in (1 / 3, 0.7, 1.5, 3):
        a = R.clear_of_ties(s, (21, 34, 3), seed=1)
        _, y = R.imresize_bytes(a, s)
        assert np.abs(y - np.floor(y) - 0.5).min() > 1e-9


@pytest.mark.parametrize("s,aa", MODES)
def test_mirror_domain_smallest_side(L, s, aa):
    n = min_side(s, aa)
    assert lib_table(L, n, s, aa)[0] == 0
    if n > 1:
        assert lib_table(L, n - 1, s, aa)[0] == E_IMAGESMALL
    # a larger side stays accepted
    assert lib_table(L, n + 7, s, aa)[0] == 0


def test_c_abi_refusals_are_decided_before_any_launch(L):
    """No device is present here: every status below is returned before the library touches the HIP runtime."""
    p, q, t = 4096, 8192, 12288          # never dereferenced
    U8, F32 = 1, 0

    def call(src=p, kind=U8, B=1, C=3, H=40, W=50, s=0.5, aa=1, yf=t, yw=t, xf=t, xw=t, out_kind=1, out=q):
        return L.ssg_imresize(src, kind, B, C, H, W, s, aa, yf, yw, xf, xw, out_kind, out, None)

    for kw in (dict(src=None), dict(out=None), dict(out=p), dict(yf=None), dict(yw=None), dict(xf=None), dict(xw=None)):
        assert call(**kw) == E_BADARG, kw
    for C in (0, 2, 4):
        assert call(C=C) == E_BADARG
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(kind=2), dict(kind=-1), dict(out_kind=3), dict(out_kind=0),
               dict(kind=F32, out_kind=1), dict(kind=F32, out_kind=2)):
        assert call(**kw) == E_BADARG, kw
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert call(s=s) == E_BADARG, s
        assert L.ssg_imresize_taps(s, 1) == E_BADARG and L.ssg_imresize_out_size(10, s) == E_BADARG
    # more than 32 taps: antialiased scales below 1 / 8; without antialiasing the same scale has four
    assert call(s=0.12, H=100, W=100) == E_TOOLARGE and L.ssg_imresize_taps(0.12, 1) == E_TOOLARGE
    assert L.ssg_imresize_taps(0.12, 0) == 4 and L.ssg_imresize_taps(1 / 8, 1) == 32 and L.ssg_imresize_taps(7.5, 1) == 4
    # 2^31 elements
    assert call(B=2, C=1, H=32768, W=32768) == E_TOOLARGE
    assert call(kind=F32, out_kind=0, B=1, C=8, H=8192, W=8192, s=2.0) == E_TOOLARGE
    # the mirror domain
    assert call(H=3, W=50, s=1 / 8) == E_IMAGESMALL and call(H=50, W=1, s=4.0) == E_IMAGESMALL


def test_tile_list(L):
    tiles = (ctypes.c_int * 16)()
    chosen = ctypes.c_int(-5)
    n = L.ssg_imresize_tiles(0.25, 1, tiles, 8, ctypes.byref(chosen))
    assert 1 <= n <= 8 and 0 <= chosen.value < n
    shapes = [(tiles[2 * i], tiles[2 * i + 1]) for i in range(n)]
    assert all(th >= 8 and tw >= 8 for th, tw in shapes) and len(set(shapes)) == n
    for s, aa in MODES + [(8.0, True), (1 / 16, False), (1 / 1000, False)]:
        assert L.ssg_imresize_tiles(s, int(aa), None, 0, ctypes.byref(chosen)) == n and 0 <= chosen.value < n, (s, aa)
    assert L.ssg_imresize_tiles(4.0, 1, None, 0, ctypes.byref(chosen)) == n and chosen.value == 0   # a few pixels of footprint
    assert L.ssg_imresize_tiles(0.01, 1, None, 0, ctypes.byref(chosen)) == n and chosen.value == -1
    assert L.ssg_imresize_tiles(0.5, 1, None, 4, None) == E_BADARG


def test_python_refusals_without_a_device(L):
    from ssl_amd import prep
    assert prep.imresize_np is prep.imresize
    with pytest.raises(RuntimeError, match="no CPU path"):
        prep.imresize(torch.zeros(3, 16, 16), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prep.imresize(torch.zeros(16, 16, 3, dtype=torch.uint8), 0.5)
    g = torch.zeros(16, 16, 3, dtype=torch.uint8)
    for s in (0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            prep.imresize(g, s)
    with pytest.raises(NotImplementedError, match="32 taps"):
        prep.imresize(g, 0.1)
    with pytest.raises(ValueError, match="1 .'L'. or 3"):
        prep.imresize(torch.zeros(16, 16, 2, dtype=torch.uint8), 0.5)
    with pytest.raises(ValueError, match="mirror"):
        prep.imresize(torch.zeros(3, 16, 3, dtype=torch.uint8), 1 / 8)
    with pytest.raises(ValueError, match="out"):
        prep.imresize(g, 0.5, out="signed")
    with pytest.raises(ValueError, match="out"):
        prep.imresize(torch.zeros(3, 16, 16), 0.5, out="unit")
    with pytest.raises(TypeError):
        prep.imresize(np.zeros((16, 16, 3), np.uint8), 0.5)
    with pytest.raises(ValueError, match="modulo"):
        prep.modcrop(np.zeros((16, 16)), 0)


def test_modcrop_layouts():
    from ssl_amd import prep
    assert prep.modcrop(np.zeros((19, 23)), 4).shape == (16, 20)
    assert prep.modcrop(np.zeros((19, 23, 3)), 12).shape == (12, 12, 3)
    assert prep.modcrop(torch.zeros(19, 23, 3, dtype=torch.uint8), 4).shape == (16, 20, 3)
    assert prep.modcrop(torch.zeros(2, 19, 23, 3, dtype=torch.uint8), 4).shape == (2, 16, 20, 3)
    assert prep.modcrop(torch.zeros(19, 23, dtype=torch.uint8), 5).shape == (15, 20)
    assert prep.modcrop(torch.zeros(3, 19, 23), 4).shape == (3, 16, 20)
    assert prep.modcrop(torch.zeros(2, 3, 19, 23), 4).shape == (2, 3, 16, 20)
    a = np.arange(19 * 23).reshape(19, 23)
    assert np.array_equal(prep.modcrop(a, 4), a[:16, :20]) and np.array_equal(R.modcrop(a, 4), a[:16, :20])
    with pytest.raises(ValueError, match="leaves none"):
        prep.modcrop(np.zeros((3, 23)), 4)


def test_abi_version_and_exports(L):
    from ssl_amd import _lib
    assert L.ssg_abi_version() == 6
    header = open(_lib.HEADER).read()
    for name in ("ssg_imresize", "ssg_imresize_out_size", "ssg_imresize_taps", "ssg_imresize_table", "ssg_imresize_tiles"):
        assert hasattr(L, name) and name in _lib.PROTOTYPES and f"int {name}(" in header
