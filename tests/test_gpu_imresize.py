"""ssl_amd.prep.imresize (ssl_amd/csrc/ssg_imresize.hip) on the GPU against the fp64 restatement
(tests/imresize_reference.py) and the reference's recorded outputs (tests/golden/f30_imresize*.npz).

Float path: within one unit in the last place of fp32 of the restatement's fp64 value (the kernel sums in the
restatement's order, so it is in fact the same bits; the unit is what another order could move at a rounding boundary),
and within the derived bound of the reference's float32 output, to which one more fp32 rounding is added for the kernel's
own.  Byte path: every byte equal, against the integer restatement at dyadic scales (ties included) and against the fp64
restatement's bytes where no sum lies within 1e-9 of a tie.  Shapes: the smallest side the mirror allows, one output
more than every tile of the kernel's list, the fewest outputs the domain allows along one axis against 40 along the
other.  The grid is not capped (one workgroup per tile and plane), so there is no cap to pass."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import imresize_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SCRIPT = os.path.join(os.path.dirname(HERE), "scripts", "generate_bicubic_img.py")
MODES = [(s, True) for s in R.SCALES.values()] + [(1 / 2, False), (1 / 3, False)]
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def fixture():
    if "fixture" not in _cache:
        cases, _ = R.load_fixture(GOLDEN)
        _cache["fixture"] = {t: c + (R.resize_planes(c[0], c[1], c[2]),) for t, c in cases.items()}
    return _cache["fixture"]


def within_one_ulp(got, y64):
    """got float32 against the fp64 value: |got - y| <= the spacing of fp32 at |y|; returns the number of elements that
    are not the correctly rounded value"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == y64.shape, (got.dtype, got.shape, y64.shape)
    ulp = np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - y64) <= ulp).all(), float(np.abs(got - y64).max())
    return int((got != y64.astype(np.float32)).sum())


def side_for(m, s):
    """the smallest input side with at least m outputs (an upscale does not reach every count)"""
    n = 1
    while R.out_size(n, s) < m:
        n += 1
    return n


def min_side(s, aa):
    for n in range(1, 200):
        try:
            R.axis_table(n, s, aa)
            return n
        except ValueError:
            pass
    raise AssertionError((s, aa))


def tiles_of(s, aa):
    from ssl_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int * 16)()
    chosen = ctypes.c_int(-1)
    n = L.ssg_imresize_tiles(s, int(aa), buf, 8, ctypes.byref(chosen))
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)], chosen.value


@pytest.mark.gpu
def test_fixture_cases_on_the_float_path(dev):
    from ssl_amd import prep
    lines, worst_ulp, worst_share = [], 0, 0.0
    for tag in R.FIXTURE_CASE_TAGS:
        x, s, aa, ref, y64 = fixture()[tag]
        got = prep.imresize(torch.from_numpy(x).to(dev), s, aa).cpu().numpy()
        off = within_one_ulp(got, y64)
        b = R.reference_bound(x, s, aa)["total"] + R.EPS32 * np.abs(y64)
        diff = np.abs(got.astype(np.float64) - ref)
        share = float((diff / b).max())
        lines.append(f"{tag:18s} not the rounded fp64 value: {off} of {got.size}  max |gpu - fp64| "
                     f"{np.abs(got - y64).max():.3e}  max |gpu - ref| {diff.max():.3e}  largest share of the bound {share:.3f}")
        print(lines[-1])
        assert share <= 1.0, lines[-1]
        worst_ulp, worst_share = max(worst_ulp, off), max(worst_share, share)
    out = os.environ.get("SSL_AMD_WRITE_PROFILES")
    if out:
        with open(os.path.join(out, "imresize_parity_gpu.txt"), "w") as f:
            f.write("the kernel's float path against the fp64 restatement and the reference's float32 outputs, per "
                    "fixture case (tests/test_gpu_imresize.py)\n" + "\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("s,aa", MODES + [(8.0, True), (0.26, False), (1 / 4, False), (1 / 16, False), (1 / 40, False)])
def test_generated_shapes_at_every_scale(dev, s, aa):
    """(without antialiasing 0.26 is the last scale of the list whose footprint is contiguous, 1 / 4 and below are compact)"""
    from ssl_amd import prep
    n1 = min_side(s, aa)
    n40 = side_for(40, s)
    tiles, chosen = tiles_of(s, aa)
    assert 0 <= chosen < len(tiles)
    shapes = [(n1, n1), (n1, n40), (n40, n1)] + [(side_for(th + 1, s), side_for(tw + 1, s)) for th, tw in tiles]
    rng = np.random.default_rng(int(s * 1000) + aa)
    for H, W in shapes:
        H, W = max(H, n1), max(W, n1)
        x = rng.standard_normal((2, H, W)).astype(np.float32)
        got = prep.imresize(torch.from_numpy(x).to(dev), s, aa).cpu().numpy()
        within_one_ulp(got, R.resize_planes(x, s, aa))
    # the smallest side mirrors across the whole image: its first output reads tap -n1 or its last tap 2 n1 - 1
    f, w = R.axis_table(n1, s, aa)
    assert f[0] < 0 or f[-1] + w.shape[1] > n1
    if n1 > 1:
        with pytest.raises(ValueError, match="mirror"):
            prep.imresize(torch.zeros(1, n1 - 1, n40, device=dev), s, aa)


BYTE_SHAPES = ((2, 45, 70, 3), (50, 41), (37, 64, 1))


def byte_cases():
    """[(input bytes, scale, expected bytes)]: dyadic scales against the integer restatement on random bytes and on the
    tie images, the other scales against the fp64 restatement's bytes on inputs that are clear of ties"""
    if "bytes" in _cache:
        return _cache["bytes"]
    out = []
    ties = {s: R.tie_image(s) for s in (1 / 2, 1 / 4)}
    for s in (1 / 8, 1 / 4, 1 / 2, 2.0, 4.0):
        rng = np.random.default_rng(int(s * 8))
        for shape in BYTE_SHAPES:
            a = rng.integers(0, 256, shape, dtype=np.uint8)
            out.append((a, s, R.imresize_bytes_int(a, s)))
        for ts, (a, n) in ties.items():
            assert n >= 32
            out.append((a, s, R.imresize_bytes_int(a, s)))
    for s in (1 / 3, 0.7, 1.5, 3):
        for i, shape in enumerate(BYTE_SHAPES):
            a = R.clear_of_ties(s, shape, seed=i)                 # asserts the 1e-9 margin
            out.append((a, s, R.imresize_bytes(a, s)[0]))
    _cache["bytes"] = out
    return out


@pytest.mark.gpu
def test_byte_path_every_byte(dev):
    from ssl_amd import prep
    for a, s, want in byte_cases():
        got = prep.imresize(torch.from_numpy(a).to(dev), s)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (a.shape, s)
        assert np.array_equal(got.cpu().numpy(), want), (a.shape, s, int((got.cpu().numpy() != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1 / 2, 1 / 4])
def test_ties_round_up_on_the_gpu(dev, s):
    from ssl_amd import prep
    a, n = R.tie_image(s)
    num, Q = R.resize_planes_int(a, s)
    ties = R.int_ties(num, Q)
    assert int(ties.sum()) == n >= 32
    got = prep.imresize(torch.from_numpy(a).to(dev), s).cpu().numpy()
    assert np.array_equal(got[ties].astype(np.int64), (num[ties] >> Q) + 1)
    assert np.array_equal(got, R.int_to_bytes(num, Q))


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1 / 2, 2.0])
def test_saturation_hits_both_clamps(dev, s):
    from ssl_amd import prep
    a = (np.kron(np.indices((12, 15)).sum(0) % 2, np.ones((4, 4))) * 255).astype(np.uint8)      # 4 x 4 blocks of 0 / 255
    num, Q = R.resize_planes_int(a, s)
    assert num.min() < -(1 << Q) and num.max() > (256 << Q)       # below -1 and above 256 before the clamp
    got = prep.imresize(torch.from_numpy(a).to(dev), s).cpu().numpy()
    assert np.array_equal(got, R.int_to_bytes(num, Q))
    assert (got[num < 0] == 0).all() and (got[num > (255 << Q)] == 255).all()


@pytest.mark.gpu
def test_layouts_batches_and_repeats(dev):
    from ssl_amd import prep
    rng = np.random.default_rng(8)
    s = 0.7
    xb = torch.from_numpy(rng.random((3, 2, 41, 53), dtype=np.float32)).to(dev)
    yb = prep.imresize(xb, s)
    assert yb.dtype == torch.float32 and tuple(yb.shape) == (3, 2, 29, 38)
    assert torch.equal(prep.imresize(xb, s), yb)                                           # a repeat
    for b in range(3):
        assert torch.equal(prep.imresize(xb[b], s), yb[b])                                 # (C,H,W)
        assert torch.equal(prep.imresize(xb[b, 1], s), yb[b, 1])                           # (H,W)
    # numpy (H,W,C) and (H,W) go to the GPU and back
    hwc = xb[0].permute(1, 2, 0).cpu().numpy()
    out = prep.imresize_np(hwc, s)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (29, 38, 2)
    assert np.array_equal(out, yb[0].permute(1, 2, 0).cpu().numpy())
    assert np.array_equal(prep.imresize(hwc[:, :, 0].astype(np.float64), s), yb[0, 0].cpu().numpy())
    # a view that is not contiguous, and the other float types through their float32 cast
    wide = torch.from_numpy(rng.random((2, 41, 106), dtype=np.float32)).to(dev)
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and torch.equal(prep.imresize(view, s), prep.imresize(view.contiguous(), s))
    assert torch.equal(prep.imresize(xb.double(), s), yb)
    half = xb.half()
    assert torch.equal(prep.imresize(half, s), prep.imresize(half.float(), s))
    # bytes: a batch against its images, (H,W,C) against (H,W) planes, 'unit'
    ab = torch.from_numpy(rng.integers(0, 256, (3, 33, 47, 3), dtype=np.uint8)).to(dev)
    for scale in (1 / 4, 1 / 3, 3):
        ob = prep.imresize(ab, scale)
        assert torch.equal(prep.imresize(ab, scale), ob)
        for b in range(3):
            assert torch.equal(prep.imresize(ab[b], scale), ob[b])
            for c in range(3):
                assert torch.equal(prep.imresize(ab[b, :, :, c], scale), ob[b, :, :, c])   # a strided (H,W) view
        unit = prep.imresize(ab, scale, out='unit')
        assert unit.dtype == torch.float32 and tuple(unit.shape) == (3, 3) + tuple(ob.shape[1:3])
        want = np.moveaxis(ob.cpu().numpy(), -1, 1).astype(np.float32) / np.float32(255)   # (numpy divides; torch on the
        assert np.array_equal(unit.cpu().numpy(), want)                                   # GPU multiplies by 1 / 255)
        assert torch.equal(prep.imresize(ab, scale, out='uint8'), ob)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prep.imresize(ab.cpu(), 0.5)


def write_pngs(folder):
    from PIL import Image
    rng = np.random.default_rng(77)
    src = {"a": rng.integers(0, 256, (37, 50, 3), dtype=np.uint8), "b": rng.integers(0, 256, (64, 50), dtype=np.uint8),
           "c": rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)}
    os.makedirs(folder)
    for name, a in src.items():
        Image.fromarray(a).save(os.path.join(folder, name + "_src.png"))
    return src


def load_script():
    spec = importlib.util.spec_from_file_location("generate_bicubic_img", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_modcrop_and_the_script_end_to_end(dev, tmp_path):
    from PIL import Image
    from ssl_amd import prep
    src = write_pngs(str(tmp_path / "in"))
    script = load_script()
    mod_d, lr_d, bic_d, dbl_d = (str(tmp_path / n) for n in ("GTmod12", "LRbicx4", "bic", "bic_double"))
    assert script.main(["--input", str(tmp_path / "in"), "--save-mod", mod_d, "--save-lr", lr_d, "--save-bic", bic_d,
                        "--mod-scale", "12", "--up-scale", "4"]) == 0
    assert script.main(["--input", str(tmp_path / "in"), "--save-bic", dbl_d, "--mod-scale", "12", "--up-scale", "4",
                        "--bic-from-double"]) == 0
    names = sorted(n + "_src.png" for n in src)
    for d in (mod_d, lr_d, bic_d, dbl_d):
        assert sorted(os.listdir(d)) == names
    for name, a in src.items():
        read = lambda d: np.array(Image.open(os.path.join(d, name + "_src.png")))      # noqa: E731
        gt = R.modcrop(a, 12)
        assert gt.shape[0] % 12 == 0 and gt.shape[1] % 12 == 0 and gt.shape[0] == a.shape[0] - a.shape[0] % 12
        assert np.array_equal(read(mod_d), gt)
        assert np.array_equal(prep.modcrop(torch.from_numpy(a).to(dev), 12).cpu().numpy(), gt)
        lr = R.imresize_bytes_int(gt, 1 / 4)
        assert lr.shape[:2] == (gt.shape[0] // 4, gt.shape[1] // 4)
        assert np.array_equal(read(lr_d), lr)
        assert np.array_equal(read(bic_d), R.imresize_bytes_int(lr, 4.0))
        planes = gt[None] if gt.ndim == 2 else np.moveaxis(gt, -1, 0)
        # the LR kept as float32 of its fp64 value, the upsample rounded to float32 and then to bytes
        up = R.to_bytes(R.imresize_float(R.imresize_float(planes.astype(np.float32), 1 / 4), 4.0).astype(np.float64))
        assert np.array_equal(read(dbl_d), up[0] if gt.ndim == 2 else np.moveaxis(up, 0, -1))
    (tmp_path / "bad").mkdir()
    Image.fromarray(src["a"]).convert("RGBA").save(str(tmp_path / "bad" / "x.png"))
    with pytest.raises(NotImplementedError, match="RGBA"):
        script.main(["--input", str(tmp_path / "bad"), "--save-lr", str(tmp_path / "bad_lr")])


def poison_cases():
    """What tests/test_gpu_imresize_poison.py runs on both builds: float cases that take every tile of the list and
    4, 8, 12, 14 and 32 taps, contiguous and compact footprints, and the byte cases above; a list of GPU tensors."""
    from ssl_amd import prep
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(99)
    out = []
    for s, aa, shape in ((4.0, True, (2, 12, 19)), (1.5, True, (2, 40, 51)), (1 / 2, True, (2, 70, 133)),
                         (1 / 3, True, (2, 55, 100)), (0.3, True, (1, 61, 120)), (1 / 8, True, (2, 80, 140)),
                         (1 / 2, False, (2, 70, 133)), (1 / 16, False, (1, 150, 290)), (1 / 40, False, (1, 700, 1400))):
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
        out.append(prep.imresize(x, s, aa))
    for a, s, _ in byte_cases():
        out.append(prep.imresize(torch.from_numpy(a).to(dev), s))
    out.append(prep.imresize(torch.from_numpy(byte_cases()[0][0]).to(dev), 1 / 4, out='unit'))
    return out
