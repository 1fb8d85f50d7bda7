"""What of the Pillow-exact resize and the dataset preparation (ssl_amd/prep.py, ssl_amd/csrc/ssg_resample.hip) can be
checked without a device: the numpy restatement (tests/pil_resize_reference.py) against Pillow itself, the library's host
tables against the restatement's, the multiscale rules against what the two reference scripts wrote
(tests/golden/f29_prep.npz, made by make_golden_prep.py), the sub-image grid against hand-derived values, and the
argument checks.  Exact equality throughout."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pil_resize_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f29_prep.npz")
SHORTEST_EDGE = 24                       # what make_golden_prep.py ran both scripts with
# (H, W) -> (h, w)
SHAPES = [((97, 131), (72, 98)), ((96, 130), (32, 43)), ((50, 50), (120, 77)), ((70, 90), (64, 64)),
          ((40, 50), (40, 32)), ((19, 7), (6, 2)), ((5, 300), (1, 100))]
E_BADARG, E_TOOLARGE = -1, -2


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", list(R.FILTERS))
def test_restatement_equals_pillow(name):
    from PIL import Image
    rng = np.random.default_rng(R.FILTERS[name])
    for (H, W), (h, w) in SHAPES:
        for c in (1, 3):
            a = rng.integers(0, 256, (H, W, c), dtype=np.uint8)
            im = Image.fromarray(a[..., 0] if c == 1 else a)
            assert im.mode == ('L' if c == 1 else 'RGB')
            want = np.array(im.resize((w, h), resample=R.FILTERS[name])).reshape(h, w, c)
            assert np.array_equal(R.resize(a, (w, h), name), want), (name, H, W, h, w, c)


@pytest.mark.parametrize("kind", ["const255", "checker", "blocks"])
def test_restatement_equals_pillow_on_clipping_content(kind):
    """4 x 4 blocks of 0 / 255 ring below 0 and above 255 before the clip; the flat image must stay 255."""
    from PIL import Image
    a = R.content(kind, 40, 52, 3, seed=1)
    for size in ((39, 30), (17, 13), (88, 68), (52, 30), (39, 40)):
        want = np.array(Image.fromarray(a).resize(size, resample=Image.LANCZOS))
        assert np.array_equal(R.resize(a, size), want), (kind, size)
    if kind == "blocks":
        bounds, coef = R.table(52, 39, 'lanczos')
        acc = np.stack([(a[:, b:b + n].astype(np.int64) * coef[x, :n, None]).sum(1) + (1 << 21)
                        for x, (b, n) in enumerate(bounds)], 1) >> 22
        assert (acc < 0).mean() > 0.05 and (acc > 255).mean() > 0.05


@pytest.mark.parametrize("name", list(R.FILTERS))
def test_library_tables_equal_the_restatement(L, name):
    """ssg_resample_ksize / ssg_resample_table: host functions (fp64, the C library's sin / cos), no device."""
    f = R.FILTERS[name]
    for (H, W), (h, w) in SHAPES:
        for insz, outsz in ((H, h), (W, w)):
            bounds, coef = R.table(insz, outsz, name)
            ks = L.ssg_resample_ksize(insz, outsz, f)
            assert ks == coef.shape[1] == R.ksize(insz, outsz, name)
            b = np.full((outsz, 2), -9, np.int32)
            k = np.full((outsz, ks), -9, np.int32)
            assert L.ssg_resample_table(insz, outsz, f, b.ctypes.data, k.ctypes.data) == 0
            assert np.array_equal(b, bounds) and np.array_equal(k, coef), (name, insz, outsz)
            assert bool((np.diff(b[:, 0]) >= 0).all())                  # xmin never decreases
            assert int(np.abs(k).max()) < 2 ** 23                       # a signed 24-bit operand


def test_prep_host_table_is_the_library_s(L):
    from ssl_amd import prep
    for name in R.FILTERS:
        b, k = prep.host_table(131, 98, prep.FILTERS[name])
        rb, rk = R.table(131, 98, name)
        assert np.array_equal(b, rb) and np.array_equal(k, rk)
    assert prep.FILTERS == R.FILTERS


def test_tile_and_limit(L):
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert L.ssg_resample_tile(ctypes.byref(th), ctypes.byref(tw)) == 0
    assert th.value >= 8 and tw.value >= 8 and th.value % 8 == 0 and tw.value % 8 == 0
    assert L.ssg_resample_tile(None, ctypes.byref(tw)) == E_BADARG
    assert L.ssg_resample_max_ratio() >= 8


def test_c_abi_argument_checks_are_decided_before_any_launch(L):
    """No device is present here: every status below is returned before the library touches the HIP runtime."""
    p, q, t = 4096, 8192, 12288          # never dereferenced

    def call(src=p, B=1, C=3, Hin=40, Win=50, Hout=30, Wout=20, f=1, xb=t, xk=t, yb=t, yk=t, kind=0, out=q):
        return L.ssg_resample(src, B, C, Hin, Win, Hout, Wout, f, xb, xk, yb, yk, kind, out, None)

    assert call(src=None) == E_BADARG and call(out=None) == E_BADARG and call(out=p) == E_BADARG
    assert call(xb=None) == E_BADARG and call(xk=None) == E_BADARG
    assert call(yb=None) == E_BADARG and call(yk=None) == E_BADARG
    for C in (0, 2, 4):
        assert call(C=C) == E_BADARG
    for kw in (dict(B=0), dict(Hin=0), dict(Win=0), dict(Hout=0), dict(Wout=0), dict(f=0), dict(f=6), dict(f=-1),
               dict(kind=3), dict(kind=-1)):
        assert call(**kw) == E_BADARG, kw
    assert call(B=2, Hin=32768, Win=32768, Hout=8192, Wout=8192, C=1) == E_TOOLARGE       # 2^31 input elements
    assert call(B=1, Hin=8192, Win=8192, Hout=32768, Wout=65536, C=1) == E_TOOLARGE       # 2^31 output elements
    r = L.ssg_resample_max_ratio()
    assert call(Win=r * 20 + 1) == E_TOOLARGE and call(Hin=r * 30 + 1) == E_TOOLARGE
    assert L.ssg_resample_ksize(0, 5, 1) == E_BADARG and L.ssg_resample_ksize(5, 0, 1) == E_BADARG
    assert L.ssg_resample_ksize(5, 5, 0) == E_BADARG and L.ssg_resample_ksize(5, 5, 6) == E_BADARG
    assert L.ssg_resample_table(5, 5, 1, None, t) == E_BADARG and L.ssg_resample_table(5, 5, 1, t, None) == E_BADARG


def test_python_argument_checks_are_decided_before_any_launch():
    from ssl_amd import prep
    img = torch.zeros((40, 50, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        prep.resize(img.float(), (20, 30))
    with pytest.raises(TypeError):
        prep.resize(img.numpy(), (20, 30))
    for bad in (torch.zeros((40, 50, 2), dtype=torch.uint8), torch.zeros((40,), dtype=torch.uint8),
                torch.zeros((1, 2, 40, 50, 3), dtype=torch.uint8), torch.zeros((0, 50, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            prep.resize(bad, (20, 30))
    for size in ((0, 30), (20, 0), (-1, 5), (20.0, 30), 20, (1, 2, 3)):
        with pytest.raises(ValueError):
            prep.resize(img, size)
    for resample in ('nearest', 0, 6, None, True):
        with pytest.raises(ValueError):
            prep.resize(img, (20, 30), resample)
    with pytest.raises(ValueError):
        prep.resize(img, (20, 30), out='float')
    with pytest.raises(NotImplementedError, match="<= 8"):
        prep.resize(img, (6, 30))                            # 50 -> 6
    with pytest.raises(RuntimeError, match="GPU"):
        prep.resize(img, (20, 30))                           # everything in order but the device
    with pytest.raises(ValueError, match="multiple of 32"):
        prep.load_img(np.zeros((31, 64, 3), np.uint8))
    with pytest.raises(TypeError):
        prep.load_img(np.zeros((64, 64), np.uint8))


def test_modes_other_than_l_and_rgb_are_refused_by_name():
    from PIL import Image
    from ssl_amd import prep
    for mode in ('RGBA', 'P', 'I;16', 'F', 'CMYK', '1'):
        with pytest.raises(NotImplementedError, match=mode.replace(';', '.')):
            prep.from_pil(Image.new(mode, (8, 8)))


@pytest.mark.parametrize("variant", ["gan", "dm"])
def test_multiscale_plan_reproduces_the_reference_scripts(golden, variant):
    from ssl_amd import prep
    sources = sorted(k[3:] for k in golden if k.startswith("in_"))
    assert len(sources) == 12
    want_names = sorted(k[len(variant) + 1:] for k in golden if k.startswith(variant + "_") and not k.endswith("_kept"))
    got_names, kept = [], []
    for name in sources:
        a = golden[f"in_{name}"]
        plan, keep = prep.multiscale_plan(a.shape[1], a.shape[0], variant, SHORTEST_EDGE)
        if keep:
            kept.append(name)
        for suffix, (w, h) in plan:
            got_names.append(name + suffix)
            rec = golden[f"{variant}_{name}{suffix}"]
            assert rec.shape[:2] == (h, w) and rec.shape[2:] == a.shape[2:], (name, suffix)
            # and the recorded pixels are the restatement's (the scripts call Pillow's LANCZOS)
            assert np.array_equal(R.resize(a, (w, h)), rec), (name, suffix)
    assert sorted(got_names) == want_names
    assert kept == list(golden[f"{variant}_kept"])
    assert os.path.getsize(GOLDEN) < 300 * 1000


def test_multiscale_plan_rules():
    from ssl_amd import prep
    plan, keep = prep.multiscale_plan(2040, 1356, 'gan')
    assert plan == [("T0", (1530, 1017)), ("T1", (1224, 813)), ("S", (770, 512))] and keep    # 452 < 512: no T2
    plan, keep = prep.multiscale_plan(2040, 1356, 'dm')
    assert plan == [("T0", (1530, 1017)), ("T1", (1224, 813)), ("T2", (680, 452)), ("T3", (770, 512))] and keep
    plan, keep = prep.multiscale_plan(400, 900, 'gan')
    assert plan == [("S", (512, 1152))] and not keep
    with pytest.raises(ValueError):
        prep.multiscale_plan(2, 50, 'dm')                    # int(2 / 3) = 0: Pillow raises too
    with pytest.raises(ValueError):
        prep.multiscale_plan(50, 50, 'esrgan')


def test_subimage_grid_and_names():
    """extract_subimages.py:82-99 by hand: arange(0, n - crop + 1, step), and n - crop appended when more than
    thresh_size pixels are left over."""
    from ssl_amd import prep
    assert prep.subimage_grid(1356, 2040) == ([0, 256, 512, 768, 844], [0, 256, 512, 768, 1024, 1280, 1528])
    assert prep.subimage_grid(512, 512) == ([0], [0])                    # a side equal to the crop
    assert prep.subimage_grid(513, 512) == ([0, 1], [0])                 # one pixel over it
    assert prep.subimage_grid(768, 1024) == ([0, 256], [0, 256, 512])    # exact fits: nothing appended
    assert prep.subimage_grid(40, 47, 16, 8) == ([0, 8, 16, 24], [0, 8, 16, 24, 31])
    assert prep.subimage_grid(40, 47, 16, 8, thresh_size=7) == ([0, 8, 16, 24], [0, 8, 16, 24])
    for h, w in ((511, 600), (600, 511)):
        with pytest.raises(ValueError):
            prep.subimage_grid(h, w)
    img = torch.arange(20 * 22, dtype=torch.int32).reshape(20, 22)
    subs = prep.extract_subimages(img, 16, 8)
    assert [i for i, _ in subs] == [1, 2, 3, 4]
    assert [(int(c[0, 0]) // 22, int(c[0, 0]) % 22) for _, c in subs] == [(0, 0), (0, 6), (4, 0), (4, 6)]
    assert all(c.shape == (16, 16) for _, c in subs)
    assert prep.subimage_name("0801x4T0", 7, ".png") == "0801T0_s007.png"
    assert prep.subimage_name("axx23b", 12, ".png") == "ab_s012.png"     # the replacements run one after the other
