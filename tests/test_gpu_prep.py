"""The Pillow-exact resize kernel (ssl_amd/csrc/ssg_resample.hip) and ssl_amd.prep on the GPU against the numpy
restatement of Pillow's algorithm (tests/pil_resize_reference.py, held to Pillow itself by tests/test_cpu_prep.py).
Exact equality throughout: the algorithm is integer from its tables on.

Output sizes sit on the kernel's first tile (ssg_resample_tile: one tile, and one tile plus a pixel on each axis, so
that every case but the one-tile ones has a ragged second tile row and column); the ratios reach all four tiles of the
host's list (32 x 64 up to about 0.6, 16 x 64 and 16 x 32 between, 8 x 32 from 1 / 3 down, at 8 : 1 on both axes and
three channels with the 114,176 B of LDS that are the most a supported call takes).  The grid is not capped: one
workgroup per tile and image."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import pil_resize_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f29_prep.npz")
TH, TW = 32, 64                      # ssg_resample_tile(); test_tile_matches_the_library ties them to the library
MAX_RATIO = 8
E_TOOLARGE = -2
ONE = (TH, TW)
PLUS = (TH + 1, TW + 1)


def _in(out, ry, rx):
    return (max(1, round(out[0] * ry)), max(1, round(out[1] * rx)))


# (input (H, W), output (h, w)): LANCZOS, both channel counts, random content
LANCZOS_SHAPES = [
    (_in(ONE, 4 / 3, 4 / 3), ONE),                     # 0.75, exactly one tile
    (_in(PLUS, 4 / 3, 4 / 3), PLUS),                   # 0.75, one tile plus a pixel
    (_in(PLUS, 1 / 0.6, 1 / 0.6), PLUS),               # 0.6
    ((3 * PLUS[0], 3 * PLUS[1]), PLUS),                # 1 / 3
    (_in(PLUS, 4.3, 4.3), PLUS),                       # near 1 / 4.3
    ((MAX_RATIO * PLUS[0], PLUS[1] + 2), PLUS),        # the largest ratio down the rows, the columns near 1
    ((PLUS[0] + 2, MAX_RATIO * PLUS[1]), PLUS),        # the largest ratio along the columns
    ((MAX_RATIO * PLUS[0], MAX_RATIO * PLUS[1]), PLUS),    # on both: the smaller tiles
    ((6 * PLUS[0], 6 * PLUS[1]), PLUS),                # 6 : 1 on both
    ((97, 131), (96, 128)),                            # load_img's rounding down to a multiple of 32
    (_in(PLUS, 1 / 1.7, 1 / 1.7), (PLUS[0] + 1, PLUS[1])),   # an upscale of about 1.7
    ((PLUS[0], 108), PLUS),                            # columns only
    ((55, PLUS[1]), PLUS),                             # rows only
    (PLUS, PLUS),                                      # identity
    ((5, 300), (1, 100)),                              # one output row
    ((19, 7), (6, 2)),
    ((215, 310), (5 * TH + 7, 3 * TW + 9)),            # six by four tiles
]
OTHER_FILTERS = ['bilinear', 'bicubic', 'box', 'hamming']
CONTENTS = ['const255', 'checker', 'blocks']

CASES = [(i, o, c, 'lanczos', 'random') for i, o in LANCZOS_SHAPES for c in (1, 3)]
CASES += [(i, PLUS, 3, f, 'random') for f in OTHER_FILTERS for i in ((3 * PLUS[0], 3 * PLUS[1]), _in(PLUS, 0.6, 0.6))]
CASES += [(i, PLUS, c, 'lanczos', k) for k in CONTENTS
          for i, c in ((_in(PLUS, 1 / 0.6, 1 / 0.6), 3), ((3 * PLUS[0], 3 * PLUS[1]), 1))]


def _id(case):
    (H, W), (h, w), c, f, k = case
    return f"{H}x{W}-{h}x{w}-c{c}-{f}-{k}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _pair(case):
    """(input (H,W,C) uint8, the restatement's output): computed once and shared (the poison test runs the same cases)."""
    (H, W), (h, w), c, f, kind = case
    a = R.content(kind, H, W, c, seed=H * 1000 + W + c)
    want = R.resize(a, (w, h), f)
    a.setflags(write=False)
    want.setflags(write=False)
    return a, want


def _gpu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _resize(dev, case):
    from ssl_amd import prep
    (_, _), (h, w), c, f, _ = case
    a, _ = _pair(case)
    return prep.resize(_gpu(a, dev), (w, h), f)


@pytest.mark.gpu
def test_tile_matches_the_library(dev):
    from ssl_amd import _lib
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.lib().ssg_resample_tile(ctypes.byref(th), ctypes.byref(tw)) == 0
    assert (th.value, tw.value) == (TH, TW) and _lib.lib().ssg_resample_max_ratio() == MAX_RATIO


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_resize_equals_the_restatement(dev, case):
    _, want = _pair(case)
    got = _resize(dev, case).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.gpu
def test_two_dimensional_input_and_odd_addresses(dev):
    """(H,W) in gives (H,W) out; a source whose first byte sits at every address modulo 4 (the footprint is read as
    aligned dwords) and rows of an odd byte length give the same bytes."""
    from ssl_amd import prep
    case = (_in(PLUS, 1 / 0.6, 1 / 0.6), PLUS, 1, 'lanczos', 'random')
    a, want = _pair(case)
    got = prep.resize(_gpu(a[..., 0], dev), (PLUS[1], PLUS[0]))
    assert got.shape == PLUS and np.array_equal(got.cpu().numpy(), want[..., 0])
    case = ((55, 107), PLUS, 3, 'lanczos', 'random')
    a, want = _pair(case)
    flat = torch.from_numpy(np.array(a)).reshape(-1)
    for shift in range(4):
        store = torch.zeros(flat.numel() + 8, dtype=torch.uint8, device=dev)
        store[shift:shift + flat.numel()] = flat.to(dev)
        view = store[shift:shift + flat.numel()].view(55, 107, 3)
        assert view.data_ptr() % 4 == (store.data_ptr() + shift) % 4
        assert np.array_equal(prep.resize(view, (PLUS[1], PLUS[0])).cpu().numpy(), want), shift


@pytest.mark.gpu
def test_batch_of_two_equals_its_singles(dev):
    from ssl_amd import prep
    size = (3 * PLUS[0] + 1, 2 * PLUS[1] + 5)
    a = np.stack([R.content('random', *size, 3, seed=s) for s in (5, 6)])
    x = _gpu(a, dev)
    both = prep.resize(x, (PLUS[1], PLUS[0]))
    assert both.shape == (2,) + PLUS + (3,)
    for b in range(2):
        assert torch.equal(both[b], prep.resize(x[b], (PLUS[1], PLUS[0])))
        assert np.array_equal(both[b].cpu().numpy(), R.resize(a[b], (PLUS[1], PLUS[0])))


@pytest.mark.gpu
def test_float_epilogues_on_every_level(dev):
    """All 256 levels through both float epilogues, identity and a resize: 'unit' is numpy's float32 v / 255, 'signed'
    is load_img's expression (numpy's division, torch's 2. * x - 1.), bit for bit, in (B,C,H,W)."""
    from ssl_amd import prep
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    a = np.stack([ramp, ramp.T, ramp[::-1]], 2)
    for size in ((16, 16), (13, 9)):
        v = R.resize(a, size)
        unit = (v.astype(np.float32) / 255.0)[None].transpose(0, 3, 1, 2)
        signed = (2. * torch.from_numpy(unit) - 1.).numpy()
        got_u = prep.resize(_gpu(a, dev), size, out='unit').cpu().numpy()
        got_s = prep.resize(_gpu(a, dev), size, out='signed').cpu().numpy()
        assert got_u.dtype == got_s.dtype == np.float32 and got_u.shape == unit.shape == got_s.shape
        assert np.array_equal(got_u.view(np.int32), unit.view(np.int32))
        assert np.array_equal(got_s.view(np.int32), signed.view(np.int32))
    assert set(np.unique(R.resize(a, (16, 16)))) == set(range(256))


@pytest.mark.gpu
def test_load_img_equals_the_fork_s_expression(dev):
    from PIL import Image
    from ssl_amd import prep
    a = R.content('random', 97, 131, 3, seed=3)
    image = Image.fromarray(a).resize((128, 96), resample=Image.LANCZOS)        # test.py:115-120 on the CPU
    want = 2. * torch.from_numpy((np.array(image).astype(np.float32) / 255.0)[None].transpose(0, 3, 1, 2)) - 1.
    for src in (a, Image.fromarray(a), Image.fromarray(a).convert("RGBA")):
        got = prep.load_img(src, dev)
        assert got.shape == (1, 3, 96, 128) and got.dtype == torch.float32
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.FILTERS))
def test_resize_equals_pillow_itself(dev, name):
    from PIL import Image
    from ssl_amd import prep
    a = R.content('random', 131, 97, 3, seed=9)
    want = np.array(Image.fromarray(a).resize((72, 98), resample=R.FILTERS[name]))
    assert np.array_equal(prep.resize(_gpu(a, dev), (72, 98), name).cpu().numpy(), want)
    assert np.array_equal(prep.resize(_gpu(a, dev), (72, 98), R.FILTERS[name]).cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["gan", "dm"])
def test_multiscale_reproduces_the_reference_scripts(dev, variant):
    """Every PNG the two reference scripts wrote (tests/golden/f29_prep.npz), by name and by pixel."""
    from ssl_amd import prep
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    names, kept = [], []
    for key in sorted(k for k in golden if k.startswith("in_")):
        name = key[3:]
        outs, keep = prep.multiscale(_gpu(golden[key], dev), variant, 24)
        kept += [name] if keep else []
        for suffix, im in outs:
            names.append(name + suffix)
            assert np.array_equal(im.cpu().numpy(), golden[f"{variant}_{name}{suffix}"]), (name, suffix)
    assert sorted(names) == sorted(k[len(variant) + 1:] for k in golden
                                   if k.startswith(variant + "_") and not k.endswith("_kept"))
    assert kept == list(golden[f"{variant}_kept"])


@pytest.mark.gpu
def test_a_ratio_past_the_limit_is_refused(dev):
    from ssl_amd import _lib, prep
    L = _lib.lib()
    a = torch.zeros((20, MAX_RATIO * 10 + 1, 3), dtype=torch.uint8, device=dev)
    out = torch.full((20, 10, 3), 7, dtype=torch.uint8, device=dev)
    xb, xk = prep._device_table(MAX_RATIO * 10 + 1, 10, 1, dev)
    rc = L.ssg_resample(a.data_ptr(), 1, 3, 20, MAX_RATIO * 10 + 1, 20, 10, 1, xb.data_ptr(), xk.data_ptr(), None, None, 0,
                        out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == E_TOOLARGE and bool((out == 7).all())
    with pytest.raises(NotImplementedError):
        prep.resize(a, (10, 20))
    assert prep.resize(a[:, :MAX_RATIO * 10], (10, 20)).shape == (20, 10, 3)     # the limit itself is taken


@pytest.mark.gpu
def test_a_table_that_leaves_its_footprint_writes_nothing(dev):
    """The tables are the caller's device memory: bounds that reach past the rows the tile staged make the workgroup
    return instead of reading beyond its LDS."""
    from ssl_amd import _lib, prep
    L = _lib.lib()
    a = torch.zeros((40, 90, 1), dtype=torch.uint8, device=dev)
    out = torch.full((40, 30, 1), 7, dtype=torch.uint8, device=dev)
    xb, xk = (t.clone() for t in prep._device_table(90, 30, 1, dev))
    xb[5, 0] = 88                                           # a window that ends beyond the tile's last column (90)
    assert L.ssg_resample(a.data_ptr(), 1, 1, 40, 90, 40, 30, 1, xb.data_ptr(), xk.data_ptr(), None, None, 0,
                          out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def poison_cases():
    """The outputs the LDS-poison test compares bit for bit (test_gpu_prep_poison.py): every case above."""
    dev = torch.device("cuda")
    from ssl_amd import prep
    out = [_resize(dev, case) for case in CASES]
    ramp = _gpu(np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2), dev)
    out += [prep.resize(ramp, (13, 9), out='unit'), prep.resize(ramp, (16, 16), out='signed')]
    return out
