"""The validation metrics without a GPU: the numpy restatement (metrics_reference.py) against the fixture captured from
the reference (golden/f24_metrics.npz), its Y arithmetic against to_y_channel's np.dot on a colour lattice, its two
summation orders against its own error bound on every input of the GPU tests, the host side of the C ABI (symbols,
refusals, workspace size) and the offline tool's text format."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import metrics_cases as MC
import metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the fixture ---
def _fixture_cases(g):
    for i in range(int(g["n_cases"])):
        a, b = g[f"c{i}_a"], g[f"c{i}_b"]
        yield i, a, b


def test_restatement_planes_equal_fixture_bit_for_bit(golden):
    g = golden("f24_metrics")
    for i, a, b in _fixture_cases(g):
        for img, key in ((a, "ya"), (b, "yb")):
            want = g[f"c{i}_{key}"]                      # to_y_channel: (H,W,1) float32, (H,W) for a 2-D image
            want = want.reshape(want.shape[:2])
            got = R.planes(img, 0, True)
            assert want.dtype == np.float32 and got.dtype == np.float32
            assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32)), (i, key)
        if f"c{i}_xa" in g.files:                        # tensor2img
            assert np.array_equal(R.quantise(g[f"c{i}_xa"]).reshape(a.shape), a)
            assert np.array_equal(R.quantise(g[f"c{i}_xb"]).reshape(b.shape), b)


def test_restatement_matches_fixture_psnr_ssim(golden):
    g = golden("f24_metrics")
    for i, a, b in _fixture_cases(g):
        for k in range(int(g["n_configs"])):
            crop, y = (int(v) for v in g[f"c{i}_cfg{k}"])
            m = R.metrics(a, b, crop, bool(y))
            for key in ("psnr", "ssim"):
                want = float(g[f"c{i}_{key}{k}"])
                assert abs(m[key] - want) <= 1e-12 * abs(want), (i, k, key, m[key], want)
            assert abs(m["ssim_sep"] - float(g[f"c{i}_ssim{k}"])) <= m["bound"]
            assert R.calculate_psnr(a, b, crop, test_y_channel=bool(y)) == m["psnr"]
            assert R.calculate_ssim(a, b, crop, test_y_channel=bool(y)) == m["ssim"]


# ------------------------------------------------------------------------------------------- the colour lattice ---
def test_y_arithmetic_equals_np_dot_on_colour_lattice():
    """Every (b, g, r) with each channel in {0, 4, ..., 252, 1, 254, 255}: the restatement's explicit
    ((24.966 b + 128.553 g) + 65.481 r) + 16.0 equals to_y_channel's np.dot bit for bit, with the lattice laid out as a
    list of pixels (np.dot's matrix-vector path) and as an image (its N-d path)."""
    levels = np.array(list(range(0, 256, 4)) + [1, 254, 255], dtype=np.uint8)
    lat = np.stack(np.meshgrid(levels, levels, levels, indexing="ij"), -1)          # (67,67,67,3)
    assert lat.reshape(-1, 3).shape[0] == 300763
    flat = np.ascontiguousarray(lat.reshape(-1, 1, 3))
    got = R.planes(flat, 0, True)[0, :, 0]
    for shaped in (lat.reshape(-1, 3), lat.reshape(67, 67 * 67, 3)):
        want = R.y_by_dot(shaped).reshape(-1)
        assert want.dtype == np.float32
        assert int((got.view(np.uint32) != want.view(np.uint32)).sum()) == 0


def test_grey_round_trip_restates_to_y_channel():
    """One channel with test_y_channel: to_y_channel's fl32(fl32(q / 255.0f) * 255.0f), for every q."""
    q = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    p = R.planes(q, 0, True)[0].reshape(-1)
    want = (q.astype(np.float32) / 255.) * 255.
    assert want.dtype == np.float32
    assert np.array_equal(p.view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.abs(p - np.arange(256)).max() < 1e-4


def test_tie_values_round_half_to_even():
    t = MC.tie_values()
    assert t.size >= 8
    prod = (t * np.float32(255.0)).astype(np.float64)
    assert np.all(prod - np.floor(prod) == 0.5)
    q = R.quantise(t.reshape(1, 1, -1))[0, :, 0].astype(np.int64)
    assert np.all(q % 2 == 0) and np.all(np.abs(q - prod) == 0.5)
    assert (q < prod).any() and (q > prod).any()        # both directions occur: neither half-up nor half-down


# -------------------------------------------------------------------------------------------------- the bound ---
@pytest.mark.parametrize("index", range(len(MC.cases())), ids=[c.name for c in MC.cases()])
def test_summation_orders_within_bound(index):
    """The 2-D window (filter2D's order) and the separable passes (the kernel's order) differ by less than the derived
    bound, and the bound is tight enough to mean something: at most 1e-9."""
    for m in MC.reference(index):
        assert m["bound"] <= 1e-9, m["bound"]
        assert abs(m["ssim"] - m["ssim_sep"]) < m["bound"], (m["ssim"], m["ssim_sep"], m["bound"])


def test_bound_on_flat_and_noise_planes_37x53():
    rng = np.random.default_rng(3753)
    flat_a, flat_b = np.full((1, 37, 53), 255, np.float32), np.full((1, 37, 53), 254, np.float32)
    noise_a = rng.integers(0, 256, (1, 37, 53)).astype(np.float32)
    noise_b = rng.integers(0, 256, (1, 37, 53)).astype(np.float32)
    for a, b in ((flat_a, flat_b), (noise_a, noise_b)):
        d = abs(R.ssim(a, b, "2d") - R.ssim(a, b, "sep"))
        bound = R.ssim_bound(a, b)
        print(f"2-D vs separable: {d:.3e}, bound {bound:.3e}")
        assert d < bound <= 1e-9


# -------------------------------------------------------------------------------------------------- host checks ---
NAMES = ("ssg_metric_workspace_bytes", "ssg_psnr_ssim", "ssg_metric_planes")
FAKE = ctypes.c_void_p(1 << 20)        # a non-null, 16-byte aligned address that a refused call never touches


def test_symbols_exported_declared_and_bound():
    from ssl_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.HEADER).read()
    for name in NAMES:
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\(", hdr)
        assert name in _lib.PROTOTYPES
    for k, v in (("SSG_METRIC_F32_RGB", 0), ("SSG_METRIC_U8_HWC", 1), ("SSG_METRIC_U8_CHW", 2)):
        assert re.search(rf"#define {k} {v}\b", hdr)
    assert L.ssg_abi_version() == 6
    import ssl_amd.metrics as M
    assert (M.KIND_F32_RGB, M.KIND_U8_HWC, M.KIND_U8_CHW) == (MC.F32_RGB, MC.U8_HWC, MC.U8_CHW) == (0, 1, 2)
    for name in ("calculate_psnr", "calculate_ssim", "calculate_metric", "psnr_ssim", "MetricAverager"):
        assert callable(getattr(M, name))
    import ssl_amd
    assert ssl_amd.metrics is M


def _psnr_ssim(L, a=FAKE, b=FAKE, kind=0, B=1, C=3, H=32, W=32, crop=4, y=1, out=FAKE, ws=FAKE, nb=None):
    if nb is None:
        nb = L.ssg_metric_workspace_bytes(B, C, H, W, crop)
    return L.ssg_psnr_ssim(a, b, kind, B, C, H, W, crop, y, out, ws, nb, None)


def test_refusals_before_any_launch():
    """Every refusal is decided on the host from the arguments alone: no pointer is followed (they are null or fake)."""
    from ssl_amd import _lib
    L = _lib.lib()
    BADARG, TOOLARGE, WORKSPACE, IMAGESMALL, ALIGN = -1, -2, -3, -4, -5
    assert _psnr_ssim(L, a=None) == BADARG and _psnr_ssim(L, b=None) == BADARG
    assert _psnr_ssim(L, out=None) == BADARG and _psnr_ssim(L, ws=None) == BADARG
    for C in (0, 2, 4):
        assert _psnr_ssim(L, C=C, nb=1 << 20) == BADARG
    assert _psnr_ssim(L, crop=-1, nb=1 << 20) == BADARG
    assert _psnr_ssim(L, kind=3, nb=1 << 20) == BADARG and _psnr_ssim(L, kind=-1, nb=1 << 20) == BADARG
    assert _psnr_ssim(L, B=0, nb=1 << 20) == BADARG and _psnr_ssim(L, H=0, nb=1 << 20) == BADARG
    assert _psnr_ssim(L, B=65536, H=11, W=11, crop=0, nb=1 << 30) == TOOLARGE
    # a cropped side shorter than 11
    assert _psnr_ssim(L, H=18, W=32, crop=4, nb=1 << 20) == IMAGESMALL
    assert _psnr_ssim(L, H=32, W=10, crop=0, nb=1 << 20) == IMAGESMALL
    assert _psnr_ssim(L, H=8, W=8, crop=4, nb=1 << 20) == IMAGESMALL      # nothing left at all
    # (11 x 11 after the crop is in the domain: the size query says so without launching anything)
    assert L.ssg_metric_workspace_bytes(1, 3, 19, 19, 4) > 0
    assert L.ssg_metric_workspace_bytes(1, 3, 18, 19, 4) == 0
    assert L.ssg_metric_workspace_bytes(1, 2, 32, 32, 0) == 0
    assert L.ssg_metric_workspace_bytes(1, 3, 32, 32, -1) == 0
    # the workspace: too small, then misaligned
    need = L.ssg_metric_workspace_bytes(1, 3, 32, 32, 4)
    assert _psnr_ssim(L, y=0, nb=need - 1) == WORKSPACE
    assert _psnr_ssim(L, ws=ctypes.c_void_p((1 << 20) + 8)) == ALIGN
    # the planes alone
    assert L.ssg_metric_planes(None, 0, 1, 3, 32, 32, 4, 1, FAKE, None) == BADARG
    assert L.ssg_metric_planes(FAKE, 0, 1, 3, 32, 32, 4, 1, None, None) == BADARG
    assert L.ssg_metric_planes(FAKE, 0, 1, 2, 32, 32, 4, 1, FAKE, None) == BADARG
    assert L.ssg_metric_planes(FAKE, 0, 1, 3, 32, 32, -1, 1, FAKE, None) == BADARG
    assert L.ssg_metric_planes(FAKE, 5, 1, 3, 32, 32, 4, 1, FAKE, None) == BADARG
    assert L.ssg_metric_planes(FAKE, 0, 1, 3, 8, 32, 4, 1, FAKE, None) == IMAGESMALL
    for rc in (BADARG, TOOLARGE, WORKSPACE, IMAGESMALL, ALIGN):
        assert L.ssg_status_string(rc)


def test_workspace_holds_partials_only():
    """At most 512 workgroups per image leave three 8-byte partials each: 12 KiB per image, whatever the image size."""
    from ssl_amd import _lib
    L = _lib.lib()
    assert L.ssg_metric_workspace_bytes(1, 3, 2040, 1356, 4) == 3 * 512 * 8
    assert L.ssg_metric_workspace_bytes(1, 3, 2040, 1356, 0) == 3 * 512 * 8
    # 16 x 3 x 256 x 256, crop 4: a 238 x 238 map, 15 x 8 tiles per plane, 360 per image
    assert L.ssg_metric_workspace_bytes(16, 3, 256, 256, 4) == 3 * 16 * 360 * 8
    # one tile: one partial of each kind, each on a 256-byte boundary
    assert L.ssg_metric_workspace_bytes(1, 1, 11, 11, 0) == 3 * 256
    assert 3 * 512 * 8 < 2040 * 1356 // 64


def test_second_trip_cases_cross_the_workgroup_cap():
    """The cases named *_second_trip have more tiles than an image gets workgroups, the cap read off the size function
    (its per-image share stops growing there): raising the cap fails here instead of sending them back to one trip."""
    from ssl_amd import _lib
    L = _lib.lib()
    share = L.ssg_metric_workspace_bytes(1, 3, 4000, 4000, 0)
    cap = share // (3 * 8)
    assert share == L.ssg_metric_workspace_bytes(1, 3, 2040, 1356, 4) and share % (3 * 8) == 0
    named = {c.name: c for c in MC.cases()}
    for name in ("many_tiles_second_trip", "y_second_trip", "grey_y_second_trip", "batch_second_trip"):
        assert MC.tiles(named[name]) > cap, (name, MC.tiles(named[name]), cap)
    assert MC.tiles(named["y_second_trip"]) == MC.tiles(named["grey_y_second_trip"]) == 24 * 23
    assert MC.tiles(named["cross_hwc_c3_y1_b3"]) < cap
    # batch_second_trip: three images at the cap, no growth from its shape to a larger one
    B, C, H, W = MC.geometry(named["batch_second_trip"])
    assert (B, named["batch_second_trip"].y) == (3, False)
    nb = L.ssg_metric_workspace_bytes(B, C, H, W, 0)
    assert nb == B * share == L.ssg_metric_workspace_bytes(B, C, 2 * H, 2 * W, 0)
    a = named["batch_second_trip"].a
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2]) and not np.array_equal(a[0], a[2])


# ---------------------------------------------------------------------------------------------- the offline tool ---
def _load_tool():
    spec = importlib.util.spec_from_file_location("calculate_psnr_ssim_tool",
                                                  os.path.join(ROOT, "scripts", "calculate_psnr_ssim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("y", [True, False])
def test_offline_tool_text_format(tmp_path, monkeypatch, y):
    from PIL import Image
    import ssl_amd.metrics as M
    monkeypatch.setattr(M, "calculate_psnr", R.calculate_psnr)
    monkeypatch.setattr(M, "calculate_ssim", R.calculate_ssim)
    tool = _load_tool()
    gt_dir = tmp_path / "Set" / "GT" / "GTmod12"
    out_dir = tmp_path / "results" / "visualization" / "Set"
    gt_dir.mkdir(parents=True)
    out_dir.mkdir(parents=True)
    rng = np.random.default_rng(5)
    want = []
    for name in ("baboon", "zebra"):
        gt = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)                         # RGB, as PIL holds it
        sr = np.clip(gt.astype(np.int32) + rng.integers(-8, 9, gt.shape), 0, 255).astype(np.uint8)
        Image.fromarray(gt).save(gt_dir / f"{name}.png")
        Image.fromarray(sr).save(out_dir / f"{name}_x4.png")
        m = R.metrics(gt[..., ::-1], sr[..., ::-1], 4, y)
        want.append((name, m["psnr"], m["ssim"]))
    (gt_dir / ".hidden").write_text("skipped")
    argv = ["--gt", str(gt_dir), "--restored", str(out_dir), "--suffix", "_x4", "--crop_border", "4",
            "--test_y_channel", "true" if y else "false"]
    assert tool.main(argv) == 0
    text = (out_dir.parent / "PSNR_SSIM_GT.txt").read_text(encoding="utf-8")
    lines = text.split("\n")
    assert len(lines) == 3 and not text.endswith("\n")
    for line, (name, p, s) in zip(lines, want):
        assert line == f"{name:25}. \tPSNR: {p:.6f} dB, \tSSIM: {s:.6f}"
        assert re.fullmatch(r"\S+ *\. \tPSNR: \d+\.\d{6} dB, \tSSIM: \d\.\d{6}", line)
    avg_p = sum(w[1] for w in want) / 2
    avg_s = sum(w[2] for w in want) / 2
    assert lines[2] == f"Average: PSNR: {avg_p:.6f} dB, SSIM: {avg_s:.6f}"


def test_public_functions_keep_the_reference_errors():
    """The shape assertion and the input_order ValueError come before anything touches a device."""
    import ssl_amd.metrics as M
    a, b = np.zeros((20, 20, 3), np.uint8), np.zeros((20, 21, 3), np.uint8)
    for fn in (M.calculate_psnr, M.calculate_ssim):
        with pytest.raises(AssertionError, match="Image shapes are different"):
            fn(a, b, 0)
        with pytest.raises(ValueError, match="Wrong input_order"):
            fn(a, a, 0, input_order="WHC")
    with pytest.raises(KeyError, match="calculate_niqe"):
        M.calculate_metric(dict(img=a, img2=a), dict(type="calculate_niqe", crop_border=0))
