"""NIQE without a GPU: the fp64 restatement (niqe_reference.py) against the fixture recorded from the reference
(golden/f26_niqe.npz, golden/make_golden_niqe.py), stage by stage; its alpha search, Gamma table and the conditioning
of Sigma; the host side of the C ABI (symbols, refusals, workspace size, the table); the parameter file's resolution;
the public functions' errors and the offline tool's text format.

The reference keeps float32 planes (an accident of its astype), the restatement is float64 from the integer plane on.
MEASURED holds each stage's largest deviation between the two over the fixture, measured when the fixture was made
(`python tests/test_cpu_niqe.py` prints them; profiles/niqe_parity.txt keeps them); the tests allow 4 x that, the
factor standing for inputs of the same kinds the fixture does not hold.  No GPU output enters these bounds."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import niqe_reference as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz")

# stage -> the largest |fixture - restatement| over the fixture ('_rel': relative to the fixture's value)
MEASURED = {
    "plane": 0.0,               # the rounded plane: integers, equal
    "plane2": 3.0518e-05,       # half an ulp of float32 at 255 twice over
    "mscn1": 8.0047e-04,        # float32 cancellation in E[I^2] - mu^2 on the flat parts of the hard-edged case
    "mscn2": 7.8147e-04,
    "feat_abs": 5.0687e-06,     # the 26 entries per row that are not an alpha
    "feat_rel": 1.1320e-03,     # (the AGGD mean (beta_r - beta_l) G(2/a) / G(1/a) near zero)
    "score_rel": 2.0893e-06,
}
FACTOR = 4.0
ALPHA = [c + 18 * s for s in (0, 1) for c in N.ALPHA_COLUMNS]
OTHER = [c for c in range(N.NF) if c not in ALPHA]


def params():
    return np.load(PARAMS)


def cases(g):
    for i in range(int(g["n_cases"])):
        yield i, g[f"c{i}_img"], str(g[f"c{i}_order"]), int(g[f"c{i}_crop"])


_RESTATED = {}


def restated(g, i):
    """The restatement's stages of fixture case i, computed once."""
    if i not in _RESTATED:
        P = params()
        _RESTATED[i] = N.niqe(g[f"c{i}_img"], int(g[f"c{i}_crop"]), P["mu_pris_param"], P["cov_pris_param"],
                              str(g[f"c{i}_order"]))
    return _RESTATED[i]


def _stage_deviation(g, i, key, got):
    """max |fixture - restatement| of one recorded plane: whole, or its bottom rows and right columns."""
    if f"c{i}_{key}" in g.files:
        return float(np.abs(got - g[f"c{i}_{key}"]).max())
    if f"c{i}_{key}_bottom" in g.files:
        b, r = g[f"c{i}_{key}_bottom"], g[f"c{i}_{key}_right"]
        return max(float(np.abs(got[-b.shape[0]:] - b).max()), float(np.abs(got[:, -r.shape[1]:] - r).max()))
    return None


def measure(g):
    out = {k: 0.0 for k in MEASURED}
    for i, img, order, crop in cases(g):
        r = restated(g, i)
        pl = g[f"c{i}_plane"].astype(np.float64)
        out["plane"] = max(out["plane"], float(np.abs(pl[:r["plane1"].shape[0], :r["plane1"].shape[1]] - r["plane1"]).max()))
        for key, got in (("plane2", r["plane2"]), ("mscn1", N.mscn(r["plane1"])), ("mscn2", N.mscn(r["plane2"]))):
            d = _stage_deviation(g, i, key, got)
            if d is not None:
                out[key] = max(out[key], d)
        want, got = g[f"c{i}_distparam"][:, OTHER], r["feat"][:, OTHER]
        ok = ~np.isnan(want)
        out["feat_abs"] = max(out["feat_abs"], float(np.abs(want - got)[ok].max()))
        out["feat_rel"] = max(out["feat_rel"], float((np.abs(want - got)[ok] / np.abs(want[ok])).max()))
        score = float(g[f"c{i}_score"])
        if not np.isnan(score):
            out["score_rel"] = max(out["score_rel"], abs(r["score"] - score) / score)
    return out


# ------------------------------------------------------------------------------------------------- the fixture ---
def test_fixture_holds_the_cases_the_metric_can_go_wrong_on(golden):
    g = golden("f26_niqe")
    shapes = {i: (img.shape, order, crop) for i, img, order, crop in cases(g)}
    assert shapes[0] == ((96, 192, 3), 'HWC', 0) and shapes[1] == ((192, 96, 3), 'HWC', 0)
    assert shapes[2] == ((200, 300, 3), 'HWC', 4)
    assert shapes[3][1] == 'CHW' and shapes[4][1] == 'HW' and g["c4_img"].dtype.kind == 'f'
    assert "c5_x" in g.files and (g["c5_x"] < 0).any() and (g["c5_x"] > 1).any()
    assert int(np.isnan(g["c6_distparam"]).any(1).sum()) == 1 and g["c6_distparam"].shape[0] == 4
    assert g["c7_distparam"].shape[0] == 1 and np.isnan(float(g["c7_score"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "f26_niqe.npz")) < 1 << 20
    # the float tensor case: img is tensor2img of x
    import metrics_reference as MR
    assert np.array_equal(MR.quantise(g["c5_x"].astype(np.float32)), g["c5_img"])


def test_window_and_taps_are_the_closed_forms():
    assert np.abs(params()["gaussian_window"] - N.window()).max() < 1e-16
    w = N.resize_taps()
    assert np.array_equal(w, np.array([-3, -9, 29, 111, 111, 29, -9, -3]) / 256.0)


def test_restatement_against_fixture_stage_by_stage(golden):
    g = golden("f26_niqe")
    m = measure(g)
    for k in MEASURED:
        print(f"{k:10s} measured {m[k]:.4e}  bound {FACTOR * MEASURED[k]:.4e}")
    for k in MEASURED:
        assert m[k] <= FACTOR * MEASURED[k], (k, m[k], MEASURED[k])
    for i, img, order, crop in cases(g):
        want, got = g[f"c{i}_distparam"], restated(g, i)["feat"]
        assert want.shape == got.shape
        assert np.array_equal(np.isnan(want), np.isnan(got)), i
        assert np.isnan(float(g[f"c{i}_score"])) == np.isnan(restated(g, i)["score"]), i


def test_alpha_equals_fixture_away_from_midpoints(golden):
    """alpha is a grid value: equal to the reference's wherever the restatement's rhatnorm lies further than 1e-6
    (relative) from a midpoint of adjacent r(gam) entries, one grid step off at most elsewhere; at most 1 % of the
    fixture's fits are that close to a midpoint."""
    g = golden("f26_niqe")
    fits = excused = 0
    for i, img, order, crop in cases(g):
        r = restated(g, i)
        want, got = g[f"c{i}_distparam"][:, ALPHA], r["feat"][:, ALPHA]
        margin = N.midpoint_margin(r["t"])
        assert margin.shape == want.shape
        far = margin > 1e-6
        assert np.array_equal(want[far], got[far]), i
        assert np.all(np.abs(want[~far] - got[~far]) <= 0.001 * (1 + 1e-9)), i
        fits += margin.size
        excused += int((~far).sum())
    print(f"{excused} of {fits} fits within 1e-6 of a midpoint")
    assert fits >= 200 and excused <= 0.01 * fits


def test_no_fixture_fit_within_1e9_of_a_midpoint(golden):
    """What the GPU test's exact alpha comparison rests on."""
    g = golden("f26_niqe")
    for i, img, order, crop in cases(g):
        assert N.midpoint_margin(restated(g, i)["t"]).min() > 1e-9, i


def test_gamma_tables_against_scipy():
    import scipy.special as S
    from ssl_amd import _lib
    _lib.build()
    gam = N.GAM
    assert gam.size == 9801
    want = np.stack([gam, S.gamma(2 / gam) ** 2 / (S.gamma(1 / gam) * S.gamma(3 / gam)), S.gamma(1 / gam) / S.gamma(3 / gam),
                     S.gamma(2 / gam) / S.gamma(1 / gam)])
    lib_table = np.empty((4, 9801))
    assert _lib.lib().ssg_niqe_table(lib_table.ctypes.data) == 0
    assert _lib.lib().ssg_niqe_table(None) == -1
    for name, t in (("restatement", N.table()), ("library", lib_table)):
        assert np.array_equal(t[0], gam), name                      # np.arange's own values
        assert np.abs(t[1:] / want[1:] - 1).max() <= 1e-13, (name, np.abs(t[1:] / want[1:] - 1).max())
        assert np.all(np.diff(t[1]) > 0), name                      # increasing: what the bisection rests on


def test_sigma_is_far_from_singular(golden):
    """lambda_min / lambda_max of Sigma > 1e-12 on every case with a score: there pinv (cut-off 1e-15) is the inverse."""
    g = golden("f26_niqe")
    P = params()
    ev = np.linalg.eigvalsh(P["cov_pris_param"])
    assert np.array_equal(P["cov_pris_param"], P["cov_pris_param"].T) and ev[0] > 0
    for i, img, order, crop in cases(g):
        r = restated(g, i)
        if np.isnan(r["score"]):
            assert i == 7
            continue
        assert r["ratio"] > 1e-12, (i, r["ratio"])
        pinv = float(r["d"] @ np.linalg.pinv(r["sigma"]) @ r["d"])
        assert abs(pinv - r["q2"]) <= 64 * r["cond"] * 2.2e-16 * r["q2"]


# -------------------------------------------------------------------------------------------------- host checks ---
NAMES = ("ssg_niqe_workspace_bytes", "ssg_niqe", "ssg_niqe_planes", "ssg_niqe_features", "ssg_niqe_table")
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
    assert re.search(r"#define SSG_NIQE_F32_PLANE 3\b", hdr)
    import ssl_amd.metrics as M
    assert M.KIND_F32_PLANE == 3
    for name in ("calculate_niqe", "niqe", "load_niqe_params"):
        assert callable(getattr(M, name)) and name in M.__all__
    assert callable(M.MetricAverager.add_niqe)


def _niqe(L, img=FAKE, kind=1, B=1, C=3, H=200, W=300, crop=4, convert=0, mu=FAKE, cov=FAKE, out=FAKE, ws=FAKE, nb=None):
    if nb is None:
        nb = L.ssg_niqe_workspace_bytes(B, C, H, W, crop)
    return L.ssg_niqe(img, kind, B, C, H, W, crop, convert, mu, cov, out, ws, nb, None)


def test_refusals_before_any_launch():
    """Every refusal is decided on the host from the arguments alone: no pointer is followed (they are null or fake)."""
    from ssl_amd import _lib
    L = _lib.lib()
    BADARG, TOOLARGE, WORKSPACE, IMAGESMALL, ALIGN = -1, -2, -3, -4, -5
    big = 1 << 30
    for k in ("img", "mu", "cov", "out", "ws"):
        assert _niqe(L, **{k: None}) == BADARG, k
    for C in (0, 2, 4):
        assert _niqe(L, C=C, nb=big) == BADARG
    assert _niqe(L, crop=-1, nb=big) == BADARG
    assert _niqe(L, kind=4, nb=big) == BADARG and _niqe(L, kind=-1, nb=big) == BADARG
    assert _niqe(L, convert=2, nb=big) == BADARG and _niqe(L, convert=-1, nb=big) == BADARG
    assert _niqe(L, convert=1, C=1, nb=big) == BADARG            # 'gray' of one channel
    assert _niqe(L, kind=3, C=3, nb=big) == BADARG               # the plane kind has one channel
    assert _niqe(L, B=0, nb=big) == BADARG and _niqe(L, W=0, nb=big) == BADARG
    assert _niqe(L, B=65536, H=96, W=96, crop=0, nb=big) == TOOLARGE
    # a cropped side shorter than 96: no block
    assert _niqe(L, H=95, W=200, crop=0, nb=big) == IMAGESMALL
    assert _niqe(L, H=200, W=103, crop=4, nb=big) == IMAGESMALL
    assert _niqe(L, H=8, W=8, crop=4, nb=big) == IMAGESMALL
    need = L.ssg_niqe_workspace_bytes(1, 3, 200, 300, 4)
    assert _niqe(L, nb=need - 1) == WORKSPACE
    assert _niqe(L, ws=ctypes.c_void_p((1 << 20) + 8)) == ALIGN
    # the planes and the features alone
    P, F = L.ssg_niqe_planes, L.ssg_niqe_features
    assert P(None, 1, 1, 3, 200, 300, 4, 0, FAKE, FAKE, None) == BADARG
    assert P(FAKE, 1, 1, 3, 200, 300, 4, 0, None, FAKE, None) == BADARG
    assert P(FAKE, 1, 1, 3, 200, 300, 4, 0, FAKE, None, None) == BADARG
    assert P(FAKE, 1, 1, 3, 200, 300, 4, 2, FAKE, FAKE, None) == BADARG
    assert P(FAKE, 1, 1, 3, 95, 300, 0, 0, FAKE, FAKE, None) == IMAGESMALL
    assert F(FAKE, 1, 1, 3, 200, 300, 4, 0, None, FAKE, need, None) == BADARG
    assert F(FAKE, 1, 1, 3, 200, 300, 4, 0, FAKE, None, need, None) == BADARG
    assert F(FAKE, 1, 1, 3, 200, 300, 4, 0, FAKE, FAKE, need - 1, None) == WORKSPACE
    assert F(FAKE, 1, 1, 3, 95, 300, 0, 0, FAKE, FAKE, big, None) == IMAGESMALL


def test_workspace_holds_planes_features_and_flags():
    """Plane 1 (fp32), plane 2 (fp64, a quarter of the pixels), 36 fp64 per block and one flag per block, each piece on
    a 256-byte boundary; 0 for every shape that would be refused."""
    from ssl_amd import _lib
    L = _lib.lib()

    def want(B, H, W, crop):
        nbh, nbw = (H - 2 * crop) // 96, (W - 2 * crop) // 96
        pieces = (4 * B * 96 * nbh * 96 * nbw, 8 * B * 48 * nbh * 48 * nbw, 8 * B * nbh * nbw * 36, 4 * B * nbh * nbw)
        return sum((p + 255) // 256 * 256 for p in pieces)

    for B, C, H, W, crop in ((1, 3, 200, 300, 4), (1, 3, 2040, 1356, 4), (16, 3, 256, 256, 0), (1, 1, 96, 96, 0),
                             (3, 1, 192, 192, 0)):
        assert L.ssg_niqe_workspace_bytes(B, C, H, W, crop) == want(B, H, W, crop)
    assert L.ssg_niqe_workspace_bytes(1, 3, 103, 200, 4) == 0
    assert L.ssg_niqe_workspace_bytes(1, 3, 104, 104, 4) > 0
    assert L.ssg_niqe_workspace_bytes(1, 2, 200, 200, 0) == 0
    assert L.ssg_niqe_workspace_bytes(1, 3, 200, 200, -1) == 0
    assert L.ssg_niqe_workspace_bytes(0, 3, 200, 200, 0) == 0


# ------------------------------------------------------------------------------------------- the parameter file ---
def test_load_niqe_params_resolution_order_and_error(tmp_path, monkeypatch):
    import torch
    import ssl_amd.metrics as M
    cpu = torch.device("cpu")
    P = params()
    # a path, a mapping
    mu, cov = M.load_niqe_params(PARAMS, device=cpu)
    assert mu.dtype == cov.dtype == torch.float64 and mu.shape == (36,) and cov.shape == (36, 36)
    assert np.array_equal(mu.numpy(), P["mu_pris_param"].reshape(-1)) and np.array_equal(cov.numpy(), P["cov_pris_param"])
    assert M.load_niqe_params(PARAMS, device=cpu)[0] is mu                         # cached per path and device
    mu2, _ = M.load_niqe_params(dict(mu_pris_param=P["mu_pris_param"] + 1, cov_pris_param=P["cov_pris_param"]), device=cpu)
    assert np.array_equal(mu2.numpy(), P["mu_pris_param"].reshape(-1) + 1)
    with pytest.raises(ValueError, match="36"):
        M.load_niqe_params(dict(mu_pris_param=np.zeros(35), cov_pris_param=np.zeros((36, 36))), device=cpu)
    # None: the environment variable first
    shifted = tmp_path / "env.npz"
    np.savez(shifted, mu_pris_param=P["mu_pris_param"] + 2, cov_pris_param=P["cov_pris_param"])
    pkg = tmp_path / "site" / "basicsr"
    (pkg / "metrics").mkdir(parents=True)
    (pkg / "__init__.py").write_text("raise RuntimeError('basicsr must be located, not imported')\n")
    np.savez(pkg / "metrics" / "niqe_pris_params.npz", mu_pris_param=P["mu_pris_param"] + 3,
             cov_pris_param=P["cov_pris_param"])
    monkeypatch.syspath_prepend(str(tmp_path / "site"))
    importlib.invalidate_caches()
    monkeypatch.setenv(M.NIQE_PARAMS_ENV, str(shifted))
    assert np.array_equal(M.load_niqe_params(device=cpu)[0].numpy(), P["mu_pris_param"].reshape(-1) + 2)
    # then the file beside an installed basicsr.metrics, found without importing basicsr
    monkeypatch.delenv(M.NIQE_PARAMS_ENV)
    assert np.array_equal(M.load_niqe_params(device=cpu)[0].numpy(), P["mu_pris_param"].reshape(-1) + 3)
    import sys
    assert "basicsr" not in sys.modules
    # then the error that names both
    os.remove(pkg / "metrics" / "niqe_pris_params.npz")
    with pytest.raises(FileNotFoundError) as e:
        M.load_niqe_params(device=cpu)
    assert M.NIQE_PARAMS_ENV in str(e.value) and "basicsr" in str(e.value)


def test_public_functions_raise_before_any_device():
    import ssl_amd.metrics as M
    img = np.zeros((100, 100, 3), np.uint8)
    with pytest.raises(ValueError, match="Wrong input_order"):
        M.calculate_niqe(img, 0, input_order="WHC")
    with pytest.raises(ValueError, match="Wrong convert_to"):
        M.calculate_niqe(img, 0, convert_to="luma")
    with pytest.raises(TypeError):
        M.niqe(img)


def test_calculate_metric_still_refuses_niqe():
    import ssl_amd.metrics as M
    a = np.zeros((100, 100, 3), np.uint8)
    with pytest.raises(KeyError, match="calculate_niqe"):
        M.calculate_metric(dict(img=a, img2=a), dict(type="calculate_niqe", crop_border=0))
    with pytest.raises(KeyError, match="calculate_niqe"):
        M.MetricAverager().add_all(None, None, dict(niqe=dict(type="calculate_niqe", crop_border=0)))


# ---------------------------------------------------------------------------------------------- the offline tool ---
def test_offline_tool_text_format(tmp_path, monkeypatch):
    from PIL import Image
    import ssl_amd.metrics as M
    P = params()
    seen = []

    def fake(img, crop_border, input_order='HWC', convert_to='y', **kw):
        seen.append(kw.get("niqe_pris_params"))
        return N.calculate_niqe(img, crop_border, input_order, convert_to, niqe_pris_params=P)

    monkeypatch.setattr(M, "calculate_niqe", fake)
    spec = importlib.util.spec_from_file_location("calculate_niqe_tool", os.path.join(ROOT, "scripts", "calculate_niqe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    folder = tmp_path / "results" / "DIV2K100"
    folder.mkdir(parents=True)
    rng = np.random.default_rng(7)
    want = []
    for name in ("baboon", "zebra_x4"):
        rgb = rng.integers(0, 256, (104, 200, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(folder / f"{name}.png")
        want.append((name, N.calculate_niqe(rgb[..., ::-1], 4, niqe_pris_params=P)))
    (folder / ".hidden").write_text("skipped")
    assert tool.main(["--input", str(folder), "--crop_border", "4", "--params", PARAMS]) == 0
    assert seen == [PARAMS, PARAMS]
    text = (folder.parent / "NIQE_DIV2K100.txt").read_text(encoding="utf-8")
    lines = text.split("\n")
    assert len(lines) == 3 and not text.endswith("\n")
    for line, (name, s) in zip(lines, want):
        assert line == f"{name}. \tNIQE: {s:.6f}"
    assert lines[2] == f"Average NIQE for DIV2K100: {sum(s for _, s in want) / 2:.6f}"


if __name__ == "__main__":
    for k, v in measure(np.load(os.path.join(ROOT, "tests", "golden", "f26_niqe.npz"))).items():
        print(f"{k:10s} {v:.4e}")
