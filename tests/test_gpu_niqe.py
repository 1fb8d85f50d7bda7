"""The NIQE kernels (ssl_amd/csrc/ssg_niqe.hip) on the GPU against the fp64 restatement (niqe_reference.py) and the
reference's recorded planes (golden/f26_niqe.npz): the two planes, the 36 features per block, the score, batching and
reproducibility, the four input kinds, 'gray', the refusal of an image without a block, and the Python layer.

No grid of these kernels is capped (one thread per pixel, one workgroup per tile / per block and scale / per image), so
no grid-stride loop has a second trip to cross.  niqe_fit's loops over the ROWS do (the flags past one workgroup's
threads, the seven row lanes of the column means), and the fixture's six blocks at most reach none of them:
test_gpu_niqe_blocks.py does, on generated inputs.  Every case runs once (module cache); the tests share the results."""
import numpy as np
import pytest
import torch

import metrics_reference as MR
import niqe_reference as N
import test_cpu_niqe as TC

pytestmark = pytest.mark.gpu

U8_HWC, U8_CHW, F32_RGB, F32_PLANE = 1, 2, 0, 3
_CACHE = {}


def _need():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def fixture():
    if "g" not in _CACHE:
        import os
        _CACHE["g"] = np.load(os.path.join(TC.ROOT, "tests", "golden", "f26_niqe.npz"))
    return _CACHE["g"]


def device_input(i):
    """Fixture case i as the C ABI takes it: (contiguous device tensor with a batch axis, kind, crop)."""
    g = fixture()
    img, order, crop = g[f"c{i}_img"], str(g[f"c{i}_order"]), int(g[f"c{i}_crop"])
    if order == 'HW':
        return torch.from_numpy(img.astype(np.float32)).cuda()[None], F32_PLANE, crop
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()[None]
    return t, (U8_CHW if order == 'CHW' else U8_HWC), crop


def run(i):
    """GPU planes, features and score of fixture case i, and the restatement run on the GPU's own planes."""
    key = ("run", i)
    if key not in _CACHE:
        from ssl_amd import metrics as M
        t, kind, crop = device_input(i)
        p1, p2 = M.niqe_planes(t, kind, crop)
        feat = M.niqe_features(t, kind, crop)
        score = M._niqe_run(t, kind, crop, 'y', TC.PARAMS)
        torch.cuda.synchronize()
        p1, p2 = p1[0].cpu().numpy(), p2[0].cpu().numpy()
        rf, rt = N.features_from_planes(p1.astype(np.float64), p2)
        P = TC.params()
        _CACHE[key] = dict(p1=p1, p2=p2, feat=feat[0].cpu().numpy(), score=float(score[0]), rfeat=rf, rt=rt,
                           rfit=N.fit(rf, P["mu_pris_param"], P["cov_pris_param"]))
    return _CACHE[key]


CASES = list(range(8))


@pytest.mark.parametrize("i", CASES)
def test_planes(i):
    """Plane 1 equals the reference's rounded plane bit for bit.  Plane 2 against the restatement on the GPU's plane 1:
    each of the two passes adds 8 products w_t v, |w_t v| <= 0.44 * 1.19 and every partial sum below 1.3, so a pass
    errs by at most 16 roundings of values below 1.3 (8 products, 8 additions): 16 * 1.3 * 2^-53 < 2^-48 each, 2^-47
    for both, times 255 (the scaling adds one more rounding of a value below 255 * 1.3): within 255 * 2^-44."""
    _need()
    g, r = fixture(), run(i)
    want = g[f"c{i}_plane"]
    H1, W1 = want.shape[0] // 96 * 96, want.shape[1] // 96 * 96
    assert r["p1"].dtype == np.float32 and r["p1"].shape == (H1, W1)
    assert np.array_equal(r["p1"].view(np.uint32), want[:H1, :W1].astype(np.float32).view(np.uint32))
    rp2 = N.plane2(r["p1"].astype(np.float64))
    assert r["p2"].dtype == np.float64 and r["p2"].shape == rp2.shape == (H1 // 2, W1 // 2)
    dev = float(np.abs(r["p2"] - rp2).max())
    print(f"c{i} plane 2: max |gpu - restatement| = {dev:.3e}  (bound {255 * 2.0 ** -44:.3e})")
    assert dev <= 255 * 2.0 ** -44


@pytest.mark.parametrize("i", CASES)
def test_features(i):
    _need()
    r = run(i)
    got, want = r["feat"], r["rfeat"]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    margin = N.midpoint_margin(r["rt"])
    assert margin.min() > 1e-9                       # no fit of the fixture within 1e-9 of a midpoint
    assert np.array_equal(got[:, TC.ALPHA], want[:, TC.ALPHA])
    a, b = got[:, TC.OTHER], want[:, TC.OTHER]
    ok = ~np.isnan(b)
    rel = float((np.abs(a - b)[ok] / np.abs(b[ok])).max())
    print(f"c{i} features: max relative deviation {rel:.3e}  (bound 1e-10), min midpoint margin {margin.min():.3e}")
    assert rel <= 1e-10


@pytest.mark.parametrize("i", CASES)
def test_score(i):
    _need()
    g, r = fixture(), run(i)
    if np.isnan(float(g[f"c{i}_score"])):
        assert np.isnan(r["score"]) and np.isnan(r["rfit"]["score"])
        return
    q2, want = r["score"] ** 2, r["rfit"]["q2"]
    bound = 64 * r["rfit"]["cond"] * 2.2e-16 * want
    print(f"c{i} score {r['score']:.9f} reference {float(g[f'c{i}_score']):.9f}: |q2 - q2_restatement| / q2 = "
          f"{abs(q2 - want) / want:.3e}  (bound {bound / want:.3e}, cond {r['rfit']['cond']:.3e})")
    assert abs(q2 - want) <= bound
    # and the reference's own float32 result, by the margin measured on the CPU
    ref = float(g[f"c{i}_score"])
    assert abs(r["score"] - ref) <= TC.FACTOR * TC.MEASURED["score_rel"] * ref


def _grey_batch():
    g = fixture()
    rng = np.random.default_rng(266)
    imgs = [g["c6_img"], rng.integers(0, 256, (192, 192, 1), dtype=np.uint8),
            np.clip(rng.normal(128, 40, (192, 192, 1)), 0, 255).astype(np.uint8)]
    return torch.from_numpy(np.stack(imgs)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def test_batch_equals_single_calls_and_repeats_bit_for_bit():
    _need()
    from ssl_amd import metrics as M
    batch = _grey_batch()

    def all_of(t):
        return (M._niqe_run(t, U8_HWC, 0, 'y', TC.PARAMS), M.niqe_features(t, U8_HWC, 0), *M.niqe_planes(t, U8_HWC, 0))

    whole, again = all_of(batch), all_of(batch)
    singles = [all_of(batch[k:k + 1].contiguous()) for k in range(3)]
    torch.cuda.synchronize()
    assert int(torch.isnan(whole[1][0]).any(1).sum()) == 1 and not bool(torch.isnan(whole[0]).any())
    for a, b in zip(whole, again):
        assert torch.equal(_bits(a), _bits(b))
    for k in range(3):
        for a, b in zip(whole, singles[k]):
            assert torch.equal(_bits(a[k:k + 1]), _bits(b)), k
    assert len({float(v) for v in whole[0]}) == 3


def test_kinds_reach_the_same_plane_and_score():
    """The four kinds: HWC / CHW / plane come from the fixture (cases 0, 3, 4); here the float RGB tensor of case 5
    against its own tensor2img image, and the HWC image handed over as CHW."""
    _need()
    from ssl_amd import metrics as M
    g = fixture()
    x = torch.from_numpy(g["c5_x"].astype(np.float32)).cuda()[None]
    p1, p2 = M.niqe_planes(x, F32_RGB, 0)
    s = M._niqe_run(x, F32_RGB, 0, 'y', TC.PARAMS)
    chw = torch.from_numpy(np.ascontiguousarray(g["c5_img"].transpose(2, 0, 1))).cuda()[None]
    s_chw = M._niqe_run(chw, U8_CHW, 0, 'y', TC.PARAMS)
    torch.cuda.synchronize()
    r = run(5)
    assert np.array_equal(p1[0].cpu().numpy(), r["p1"]) and np.array_equal(p2[0].cpu().numpy(), r["p2"])
    assert float(s[0]) == r["score"] == float(s_chw[0])
    assert {device_input(i)[1] for i in (0, 3, 4)} == {U8_HWC, U8_CHW, F32_PLANE}


def test_gray_is_the_documented_formula():
    _need()
    from ssl_amd import metrics as M
    g = fixture()
    img = g["c2_img"]
    t = torch.from_numpy(img).cuda()[None]
    p1, p2 = M.niqe_planes(t, U8_HWC, 4, 'gray')
    got = M.calculate_niqe(img, 4, convert_to='gray', niqe_pris_params=TC.PARAMS)
    want_p1 = N.plane1(img, 4, 'HWC', 'gray')
    assert np.array_equal(p1[0].cpu().numpy().astype(np.float64), want_p1)
    assert not np.array_equal(want_p1, N.plane1(img, 4, 'HWC', 'y'))
    P = TC.params()
    want = N.niqe(img, 4, P["mu_pris_param"], P["cov_pris_param"], 'HWC', 'gray')
    assert abs(got ** 2 - want["q2"]) <= 64 * want["cond"] * 2.2e-16 * want["q2"]


def test_image_without_a_block_is_refused():
    _need()
    from ssl_amd import metrics as M
    with pytest.raises(RuntimeError, match=r"status -4"):
        M.calculate_niqe(np.zeros((95, 200, 3), np.uint8), 0, niqe_pris_params=TC.PARAMS)
    with pytest.raises(RuntimeError, match=r"status -4"):
        M.calculate_niqe(np.zeros((103, 200, 3), np.uint8), 4, niqe_pris_params=TC.PARAMS)


def test_python_layer():
    """calculate_niqe on the fixture's arrays in their own input orders; niqe on a device tensor agrees with
    calculate_niqe on tensor2img's image and, once the parameters are on the device, does not synchronise with the
    host; MetricAverager.add_niqe over two image sizes."""
    _need()
    from ssl_amd import metrics as M
    g = fixture()
    for i in (0, 3, 4):
        s = M.calculate_niqe(g[f"c{i}_img"], int(g[f"c{i}_crop"]), input_order=str(g[f"c{i}_order"]),
                             niqe_pris_params=TC.PARAMS)
        assert isinstance(s, float) and s == run(i)["score"], i
    x = torch.from_numpy(g["c5_x"].astype(np.float32)).cuda()
    first = M.niqe(x, niqe_pris_params=TC.PARAMS)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = M.niqe(x, niqe_pris_params=TC.PARAMS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (1,)
    assert float(out[0]) == float(first[0]) == M.calculate_niqe(MR.quantise(g["c5_x"].astype(np.float32)), 0,
                                                                niqe_pris_params=TC.PARAMS)
    y = torch.from_numpy(np.ascontiguousarray(g["c2_img"][..., ::-1].transpose(2, 0, 1)).astype(np.float32) / 255).cuda()
    avg = M.MetricAverager()
    avg.add_niqe("niqe", x, niqe_pris_params=TC.PARAMS)
    avg.add_niqe("niqe", y[None], crop_border=4, niqe_pris_params=TC.PARAMS)
    res = avg.result()
    assert set(res) == {"niqe"}
    assert res["niqe"] == pytest.approx((run(5)["score"] + run(2)["score"]) / 2, rel=1e-15)


def poison_cases():
    """What the LDS-poison test runs on the product build and again on the poisoned profiling build: score, features and
    both planes of the 2 x 3 block image with remainders, of the float plane, and of the batch with the NaN row."""
    from ssl_amd import metrics as M
    out = []
    for t, kind, crop in (device_input(2), device_input(4), (_grey_batch(), U8_HWC, 0)):
        out.append(M._niqe_run(t, kind, crop, 'y', TC.PARAMS))
        out.append(M.niqe_features(t, kind, crop))
        out += list(M.niqe_planes(t, kind, crop))
    torch.cuda.synchronize()
    return out
