"""The metric kernels (ssl_amd/csrc/ssg_metrics.hip) on the MI355X against the numpy restatement (metrics_reference.py)
on the inputs of metrics_cases.py: the planes bit for bit, the squared-difference sums exactly (integers) or to the
bound of a sum of N non-negative terms (Y), PSNR to 1e-12 dB of 10 log10 of those sums, SSIM to the restatement's derived
bound; then metric_planes past one trip of its capped grid, determinism (repeat, side stream, HIP graph, whatever the
workspace held), the averager, the public functions on the fixture and the refusals with real device pointers."""
import ctypes
import math

import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
CASES = MC.cases()
IDS = [c.name for c in CASES]


def _dev(x):
    return torch.as_tensor(x, device=DEV).contiguous()


def _run(case):
    from ssl_amd import metrics as M
    B, C, H, W = MC.geometry(case)
    out = M._run(_dev(case.a), _dev(case.b), case.kind, B, C, H, W, case.crop, case.y)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_planes_equal_restatement(index):
    from ssl_amd import metrics as M
    case = CASES[index]
    ref = MC.reference(index)
    for which, key in ((0, "planes_a"), (1, "planes_b")):
        got = M.metric_planes(_dev(case.a if which == 0 else case.b), case.kind, case.crop, case.y).cpu()
        want = torch.from_numpy(np.stack([m[key] for m in ref]))
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


_worst = {"ratio": 0.0, "case": None}


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_psnr_ssim_against_restatement(index):
    case = CASES[index]
    ref = MC.reference(index)
    out = _run(case)
    assert out.shape == (len(ref), 4)
    for row, m in zip(out, ref):
        psnr, ssim, sq, n = (float(v) for v in row)
        assert n == m["n"]
        if not case.y:
            assert m["sq_exact"] is not None and sq == float(m["sq_exact"])      # counted in integers: exact
        else:
            assert abs(sq - m["sq_sum"]) <= (m["n"] + 3) * U * m["sq_sum"], (sq, m["sq_sum"])
        if sq == 0.0:
            assert psnr == math.inf and m["psnr"] == math.inf
        else:
            want = 10.0 * math.log10(255.0 * 255.0 / (sq / n))
            assert abs(psnr - want) <= 1e-12, (psnr, want)
            assert abs(psnr - m["psnr"]) <= 1e-9
        err = abs(ssim - m["ssim"])
        ratio = err / m["bound"]
        if ratio > _worst["ratio"]:
            _worst.update(ratio=ratio, case=case.name)
        print(f"{case.name}: |SSIM - SSIM64| = {err:.3e}, bound {m['bound']:.3e}, ratio {ratio:.3e}; worst so far "
              f"{_worst['ratio']:.3e} ({_worst['case']})")
        assert err <= m["bound"], (ssim, m["ssim"], m["bound"])
        if case.name.startswith("identical"):
            assert ssim == 1.0


def _plane_trip_inputs():
    """Two inputs with more than 4,096 x 256 = 1,048,576 plane elements: metric_planes' grid is capped there and every
    thread walks on by gridDim.x * 256.  Outside metrics_cases.cases(): no SSIM restatement is needed for the planes."""
    rng = np.random.default_rng(4096)
    q = rng.integers(0, 256, (3, 600, 600), dtype=np.uint8)                              # BGR planes
    x = rng.random((3, 1032, 1032), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
    return (("u8_chw_600", MC.U8_CHW, 0, False, q[None], R.planes(q.transpose(1, 2, 0), 0, False)),
            ("f32_y_1032_crop1", MC.F32_RGB, 1, True, x[None], R.planes(R.quantise(x), 1, True)))


@pytest.mark.parametrize("which", [0, 1], ids=["u8_chw_600", "f32_y_1032_crop1"])
def test_planes_past_one_grid_trip(which):
    from ssl_amd import metrics as M
    name, kind, crop, y, img, want = _plane_trip_inputs()[which]
    assert want.size > 4096 * 256
    got = M.metric_planes(_dev(img), kind, crop, y).cpu()
    want = torch.from_numpy(want[None])
    assert got.dtype == torch.float32 and got.shape == want.shape
    differing = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"TRIP planes {name}: {want.numel()} elements, {differing} differing")
    assert differing == 0


def test_fixture_through_public_functions(golden):
    from ssl_amd import metrics as M
    g = golden("f24_metrics")
    for i in range(int(g["n_cases"])):
        a, b = g[f"c{i}_a"], g[f"c{i}_b"]
        for k in range(int(g["n_configs"])):
            crop, y = (int(v) for v in g[f"c{i}_cfg{k}"])
            want_p, want_s = float(g[f"c{i}_psnr{k}"]), float(g[f"c{i}_ssim{k}"])
            bound = R.metrics(a, b, crop, bool(y))["bound"]
            opt = dict(crop_border=crop, test_y_channel=bool(y))
            calls = [(M.calculate_psnr(a, b, **opt), M.calculate_ssim(a, b, **opt)),
                     (M.calculate_psnr(_dev(a), _dev(b), **opt), M.calculate_ssim(_dev(a), _dev(b), **opt)),
                     (M.calculate_metric(dict(img=a, img2=b), dict(type="calculate_psnr", **opt)),
                      M.calculate_metric(dict(img=a, img2=b), dict(type="calculate_ssim", **opt)))]
            if a.ndim == 3:      # the same image as (C,H,W), and as the float image the offline script passes
                ac, bc = np.ascontiguousarray(a.transpose(2, 0, 1)), np.ascontiguousarray(b.transpose(2, 0, 1))
                calls.append((M.calculate_psnr(ac, bc, input_order='CHW', **opt),
                              M.calculate_ssim(ac, bc, input_order='CHW', **opt)))
            af, bf = a.astype(np.float32) / 255. * 255, b.astype(np.float32) / 255. * 255
            calls.append((M.calculate_psnr(af, bf, **opt), M.calculate_ssim(af, bf, **opt)))
            if f"c{i}_xa" in g.files:    # the model's tensors: tensor2img dropped
                xa, xb = _dev(g[f"c{i}_xa"]), _dev(g[f"c{i}_xb"])
                calls.append((M.calculate_metric(dict(img=xa, img2=xb), dict(type="calculate_psnr", **opt)),
                              M.calculate_metric(dict(img=xa[None], img2=xb[None]), dict(type="calculate_ssim", **opt))))
                both = M.psnr_ssim(xa.half()[None], xb.half()[None], crop, bool(y))      # fp16 is cast
                assert both.shape == (1, 2) and both.dtype == torch.float64 and both.is_cuda
                pair = M.psnr_ssim(xa[None], xb[None], crop, bool(y)).cpu()
                calls.append((float(pair[0, 0]), float(pair[0, 1])))
            for p, s in calls:
                assert isinstance(p, float) and isinstance(s, float)
                assert abs(p - want_p) <= 1e-9 * want_p, (i, k, p, want_p)
                assert abs(s - want_s) <= bound, (i, k, s, want_s, bound)


# ------------------------------------------------------------------------------------------------ determinism ---
class Raw:
    """ssg_psnr_ssim through the C ABI with preallocated output and workspace, on torch's current stream."""

    def __init__(self, case):
        from ssl_amd import _lib
        self.L = _lib.lib()
        self.case = case
        self.geom = MC.geometry(case)
        self.nb = self.L.ssg_metric_workspace_bytes(*self.geom, case.crop)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out = torch.zeros((self.geom[0], 4), dtype=torch.float64, device=DEV)

    def __call__(self, a, b):
        rc = self.L.ssg_psnr_ssim(a.data_ptr(), b.data_ptr(), self.case.kind, *self.geom, self.case.crop,
                                  int(self.case.y), self.out.data_ptr(), self.ws.data_ptr(), self.nb,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc


def _named(name):
    return CASES[IDS.index(name)]


@pytest.mark.parametrize("name", ["many_tiles_second_trip", "floats_outside_unit", "cross_hwc_c3_y1_b3"])
def test_repeat_and_side_stream_bit_equal(name):
    case = _named(name)
    a, b = _dev(case.a), _dev(case.b)
    first, again, side_call = Raw(case), Raw(case), Raw(case)
    first(a, b)
    again(a, b)
    torch.cuda.synchronize()
    assert torch.equal(first.out, again.out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        side_call(a, b)
    side.synchronize()
    assert torch.equal(first.out, side_call.out)


@pytest.mark.parametrize("name", ["batch_second_trip", "cross_hwc_c3_y1_b3"])
def test_result_ignores_what_the_workspace_held(name):
    """Every partial the fold reads was written by this call's metric_tiles: a workspace of 0xFF bytes (NaN as fp64,
    2^64 - 1 as a count) and one of zeros give the same bits, with 512 workgroups for 663 tiles and with one per tile."""
    case = _named(name)
    assert (MC.tiles(case) > 512) == (name == "batch_second_trip")
    a, b = _dev(case.a), _dev(case.b)
    outs = []
    for byte in (0xFF, 0x00):
        raw = Raw(case)
        raw.ws.fill_(byte)
        raw(a, b)
        torch.cuda.synchronize()
        outs.append(raw.out.clone())
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))


def test_replays_as_hip_graph():
    """One capture, replayed over three input batches written into the captured buffers: each replay equals the eager
    call on that batch bit for bit."""
    case = _named("floats_outside_unit")
    gen = torch.Generator().manual_seed(7)
    batches = [(torch.rand(case.a.shape, generator=gen) * 1.2 - 0.1, torch.rand(case.a.shape, generator=gen))
               for _ in range(3)]
    a, b = _dev(case.a).clone(), _dev(case.b).clone()
    eager, rec = Raw(case), Raw(case)
    eager(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec(a, b)
    for xa, xb in batches:
        a.copy_(xa)
        b.copy_(xb)
        eager(a, b)
        torch.cuda.synchronize()
        want = eager.out.clone()
        rec.out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rec.out, want)
        assert bool((want[:, 1] < 0.5).all())      # unrelated noise images: the replay saw the new batch


def test_averager_equals_mean_of_single_calls():
    from ssl_amd import metrics as M
    gen = torch.Generator().manual_seed(11)
    shapes = [(3, 24, 31), (3, 24, 31), (3, 40, 23), (3, 19, 52), (3, 40, 23)]
    opts = dict(psnr=dict(type="calculate_psnr", crop_border=4, test_y_channel=True),
                ssim=dict(type="calculate_ssim", crop_border=4, test_y_channel=True))
    avg, single, one_by_one = M.MetricAverager(), dict(psnr=0.0, ssim=0.0), M.MetricAverager()
    for idx, shape in enumerate(shapes):
        gt = torch.rand(shape, generator=gen).to(DEV)
        sr = (gt + 0.03 * torch.randn(shape, generator=gen).to(DEV))
        avg.add_all(sr[None], gt[None], opts)
        for name, opt in opts.items():
            one_by_one.add(name, sr, gt, **opt)
            single[name] += M.calculate_metric(dict(img=sr, img2=gt), opt)
    for name in single:
        single[name] /= idx + 1
    assert avg.result() == single
    assert one_by_one.result() == single
    assert M.MetricAverager().result() == {}


# --------------------------------------------------------------------------------------------------- refusals ---
def test_refusals_leave_outputs_untouched():
    from ssl_amd import _lib
    from ssl_amd import metrics as M
    L = _lib.lib()
    a = torch.rand((1, 3, 32, 32), device=DEV)
    b = torch.rand((1, 3, 32, 32), device=DEV)
    out = torch.full((1, 4), -7.0, dtype=torch.float64, device=DEV)
    planes = torch.full((1, 3, 32, 32), -7.0, device=DEV)
    nb = L.ssg_metric_workspace_bytes(1, 3, 32, 32, 0)
    ws = torch.full((nb + 16,), 0x5a, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(C=3, H=32, W=32, crop=0, kind=0, wsp=None, n=nb):
        return L.ssg_psnr_ssim(a.data_ptr(), b.data_ptr(), kind, 1, C, H, W, crop, 1, out.data_ptr(),
                               ws.data_ptr() if wsp is None else wsp, n, st)

    assert call(C=2) == -1 and call(C=4) == -1
    assert call(crop=-1) == -1
    assert call(kind=7) == -1
    assert call(crop=11) == -4          # 32 - 22 = 10 < 11
    assert call(H=10) == -4
    assert call(n=nb - 1) == -3
    assert call(wsp=ws.data_ptr() + 8) == -5
    assert L.ssg_metric_planes(a.data_ptr(), 0, 1, 2, 32, 32, 0, 1, planes.data_ptr(), st) == -1
    assert L.ssg_metric_planes(a.data_ptr(), 0, 1, 3, 32, 32, 16, 1, planes.data_ptr(), st) == -4
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((planes == -7.0).all()) and bool((ws == 0x5a).all())
    # the accepted call writes all four values
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != -7.0).all()) and float(out[0, 3]) == 32 * 32
    # the Python layer turns a refusal into an error
    with pytest.raises(RuntimeError):
        M.psnr_ssim(a, b, crop_border=11)
    with pytest.raises(RuntimeError):
        M.psnr_ssim(torch.rand((1, 2, 32, 32), device=DEV), torch.rand((1, 2, 32, 32), device=DEV))


# ------------------------------------------------------------------ shared with test_gpu_metrics_poison.py ----
def poison_cases():
    """What the LDS-poison test runs on the product build and again on the poisoned profiling build: the raw (B,4)
    results and both images' planes of one map pixel, one tile plus one on each axis, floats on Y, and the two kinds of
    second trip (one Y plane; three planes and three images)."""
    from ssl_amd import metrics as M
    out = []
    for name in ("one_map_pixel", "tile_plus_one", "floats_outside_unit", "y_second_trip", "batch_second_trip"):
        case = _named(name)
        a, b = _dev(case.a), _dev(case.b)
        out.append(M._run(a, b, case.kind, *MC.geometry(case), case.crop, case.y))
        out += [M.metric_planes(t, case.kind, case.crop, case.y) for t in (a, b)]
    torch.cuda.synchronize()
    return out
