"""LPIPS and DISTS without a GPU: the restatement against a second formulation, the packages' fp32 torch lines within
the wider bound, the networks' shapes, both key layouts, the constants, the search for weights, the dispatch of
calculate_metric, and the reference's two functions on CPU tensors against the restatement on the same network's
features."""
import numpy as np
import pytest
import torch

import featmetric_cases as C
import featmetric_reference as R
from ssl_amd import metrics, metrics_feat as MF

UNIT, CHUNK, CAP = 256, 8192, 4            # (a small cap keeps the CPU cases small; the GPU tests use the library's)


@pytest.fixture(scope="module")
def lpips_sets():
    return [(name, C.lpips_maps(N, layers, content)) for name, N, layers, content in C.lpips_cases(UNIT, CAP)]


@pytest.fixture(scope="module")
def dists_sets():
    return [(name, C.dists_maps(N, layers, content)) for name, N, layers, content in C.dists_cases(CHUNK)]


@pytest.fixture(scope="module")
def nets():
    """random-weight networks on the CPU, built once: (LPIPS alex, LPIPS vgg, DISTS)"""
    return (MF.LPIPS('alex', C.lpips_state('alex')[0]), MF.LPIPS('vgg', C.lpips_state('vgg')[0]),
            MF.DISTS(C.dists_state()[0]))


def test_lpips_restatement_against_second_formulation(lpips_sets):
    for name, (f0, f1, w) in lpips_sets:
        ref = R.lpips(f0, f1, w)
        assert R.share(R.lpips_second(f0, f1, w), ref.layers, ref.layers_bound) <= 1.0, name
        if "identical" in name:
            assert (ref.layers == 0).all()


def test_dists_restatement_against_second_formulation(dists_sets):
    for name, (x, y, a, b) in dists_sets:
        ref = R.dists(x, y, a, b)
        assert np.isfinite(ref.score_bound).all(), name
        assert R.share(R.dists_second(x, y, a, b), ref.score, ref.score_bound) <= 1.0, name
        if "same" in name:
            assert (np.abs(ref.score) <= ref.score_bound).all()
        one = [S2[:, :] for S2, xs in zip(ref.S2, x) if xs.shape[2] * xs.shape[3] == 1]
        assert bool(one) == ("edges" in name) and all((s == 1).all() for s in one), name   # a one-element plane: S2 = 1


def test_torch_lines_within_the_wider_bound(lpips_sets, dists_sets):
    for name, (f0, f1, w) in lpips_sets:
        ref = R.lpips(f0, f1, w)
        got = MF.lpips_torch_lines(f0, f1, [t.reshape(1, -1, 1, 1) for t in w]).reshape(-1)
        share = R.share(got, ref.value, ref.torch_value_bound)
        print(f"lpips {name}: torch's fp32 lines (CPU) use {share:.3g} of the wider bound")
        assert share <= 1.0, name
    for name, (x, y, a, b) in dists_sets:
        ref = R.dists(x, y, a, b)
        got = MF.dists_torch_lines(x, y, a.reshape(1, -1, 1, 1), b.reshape(1, -1, 1, 1))
        share = R.share(got, ref.score, ref.torch_score_bound)
        print(f"dists {name}: torch's fp32 lines (CPU) use {share:.3g} of the wider bound "
              f"(largest bound {float(ref.torch_score_bound.max()):.3g})")
        assert share <= 1.0, name


@pytest.mark.parametrize("shape", C.IMAGE_SHAPES)
def test_network_shapes(nets, shape):
    alex, vgg, dists = nets
    x = C.images(shape)[0]
    N, _, H, W = shape
    with torch.no_grad():
        fa, fv, fd = alex.features(x * 2 - 1), vgg.features(x * 2 - 1), dists.features(x)
    h, w = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    want = [(h, w)]
    h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    want.append((h, w))
    want += [((h - 3) // 2 + 1, (w - 3) // 2 + 1)] * 3
    assert [tuple(f.shape) for f in fa] == [(N, c, a, b) for c, (a, b) in zip(C.ALEX_CHANNELS, want)]
    assert [tuple(f.shape) for f in fv] == [(N, c, H >> s, W >> s) for s, c in enumerate(C.VGG_CHANNELS)]
    sizes, (a, b) = [(H, W)], (H, W)
    for _ in range(4):
        a, b = (a + 2 - 3) // 2 + 1, (b + 2 - 3) // 2 + 1
        sizes.append((a, b))
    assert [tuple(f.shape) for f in fd] == [shape] + [(N, c, a, b) for c, (a, b) in zip(C.VGG_CHANNELS, sizes)]
    with torch.no_grad():
        assert alex(x, x, normalize=True).shape == (N, 1, 1, 1) and dists(x, x).shape == (N,)


def _same_parameters(a, b):
    pa, pb = dict(a.state_dict()), dict(b.state_dict())
    assert pa.keys() == pb.keys() and len(pa) > 5
    return all(torch.equal(pa[k].view(torch.int32), pb[k].view(torch.int32)) for k in pa)


def test_both_key_layouts_load_to_equal_modules(nets, tmp_path):
    for net, built in (('alex', nets[0]), ('vgg', nets[1])):
        package, trunk, small = C.lpips_state(net)
        assert _same_parameters(built, MF.LPIPS(net, (trunk, small)))
        torch.save(trunk, tmp_path / f"{net}_trunk.pth"), torch.save(small, tmp_path / f"{net}_lin.pth")
        assert _same_parameters(built, MF.LPIPS(net, (str(tmp_path / f"{net}_trunk.pth"), str(tmp_path / f"{net}_lin.pth"))))
    package, trunk, small = C.dists_state()
    assert _same_parameters(nets[2], MF.DISTS((trunk, small)))
    with pytest.raises(KeyError):
        MF.LPIPS('alex', C.lpips_state('alex')[1])            # a trunk without the lin layers
    with pytest.raises(ValueError):
        MF.LPIPS('alex', C.lpips_state('vgg')[0])             # another network's weights


def test_environment_variable_names_the_weights(nets, tmp_path, monkeypatch):
    package, trunk, small = C.dists_state()
    torch.save(trunk, tmp_path / "t.pth"), torch.save(small, tmp_path / "s.pth")
    import os
    monkeypatch.setenv(MF.DISTS_WEIGHTS_ENV, str(tmp_path / "t.pth") + os.pathsep + str(tmp_path / "s.pth"))
    assert _same_parameters(nets[2], MF.DISTS())
    torch.save(C.lpips_state('alex')[0], tmp_path / "a.pth")
    monkeypatch.setenv(MF.LPIPS_WEIGHTS_ENV, str(tmp_path / "a.pth"))
    assert _same_parameters(nets[0], MF.LPIPS('alex'))


def test_constants(nets):
    a = np.hanning(5)[1:-1]
    g = np.outer(a, a) / np.outer(a, a).sum()
    pool = MF.L2pooling(channels=7)
    assert pool.filter.shape == (7, 1, 3, 3) and pool.padding == 1 and pool.stride == 2
    assert np.allclose(pool.filter[3, 0].numpy(), g, rtol=0, atol=1e-7) and abs(float(pool.filter[0].sum()) - 1) < 1e-6
    x = torch.rand(1, 7, 6, 5)
    want = (torch.nn.functional.conv2d(x ** 2, pool.filter, stride=2, padding=1, groups=7) + 1e-12).sqrt()
    assert torch.equal(pool(x), want) and want.shape == (1, 7, 3, 3)
    s = MF.ScalingLayer()
    assert s.shift.reshape(-1).tolist() == torch.Tensor([-.030, -.088, -.188]).tolist()
    assert s.scale.reshape(-1).tolist() == torch.Tensor([.458, .448, .450]).tolist()
    assert torch.equal(s(x[:, :3]), (x[:, :3] - s.shift) / s.scale)
    d = nets[2]
    assert d.mean.reshape(-1).tolist() == torch.tensor([0.485, 0.456, 0.406]).tolist()
    assert d.std.reshape(-1).tolist() == torch.tensor([0.229, 0.224, 0.225]).tolist()
    assert sum(isinstance(m, MF.L2pooling) for m in d.net) == 4 and d.alpha.shape == (1, 1475, 1, 1)
    assert not any(isinstance(m, torch.nn.MaxPool2d) for m in d.net)
    assert not any(p.requires_grad for p in d.parameters()) and not d.train().training


def test_file_not_found_with_every_source_absent(monkeypatch, tmp_path):
    monkeypatch.delenv(MF.LPIPS_WEIGHTS_ENV, raising=False)
    monkeypatch.delenv(MF.DISTS_WEIGHTS_ENV, raising=False)
    monkeypatch.setattr(MF, "_package_file", lambda *a: None)
    monkeypatch.setattr(MF, "_hub_trunk", lambda net: None)
    for build, env in ((lambda: MF.LPIPS('alex'), MF.LPIPS_WEIGHTS_ENV), (lambda: MF.LPIPS('vgg'), MF.LPIPS_WEIGHTS_ENV),
                       (lambda: MF.DISTS(), MF.DISTS_WEIGHTS_ENV)):
        with pytest.raises(FileNotFoundError) as err:
            build()
        assert env in str(err.value) and "weights=" in str(err.value) and "Nothing is downloaded" in str(err.value)
    with pytest.raises(FileNotFoundError):
        metrics.calculate_metric(dict(img=np.zeros((40, 40, 3), np.uint8), img2=np.zeros((40, 40, 3), np.uint8)),
                                 dict(type='calculate_lpips', crop_border=4))


def _bgr_pair(shape=(45, 67, 3), seed=5):
    gen = np.random.default_rng(seed)
    gt = gen.integers(0, 256, shape, dtype=np.uint8)
    sr = np.clip(gt.astype(np.int32) + gen.integers(-20, 21, shape), 0, 255).astype(np.uint8)
    return sr, gt


@pytest.fixture
def on_cpu(monkeypatch):
    """the functions' own choice of device (the GPU where there is one) set to the CPU"""
    monkeypatch.setattr(MF, "_device", lambda: torch.device("cpu"))


@pytest.mark.parametrize("crop", [0, 4])
def test_reference_functions_on_cpu_against_the_restatement(nets, crop, on_cpu):
    alex, _, dists = nets
    sr, gt = _bgr_pair()
    aw, dw = C.lpips_state('alex')[0], C.dists_state()[0]
    cut = (lambda a: a[crop:-crop, crop:-crop]) if crop else (lambda a: a)
    rgb = lambda a: torch.from_numpy(np.ascontiguousarray(cut(a)[:, :, ::-1].transpose(2, 0, 1))).float()[None] / 255
    unit = lambda a: (torch.from_numpy(np.ascontiguousarray(
        (cut(a).astype(np.float64) / 255.)[:, :, ::-1].transpose(2, 0, 1))).float()[None] - 0.5) / 0.5
    with torch.no_grad():
        f_sr, f_gt = alex.features(unit(sr)), alex.features(unit(gt))
        d_sr, d_gt = dists.features(rgb(sr)), dists.features(rgb(gt))
    ref = R.lpips(f_sr, f_gt, list(alex.lins))
    got = metrics.calculate_lpips(sr, gt, crop, lpips_weights=aw)
    assert abs(got - ref.value[0]) <= ref.torch_value_bound[0]
    assert got == metrics.calculate_metric(dict(img=sr, img2=gt), dict(type='calculate_lpips', crop_border=crop, lpips_weights=aw))
    assert got == metrics.calculate_lpips(sr.transpose(2, 0, 1), gt.transpose(2, 0, 1), crop, input_order='CHW', lpips_weights=aw)
    ref = R.dists(d_gt, d_sr, dists.alpha, dists.beta)
    got = metrics.calculate_dists(sr, gt, crop, dists_weights=dw)
    assert abs(got - ref.score[0]) <= ref.torch_score_bound[0]
    assert got == metrics.calculate_metric(dict(img=sr, img2=gt), dict(type='calculate_dists', crop_border=crop, dists_weights=dw))
    # one network per weights source, not one per call: calculate_metric, which copies its options, included
    built = len(MF._models)
    for _ in range(2):
        metrics.calculate_metric(dict(img=sr, img2=gt), dict(type='calculate_lpips', crop_border=crop, lpips_weights=aw))
        metrics.calculate_metric(dict(img=sr, img2=gt), dict(type='calculate_dists', crop_border=crop, dists_weights=dw))
        metrics.calculate_lpips(sr, gt, crop, lpips_weights=aw)
    assert len(MF._models) == built
    assert sum(k[2] == "cpu" and k[3] in (id(aw), id(dw)) for k in MF._models) == 2


def test_kernel_wrappers_refuse_cpu_and_other_types_whatever_the_flag():
    """nothing but fp32 GPU tensors reaches the C ABI, with set_native_criteria on or off (no GPU is needed to refuse)"""
    from ssl_amd.losses import set_native_criteria
    f, w = torch.rand(1, 4, 3, 3), torch.rand(4)
    for flag in (True, False):
        prev = set_native_criteria(flag)
        try:
            for t in (f, f.half(), f.double(), f.bfloat16()):
                with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                    MF.lpips_layers([t], [t], [w])
                with pytest.raises(ValueError, match="fp32 tensors on one GPU"):
                    MF.dists_score([t], [t], w, w)
        finally:
            set_native_criteria(prev)


def test_refusals_and_dispatch():
    sr, gt = _bgr_pair()
    aw = C.lpips_state('alex')[0]
    with pytest.raises(ValueError, match="test_y_channel"):
        metrics.calculate_lpips(sr, gt, 4, test_y_channel=True, lpips_weights=aw)
    with pytest.raises(ValueError, match="input_order"):
        metrics.calculate_lpips(sr, gt, 4, input_order='WHC', lpips_weights=aw)
    with pytest.raises(AssertionError):
        metrics.calculate_lpips(sr, gt[1:], 4, lpips_weights=aw)
    with pytest.raises(KeyError, match="calculate_fid"):
        metrics.calculate_metric(dict(img=sr, img2=gt), dict(type='calculate_fid'))
    for name in ("calculate_lpips", "calculate_dists", "lpips_dists", "LPIPS", "DISTS"):
        assert name in metrics.__all__ and getattr(metrics, name) is getattr(MF, name)
    assert hasattr(metrics.MetricAverager, "add_lpips") and hasattr(metrics.MetricAverager, "add_dists")


def test_batched_call_and_averager_on_cpu_tensors(on_cpu):
    aw, dw = C.lpips_state('alex')[0], C.dists_state()[0]
    sr, gt = C.images((2, 3, 48, 40))
    out = metrics.lpips_dists(sr, gt, crop_border=4, lpips_weights=aw, dists_weights=dw)
    assert out.shape == (2, 2) and out.dtype == torch.float64 and bool(torch.isfinite(out).all())
    alone = metrics.lpips_dists(sr[1], gt[1], crop_border=4, lpips_weights=aw, dists_weights=dw)
    assert torch.allclose(alone[0], out[1], rtol=1e-5, atol=1e-7)
    avg = metrics.MetricAverager()
    avg.add_lpips("lpips", sr, gt, crop_border=4, lpips_weights=aw)
    avg.add_dists("dists", sr, gt, crop_border=4, dists_weights=dw)
    res = avg.result()
    assert abs(res["lpips"] - float(out[:, 0].mean())) < 1e-12 and abs(res["dists"] - float(out[:, 1].mean())) < 1e-12
    zero = metrics.lpips_dists(gt, gt, lpips_weights=aw, dists_weights=dw)
    assert float(zero[:, 0].abs().max()) == 0.0 and float(zero[:, 1].abs().max()) < 1e-5


def test_offline_scripts_write_the_reference_lines(tmp_path, on_cpu):
    import importlib.util
    import os
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / "Set" / "GT").mkdir(parents=True), (tmp_path / "out" / "vis").mkdir(parents=True)
    pairs = {}
    for i, name in enumerate(("baboon", "zebra")):
        sr, gt = _bgr_pair((40, 52, 3), seed=i)
        Image.fromarray(gt[..., ::-1]).save(tmp_path / "Set" / "GT" / f"{name}.png")
        Image.fromarray(sr[..., ::-1]).save(tmp_path / "out" / "vis" / f"{name}_x4.png")
        pairs[name] = (sr, gt)
    aw, dw = C.lpips_state('alex')[0], C.dists_state()[0]
    torch.save(aw, tmp_path / "alex.pth"), torch.save(dw, tmp_path / "dists.pth")
    for kind, wfile, fn, opt, last in (("LPIPS", "alex.pth", metrics.calculate_lpips, dict(lpips_weights=aw), "Average: LPIPS: "),
                                       ("DISTS", "dists.pth", metrics.calculate_dists, dict(dists_weights=dw),
                                        f"DISTS for {tmp_path / 'Set' / 'GT'} is: ")):
        spec = importlib.util.spec_from_file_location(f"calculate_{kind.lower()}_script",
                                                      os.path.join(root, "scripts", f"calculate_{kind.lower()}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.main(["--gt", str(tmp_path / "Set" / "GT"), "--restored", str(tmp_path / "out" / "vis"), "--suffix", "_x4",
                         "--weights", str(tmp_path / wfile)]) == 0
        text = (tmp_path / "out" / f"{kind}_Set.txt").read_text(encoding="utf-8").split("\n")
        want = [fn(*pairs[n], 4, **opt) for n in ("baboon", "zebra")]
        assert text[:2] == [f"{n:25}. \t{kind}: {v:.6f}." for n, v in zip(("baboon", "zebra"), want)]
        assert text[2] == last + f"{sum(want) / 2:.6f}" and len(text) == 3
