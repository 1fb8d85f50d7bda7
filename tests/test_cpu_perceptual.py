"""The perceptual loss without a GPU: the extractor against a network spelled out layer by layer, the layer names of
all eight VGG types, both loss classes against the reference's expression written out (the same bits on CPU tensors),
the search for weights, and torch's own fp32 result against the bound tests/perceptual_reference.py derives for it."""
import pytest
import torch
from torch import nn

import perceptual_cases as C
import perceptual_reference as R


def _conv(i, o):
    return nn.Conv2d(i, o, kernel_size=3, stride=1, padding=1)


def _literal_vgg19():
    """torchvision's vgg19().features[:35], written out (train_BSGRAN/models/loss.py:9-47 prints the same list)"""
    return nn.Sequential(
        _conv(3, 64), nn.ReLU(), _conv(64, 64), nn.ReLU(), nn.MaxPool2d(2, 2),                                 # 0 .. 4
        _conv(64, 128), nn.ReLU(), _conv(128, 128), nn.ReLU(), nn.MaxPool2d(2, 2),                             # 5 .. 9
        _conv(128, 256), nn.ReLU(), _conv(256, 256), nn.ReLU(), _conv(256, 256), nn.ReLU(), _conv(256, 256),   # 10 .. 16
        nn.ReLU(), nn.MaxPool2d(2, 2),                                                                         # 17, 18
        _conv(256, 512), nn.ReLU(), _conv(512, 512), nn.ReLU(), _conv(512, 512), nn.ReLU(), _conv(512, 512),   # 19 .. 25
        nn.ReLU(), nn.MaxPool2d(2, 2),                                                                         # 26, 27
        _conv(512, 512), nn.ReLU(), _conv(512, 512), nn.ReLU(), _conv(512, 512), nn.ReLU(), _conv(512, 512))   # 28 .. 34


@pytest.fixture(scope="module")
def state():
    return C.vgg_state_dict("vgg19", seed=0)


@pytest.fixture(scope="module")
def literal_features(state):
    """the features at 2, 7, 16, 25, 34 of the literal network on the fixture images (x, gt), computed once"""
    net = _literal_vgg19()
    net.load_state_dict({k[len("features."):]: v for k, v in state.items()})
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    out = []
    with torch.no_grad():
        for img in C.images():
            h, feats = (img - mean) / std, []
            for i, layer in enumerate(net):
                h = layer(h)
                if i in C.VGG19_TAP_INDICES:
                    feats.append(h)
            out.append(feats)
    return out


def test_layer_names_of_all_eight_types():
    from ssl_amd.losses.perceptual import vgg_layer_names
    n19 = vgg_layer_names("vgg19")
    assert [n19.index(k) for k in C.VGG19_TAPS] == list(C.VGG19_TAP_INDICES)
    want = {"vgg11": (21, {"conv1_1": 0, "pool1": 2, "conv2_1": 3, "conv3_2": 8, "conv5_2": 18, "pool5": 20}),
            "vgg13": (25, {"conv1_2": 2, "pool1": 4, "conv3_2": 12, "conv5_2": 22, "relu5_2": 23}),
            "vgg16": (31, {"conv1_2": 2, "conv3_3": 14, "conv4_3": 21, "conv5_3": 28, "pool5": 30}),
            "vgg19": (37, {"relu1_1": 1, "conv3_4": 16, "relu5_4": 35, "pool5": 36}),
            "vgg11_bn": (29, {"conv1_1": 0, "bn1_1": 1, "relu1_1": 2, "pool1": 3, "conv2_1": 4, "pool5": 28}),
            "vgg13_bn": (35, {"bn1_2": 4, "pool1": 6, "conv5_2": 31}),
            "vgg16_bn": (44, {"conv5_3": 40, "bn5_3": 41, "pool5": 43}),
            "vgg19_bn": (53, {"conv1_2": 3, "conv5_4": 49, "bn5_4": 50, "relu5_4": 51, "pool5": 52})}
    for vgg_type, (count, places) in want.items():
        names = vgg_layer_names(vgg_type)
        assert len(names) == count == len(set(names)), vgg_type
        assert {k: names.index(k) for k in places} == places, vgg_type
    with pytest.raises(ValueError):
        vgg_layer_names("vgg12")


def test_extractor_equals_the_literal_network_and_kair_agrees(state, literal_features):
    from ssl_amd.losses import VGGFeatureExtractor, kair
    ours = VGGFeatureExtractor(list(C.VGG19_TAPS), vgg_weights=state)
    theirs = kair.VGGFeatureExtractor(list(C.VGG19_TAP_INDICES), vgg_weights=state)
    assert not ours.vgg_net.training and not theirs.features.training
    assert all(not p.requires_grad for p in ours.parameters()) and all(not p.requires_grad for p in theirs.parameters())
    assert len(list(ours.parameters())) == 32 and "pool5" not in ours.vgg_net._modules
    for img, want in zip(C.images(), literal_features):
        got = ours(img)
        assert list(got.keys()) == list(C.VGG19_TAPS)
        for a, b, c, shape in zip(got.values(), want, theirs(img), C.vgg_feature_shapes()):
            assert tuple(a.shape) == shape and torch.equal(a, b) and torch.equal(c, b)
            assert float(a.min()) < 0                       # (a conv's output, not yet through its ReLU)
    single = kair.VGGFeatureExtractor(7, vgg_weights=state)(C.images()[0])
    assert torch.equal(single, literal_features[0][1])
    ours.train()
    assert not ours.vgg_net.training


def test_extractor_options(state):
    from ssl_amd.losses import VGGFeatureExtractor
    x = C.images()[0]
    taps = ["relu1_1", "pool1", "conv2_2"]
    plain = VGGFeatureExtractor(taps, vgg_weights=state)(x)
    assert [tuple(v.shape[1:]) for v in plain.values()] == [(64, 32, 32), (64, 16, 16), (128, 16, 16)]
    assert float(plain["relu1_1"].min()) == 0
    nopool = VGGFeatureExtractor(["relu1_1", "conv2_2"], vgg_weights=state, remove_pooling=True)
    assert "pool1" not in nopool.vgg_net._modules and tuple(nopool(x)["conv2_2"].shape) == (2, 128, 32, 32)
    stride1 = VGGFeatureExtractor(taps, vgg_weights=state, pooling_stride=1)(x)
    assert tuple(stride1["pool1"].shape) == (2, 64, 31, 31)
    ranged = VGGFeatureExtractor(taps, vgg_weights=state, range_norm=True)(2 * x - 1)
    raw = VGGFeatureExtractor(taps, vgg_weights=state, use_input_norm=False, range_norm=True)
    assert not hasattr(raw, "mean")
    for k in taps:
        assert torch.allclose(ranged[k], plain[k], atol=1e-5)
    trained = VGGFeatureExtractor(taps, vgg_weights=state, requires_grad=True)
    assert trained.vgg_net.training and all(p.requires_grad for p in trained.parameters())
    bn = VGGFeatureExtractor(["bn1_1", "relu2_1"], "vgg11_bn", vgg_weights=C.vgg_state_dict("vgg11_bn", 3),
                             use_input_norm=False)
    got = bn(x)
    assert float(got["bn1_1"].min()) < 0 and not bn.vgg_net.training
    with pytest.raises(ValueError):
        VGGFeatureExtractor(["relu1_2"], "vgg11", vgg_weights=state)
    with pytest.raises(KeyError, match="features.3.weight"):        # (vgg19's features.3 is a ReLU)
        VGGFeatureExtractor(["conv2_1"], "vgg11", vgg_weights=state)
    with pytest.raises(ValueError, match="another vgg_type"):
        VGGFeatureExtractor(["conv1_1"], vgg_weights=dict(state, **{"features.0.weight": torch.zeros(64, 1, 3, 3)}))


def test_weights_are_searched_in_three_places_and_never_downloaded(state, tmp_path, monkeypatch):
    from ssl_amd.losses import VGGFeatureExtractor
    from ssl_amd.losses.perceptual import VGG_PRETRAIN_PATH, VGG_WEIGHTS_ENV
    monkeypatch.delenv(VGG_WEIGHTS_ENV, raising=False)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError) as err:
        VGGFeatureExtractor(["conv1_2"])
    for way in ("vgg_weights=", VGG_WEIGHTS_ENV, VGG_PRETRAIN_PATH, "Nothing is downloaded"):
        assert way in str(err.value)
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        VGGFeatureExtractor(["conv1_2"], vgg_weights=str(tmp_path / "nowhere.pth"))
    small = {k: v for k, v in state.items() if int(k.split(".")[1]) <= 2}
    x = C.images()[0]
    want = VGGFeatureExtractor(["conv1_2"], vgg_weights=small)(x)["conv1_2"]
    torch.save(small, tmp_path / "by_env.pth")
    monkeypatch.setenv(VGG_WEIGHTS_ENV, str(tmp_path / "by_env.pth"))
    assert torch.equal(VGGFeatureExtractor(["conv1_2"])(x)["conv1_2"], want)
    monkeypatch.delenv(VGG_WEIGHTS_ENV)
    (tmp_path / "experiments" / "pretrained_models").mkdir(parents=True)
    torch.save(small, tmp_path / VGG_PRETRAIN_PATH)
    assert torch.equal(VGGFeatureExtractor(["conv1_2"])(x)["conv1_2"], want)
    assert torch.equal(VGGFeatureExtractor(["conv1_2"], vgg_weights=str(tmp_path / "by_env.pth"))(x)["conv1_2"], want)


def _gram(x):
    n, c, h, w = x.size()
    f = x.view(n, c, w * h)
    return f.bmm(f.transpose(1, 2)) / (c * h * w)


@pytest.mark.parametrize("criterion", ["l1", "l2", "fro"])
@pytest.mark.parametrize("style", [0.0, 0.5])
def test_basicsr_class_on_cpu_is_the_reference_expression(state, literal_features, criterion, style):
    from ssl_amd.losses import PerceptualLoss
    layer_weights = dict(zip(C.VGG19_TAPS, C.KAIR_WEIGHTS))
    crit = PerceptualLoss(layer_weights, perceptual_weight=0.7, style_weight=style, criterion=criterion, vgg_weights=state)
    x, gt = C.images()
    x = x.clone().requires_grad_(True)
    percep, style_loss = crit(x, gt)
    fx, fg = crit.vgg(x), literal_features[1]
    kind = {"l1": "l1", "l2": "mse", "fro": "fro"}[criterion]
    want = R.torch_loop(list(fx.values()), fg, C.KAIR_WEIGHTS, kind, 0.7)
    assert torch.equal(percep, want) and percep.dtype == torch.float32
    if style:
        want_style = R.torch_loop([_gram(v) for v in fx.values()], [_gram(v) for v in fg], C.KAIR_WEIGHTS, kind, style)
        assert torch.equal(style_loss, want_style)
        total = percep + style_loss
        want = want + want_style
    else:
        assert style_loss is None
        total = percep
    g1, = torch.autograd.grad(total, x, retain_graph=True)
    g2, = torch.autograd.grad(want, x)
    assert torch.equal(g1, g2) and float(g1.abs().max()) > 0
    assert crit(x, gt)[0] is not None and PerceptualLoss(layer_weights, perceptual_weight=0, style_weight=1.0,
                                                         vgg_weights=state)(x, gt)[0] is None
    with pytest.raises(NotImplementedError):
        PerceptualLoss(layer_weights, criterion="l3", vgg_weights=state)


@pytest.mark.parametrize("lossfn_type", ["l1", "l2"])
def test_kair_class_on_cpu_is_the_reference_expression(state, literal_features, lossfn_type):
    from ssl_amd.losses import kair
    crit = kair.PerceptualLoss(lossfn_type=lossfn_type, vgg_weights=state)
    assert isinstance(crit.lossfn, nn.L1Loss if lossfn_type == "l1" else nn.MSELoss) and isinstance(crit.vgg, nn.Module)
    x, gt = C.images()
    got = crit(x, gt)
    want = 0.0
    for i, (a, b) in enumerate(zip(literal_features[0], literal_features[1])):
        want += C.KAIR_WEIGHTS[i] * crit.lossfn(a, b)
    assert torch.equal(got, want)
    single = kair.PerceptualLoss(feature_layer=7, lossfn_type=lossfn_type, vgg_weights=state)
    assert torch.equal(single(x, gt), 0.0 + crit.lossfn(literal_features[0][1], literal_features[1][1]))
    crit.lossfn = nn.SmoothL1Loss()                    # (a replaced criterion is applied as given)
    want = 0.0
    for i, (a, b) in enumerate(zip(literal_features[0], literal_features[1])):
        want += C.KAIR_WEIGHTS[i] * crit.lossfn(a, b)
    assert torch.equal(crit(x, gt), want)


@pytest.mark.parametrize("kind", ["l1", "mse", "fro"])
def test_torchs_fp32_result_meets_its_bound(literal_features, kind):
    xs = [t.clone().requires_grad_(True) for t in literal_features[0]]
    gs = literal_features[1]
    loss = R.torch_loop(xs, gs, C.KAIR_WEIGHTS, kind)
    grads = torch.autograd.grad(loss, xs)
    want = R.criterion(xs, gs, C.KAIR_WEIGHTS, kind)
    shares = [R.share(loss, want.total, want.torch_total_bound)]
    shares += [R.share(g, w, b) for g, w, b in zip(grads, want.grads, want.torch_grad_bound)]
    print(f"torch fp32 {kind}: share of its bound, loss {shares[0]:.3e}, gradients {max(shares[1:]):.3e}")
    assert max(shares) <= 1.0
    assert want.total_bound < want.torch_total_bound
