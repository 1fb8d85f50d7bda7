"""The ragged degradation kernels (ssl_amd/csrc/ssg_blindsr.hip) on the GPU against tests/blindsr_reference.py: the
convolution and the resizes within the derived first-order bounds, the noise stages bit for bit, every image of a ragged
launch bit-equal to the same image run alone, launches past one trip of the capped grid, and the whole chain stage by
stage.  Shapes are small: every test takes seconds."""
import numpy as np
import pytest
import torch

import blindsr_cases as cases
import blindsr_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _apply(dev, family, images, stages, fields=None):
    from ssl_amd import blindsr
    fam = {"conv": blindsr.CONV, "resize": blindsr.RESIZE, "noise": blindsr.NOISE}[family]
    f = None if fields is None else [None if q is None else torch.from_numpy(q).to(dev) for q in fields]
    out = blindsr.ragged_apply(fam, [torch.from_numpy(x).to(dev) for x in images], stages, f)
    torch.cuda.synchronize()
    return out


def _within(got, want, bound, what):
    """the largest share of the bound used; asserts every element inside it"""
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), what


@pytest.mark.parametrize("k", cases.CONV_KS)
def test_conv_every_side_stride_and_channel_count(dev, k):
    """sides 1 .. 70 in every pair (an axis shorter than the radius, a tile's side + 1), strides 1, 2 and 4, one and three
    channels, an asymmetric kernel (a missing flip is an error of 1e-2), with and without the clip: one ragged launch"""
    images, stages = cases.conv_cases(k)
    got = _apply(dev, "conv", images, stages)
    share = 0.0
    for x, st, y in zip(images, stages, got):
        want, bound = R.conv(x, st.params["kernel"], st.params["stride"], st.params["clip"])
        share = max(share, _within(y, want, bound, (k, x.shape, st.params["stride"])))
    print(f"conv k={k}: {len(images)} images, {share:.3f} of the bound")


@pytest.mark.parametrize("interp", [R.LINEAR, R.CUBIC, R.AREA])
def test_resize_every_ratio(dev, interp):
    """ratios 1/2, 1/3, 1/4, 0.53, 1/1.17, 1, 1.37 and 2, a single pixel out and in, unequal ratios, one axis reduced
    and the other enlarged (AREA then takes its linear rule), an 8 x 8 box: one ragged launch per mode"""
    images, stages = cases.resize_cases(interp)
    got = _apply(dev, "resize", images, stages)
    share = 0.0
    for x, st, y in zip(images, stages, got):
        want, bound = R.resize(x, st.oh, st.ow, interp, st.params["clip"])
        share = max(share, _within(y, want, bound, (interp, x.shape, st.oh, st.ow)))
    print(f"resize interp={interp}: {len(images)} images, {share:.3f} of the bound")


def test_noise_every_mode_bit_for_bit(dev):
    """every mode of the three functions in one launch; the first row lies exactly at (k + 1/2) / 255, and the NaN pixel
    reaches the output wherever the reference's expression reads the image"""
    images, stages, fields = cases.noise_cases()
    got = _apply(dev, "noise", images, stages, fields)
    for x, st, f, y in zip(images, stages, fields, got):
        want = cases.noise_reference(x, st, f)
        _same_bits(y, want, st.params["op"])
        if st.params["op"] != "POISSON_COLOR":                  # (which replaces the image by the draw)
            assert bool(torch.isnan(y[0, 5, 7])), st.params["op"]


@pytest.mark.parametrize("family", ["conv", "resize", "noise"])
def test_every_image_of_a_ragged_launch_is_the_image_run_alone(dev, family):
    """five images of five sizes under five different operations in one launch, then each alone: the same bits"""
    from ssl_amd.blindsr import Stage
    rng = np.random.default_rng(5)
    sizes = [(1, 33, 70), (3, 9, 5), (3, 40, 41), (1, 2, 1), (3, 17, 64)]
    images = [(rng.random(s, dtype=np.float32) * 1.2 - 0.1).astype(np.float32) for s in sizes]
    fields = None
    if family == "conv":
        stages = [Stage("conv", h, w, -(-h // s), -(-w // s), dict(kernel=cases.asymmetric_kernel(rng, k), stride=s, clip=c))
                  for (_, h, w), k, s, c in zip(sizes, (3, 9, 5, 7, 9), (1, 2, 4, 1, 2), (True, False, True, False, True))]
    elif family == "resize":
        outs = [(16, 35), (18, 10), (13, 20), (5, 3), (17, 32)]
        stages = [Stage("resize", h, w, oh, ow, dict(interp=i, clip=c))
                  for (_, h, w), (oh, ow), i, c in zip(sizes, outs, (3, 2, 3, 1, 3), (True, False, True, False, False))]
    else:
        ops = ["GAUSS_GRAY", "SPECKLE_CORR", "POISSON_GRAY", "SPECKLE_COLOR", "GAUSS_CORR"]
        all_images, all_stages, all_fields = cases.noise_cases(seed=1, nan=False)
        by_op = {st.params["op"]: (st, f) for (st, f), (_, C) in zip(zip(all_stages, all_fields), cases.NOISE_MODES) if C == 3}
        sizes = [(3, h, w) for _, h, w in sizes]
        images = [(rng.random(s, dtype=np.float32) * 1.2 - 0.1).astype(np.float32) for s in sizes]
        stages, fields = [], []
        for (C, h, w), op in zip(sizes, ops):
            st = by_op[op][0]
            planes = 1 if op.endswith("GRAY") else C
            stages.append(Stage("noise", h, w, h, w, st.params))
            fields.append((rng.standard_normal((planes, h, w)) * 3 + 20).astype(np.float32))
    together = _apply(dev, family, images, stages, fields)
    for i in range(len(images)):
        alone = _apply(dev, family, images[i:i + 1], stages[i:i + 1], None if fields is None else fields[i:i + 1])[0]
        assert torch.equal(_bits(alone), _bits(together[i])), (family, i)


@pytest.mark.parametrize("family", ["conv", "resize", "noise"])
def test_more_tiny_images_than_one_trip_of_the_capped_grid(dev, family):
    """1,300 images of 1 x 1 .. 3 x 4: one tile each, so the tile prefix is walked past the grid cap (grid-stride)"""
    from ssl_amd import _lib
    from ssl_amd.blindsr import Stage
    n = 1300
    assert n > _lib.lib().ssg_blindsr_grid_cap()
    rng = np.random.default_rng(6)
    shapes = [((1, 3)[i % 2], 1 + i % 3, 1 + (i // 3) % 4) for i in range(n)]
    images = [(rng.random(s, dtype=np.float32) * 1.2 - 0.1).astype(np.float32) for s in shapes]
    fields = None
    if family == "conv":
        kern = {k: cases.asymmetric_kernel(rng, k) for k in cases.CONV_KS}
        stages = [Stage("conv", h, w, h, w, dict(kernel=kern[cases.CONV_KS[i % 4]], stride=1, clip=False))
                  for i, (_, h, w) in enumerate(shapes)]
    elif family == "resize":
        stages = [Stage("resize", h, w, 1 + (i // 5) % 4, 1 + (i // 7) % 5, dict(interp=1 + i % 3, clip=False))
                  for i, (_, h, w) in enumerate(shapes)]
    else:
        stages = [Stage("noise", h, w, h, w, dict(op=("GAUSS_COLOR", "SPECKLE_GRAY")[i % 2], scale=(3 + i % 20) / 255.0,
                                                    matrix=None, clip=True, lead_clip=bool(i % 2)))
                  for i, (_, h, w) in enumerate(shapes)]
        fields = [rng.standard_normal(((C, 1)[i % 2], h, w)).astype(np.float32) for i, (C, h, w) in enumerate(shapes)]
    got = _apply(dev, family, images, stages, fields)
    assert len(got) == n
    for i in list(range(0, n, 7)) + list(range(n - 300, n)):
        x, st = images[i], stages[i]
        if family == "conv":
            want, bound = R.conv(x, st.params["kernel"], 1, False)
            _within(got[i], want, bound, (family, i))
        elif family == "resize":
            want, bound = R.resize(x, st.oh, st.ow, st.params["interp"], False)
            _within(got[i], want, bound, (family, i))
        else:
            _same_bits(got[i], cases.noise_reference(x, st, fields[i]), (family, i))


def _jpeg_reference(x, quality):
    """the codec restatement on a planar float image: single2uint, libjpeg's round trip, uint2single"""
    import jpeg_codec_reference as J
    u8 = (np.clip(x, 0, 1) * np.float32(255.)).round().astype(np.uint8).transpose(1, 2, 0)
    return (J.roundtrip(np.ascontiguousarray(u8), quality).astype(np.float32) / np.float32(255.)).transpose(2, 0, 1)


@pytest.mark.parametrize("variant,seed,shapes", cases.CHAIN_CASES)
def test_chain_stage_by_stage(dev, variant, seed, shapes):
    """BlindSRDegradation.feed on three small images with seeded decisions and given noise fields.  Every stage is held to
    the restatement ON THE INPUT THE GPU STAGE HAD (the trace): conv and resize within their bounds, the noise stages and
    the Poisson rates bit for bit, JPEG stages byte for byte through tests/jpeg_codec_reference.py, the crops exactly.
    Because each stage's restatement starts from the GPU's own input, no rounding stage sees two different inputs: the
    number of bytes a near-tie could flip is zero by construction, and none is allowed."""
    from ssl_amd import blindsr
    images = cases.chain_images(shapes, seed)
    draws = cases.seeded_draws(seed)
    deg = blindsr.BlindSRDegradation(sf=cases.CHAIN_SF, lq_patchsize=cases.CHAIN_PATCH, variant=variant, draws=draws)
    trace = []
    lq, hq = deg.feed([torch.from_numpy(x).to(dev) for x in images], trace=trace)
    torch.cuda.synchronize()
    progs = deg.programs
    kinds = {s.kind if s.kind != "noise" else s.params["op"].split("_")[0] for p in progs for s in p.stages}
    kinds |= {"strided" for p in progs for s in p.stages if s.kind == "conv" and s.params["stride"] > 1}
    assert "imresize" not in kinds
    assert kinds >= ({"conv", "resize", "GAUSS", "SPECKLE", "poisson", "jpeg"} if variant == "plus" else
                     {"conv", "strided", "resize", "GAUSS", "jpeg"}), kinds
    # one launch per family present in a slot, however many images: far fewer than stages
    n_stages = sum(len(p.stages) for p in progs)
    assert 0 < deg.launches < n_stages
    cur = [x.transpose(2, 0, 1)[:, :p.rows, :p.cols] for x, p in zip(images, progs)]
    given, rates = iter(draws.given), iter(draws.rates)
    shares = {"conv": 0.0, "resize": 0.0}
    for slot, snap in enumerate(trace):
        here = [(i, p.stages[slot]) for i, p in enumerate(progs) if slot < len(p.stages)]
        planes = lambda i, st: (0 if st.kind != "noise" else (1 if st.params["op"].endswith("GRAY") else cur[i].shape[0]))
        n_normal = sum(planes(i, st) * st.h * st.w for i, st in here)
        normal = next(given) if n_normal else None
        poisson = [(i, st) for i, st in here if st.kind == "poisson"]
        drawn = next(given) if poisson else None
        rate = next(rates) if poisson else None
        at_n = at_p = 0
        for i, st in here:
            x, y = np.ascontiguousarray(cur[i], dtype=np.float32), snap[i]
            assert tuple(y.shape) == (x.shape[0], st.oh, st.ow)
            if st.kind in ("conv", "resize"):
                want, bound = R.stage(st, x)
                shares[st.kind] = max(shares[st.kind], _within(y, want, bound, (slot, i, st.kind)))
            elif st.kind == "noise":
                m = planes(i, st) * st.h * st.w
                f = normal.reshape(-1)[at_n:at_n + m].reshape(-1, st.h, st.w)
                at_n += m
                _same_bits(y, R.stage(st, x, f)[0], (slot, i, st.params["op"]))
            elif st.kind == "poisson":
                m = (1 if st.params["gray"] else x.shape[0]) * st.h * st.w
                f = drawn.reshape(-1)[at_p:at_p + m].reshape(-1, st.h, st.w)
                want_rate = R.poisson_rates(x, st.params["vals"], st.params["gray"])
                assert np.array_equal(rate.reshape(-1)[at_p:at_p + m].view(np.int32), want_rate.reshape(-1).view(np.int32))
                at_p += m
                _same_bits(y, R.stage(st, x, f)[0], (slot, i, "poisson"))
            else:
                assert st.kind == "jpeg"
                _same_bits(y, _jpeg_reference(x, st.params["quality"]), (slot, i, "jpeg"))
            cur[i] = y.cpu().numpy()
    p, sf = cases.CHAIN_PATCH, cases.CHAIN_SF
    assert tuple(lq.shape) == (3, 3, p, p) and tuple(hq.shape) == (3, 3, p * sf, p * sf)
    for i, (x, prog) in enumerate(zip(images, progs)):
        t, l = prog.crop
        assert np.array_equal(lq[i].cpu().numpy(), cur[i][:, t:t + p, l:l + p])
        assert np.array_equal(hq[i].cpu().numpy(), x.transpose(2, 0, 1)[:, t * sf:(t + p) * sf, l * sf:(l + p) * sf])
    print(f"chain {variant}: {n_stages} stages in {deg.launches} ragged launches; shares of the bound {shares}")


def test_single_image_functions_are_the_batch_of_one(dev):
    """add_blur, add_resize and the three noise functions on one HWC image: the program of one stage, the same bits as the
    stage in a batch, numpy in and numpy out"""
    from ssl_amd import blindsr
    x = cases.chain_images(((40, 52),), 3)[0]
    for fn, kind in ((blindsr.add_blur, "conv"), (blindsr.add_resize, "resize"), (blindsr.add_Gaussian_noise, "noise"),
                     (blindsr.add_speckle_noise, "noise"), (blindsr.add_Poisson_noise, "poisson")):
        d1, d2 = cases.seeded_draws(9), cases.seeded_draws(9)
        got = fn(x, draws=d1)
        st = {blindsr.add_blur: lambda: blindsr._blur_stage(40, 52, 4, d2),
              blindsr.add_resize: lambda: blindsr._add_resize_stage(40, 52, 4, d2),
              blindsr.add_Gaussian_noise: lambda: blindsr._gaussian_stage(40, 52, 3, 1, 12, d2),
              blindsr.add_speckle_noise: lambda: blindsr._speckle_stage(40, 52, 3, 2, 25, d2),
              blindsr.add_Poisson_noise: lambda: blindsr._poisson_stage(40, 52, 3, d2)}[fn]()
        assert st.kind == kind and isinstance(got, np.ndarray) and got.shape == (st.oh, st.ow, 3) and got.dtype == np.float32
        out, _ = blindsr.run_stages([torch.from_numpy(x).to(dev).permute(2, 0, 1).contiguous()], [[st]], d2)
        assert np.array_equal(got.view(np.int32), out[0].permute(1, 2, 0).contiguous().cpu().numpy().view(np.int32))
    lq, hq = blindsr.degradation_bsrgan(cases.chain_images(((96, 100),), 4)[0], sf=4, lq_patchsize=16, draws=cases.seeded_draws(2))
    assert lq.shape == (16, 16, 3) and hq.shape == (64, 64, 3) and lq.min() >= 0 and lq.max() <= 1
    with pytest.raises(NotImplementedError):
        blindsr.degradation_bsrgan(x, isp_model=object())


def poison_cases():
    """the outputs the LDS-poison audit compares (test_gpu_blindsr_poison.py): the convolution stages its window and its
    taps through LDS; one launch per family"""
    dev = torch.device("cuda:0")
    out = []
    for k in (3, 9):
        images, stages = cases.conv_cases(k, seed=1)
        out += _apply(dev, "conv", images, stages)
    images, stages = cases.resize_cases(R.AREA, seed=1)
    out += _apply(dev, "resize", images, stages)
    images, stages, fields = cases.noise_cases(seed=1, nan=False)
    out += _apply(dev, "noise", images, stages, fields)
    return out
