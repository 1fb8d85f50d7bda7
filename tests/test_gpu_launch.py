"""Every call family whose launch goes through ssl_amd/_gpu.py on a stream and a GPU that are not the default ones.

A launch on the wrong stream is silent, so the side-stream test makes it visible: on the side stream the input first
holds a constant, then the stream idles for 20 million cycles (8 to 20 ms at any clock between 1 and 2.5 GHz, hundreds
of times a launch's host latency; derived from the clock range, not measured), then the real input is copied in and the
wrapper runs.  A wrapper that launched on the default stream would read the constant."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SLEEP_CYCLES = 20_000_000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _rand(shape, seed, device):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(device)


def _filter2d(device):
    from ssl_amd import datapath
    kernel = _rand((1, 3, 3), 1, device)
    return _rand((1, 3, 8, 8), 2, device), lambda x: (datapath.filter2D(x, kernel),)


def _usm_sharp(device):
    from ssl_amd import datapath
    return _rand((1, 1, 26, 26), 3, device), lambda x: (datapath.USMSharp()(x),)


def _similarity(device):
    from ssl_amd.losses.similarity.similaritywrapper import compute_similarity
    mask = torch.zeros(16, 16, device=device)
    mask[3, 12] = mask[9, 4] = 1
    weight = _rand((2, 5, 5), 4, device)

    def call(x):
        image = x.detach().clone().requires_grad_(True)
        out = compute_similarity(image, mask, psize=5, ksize=3)
        out.backward(weight)
        return out.detach(), image.grad
    return _rand((3, 16, 16), 5, device), call


def _l1_loss(device):
    from ssl_amd.losses import basic_loss
    target = _rand((70,), 6, device)

    def call(x):
        pred = x.detach().clone().requires_grad_(True)
        assert basic_loss._native_pair(pred, target), "this pair would take the torch expressions, not the kernels"
        loss = basic_loss.L1Loss()(pred, target)
        loss.backward()
        return loss.detach(), pred.grad
    return _rand((70,), 7, device), call


def _resize(device):
    from ssl_amd import prep
    y = torch.randint(0, 256, (9, 11, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).to(device)
    return y, lambda x: (prep.resize(x, (5, 4)),)


def _ragged_resize(device):
    from ssl_amd import blindsr
    stage = blindsr.Stage("resize", 6, 7, 4, 5, dict(interp=2, clip=True))
    return _rand((1, 6, 7), 9, device), lambda x: tuple(blindsr.ragged_apply(blindsr.RESIZE, [x], [stage]))


FAMILIES = {"filter2D": _filter2d, "USMSharp": _usm_sharp, "compute_similarity": _similarity, "L1Loss": _l1_loss,
            "prep.resize": _resize, "ragged_apply": _ragged_resize}


def _same(a, b):
    return len(a) == len(b) and all(s.shape == t.shape and torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_call_on_a_side_stream_reads_what_that_stream_wrote(dev, family):
    y, call = FAMILIES[family](dev)
    constant = 3 if y.dtype == torch.uint8 else 0.25
    want = call(y)
    torch.cuda.synchronize()
    assert not _same(want, call(torch.full_like(y, constant))), "a stale read would give the same result: no test"
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = torch.empty_like(y).fill_(constant)
        torch.cuda._sleep(SLEEP_CYCLES)
        x.copy_(y)
        got = call(x)
    side.synchronize()
    assert _same(want, got)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
@pytest.mark.parametrize("family", ["compute_similarity", "filter2D"])
def test_a_call_runs_on_the_gpu_that_holds_its_tensors(dev, family):
    """cuda:0 is current, the tensors are cuda:1's: the same bits as with cuda:1 current."""
    other = torch.device("cuda:1")
    y, call = FAMILIES[family](other)
    with torch.cuda.device(other):
        want = call(y)
        torch.cuda.synchronize()
    assert torch.cuda.current_device() == 0
    got = call(y)
    torch.cuda.synchronize(other)
    assert all(t.device == other for t in got) and _same(want, got)
