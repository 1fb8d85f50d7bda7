"""The JPEG round-trip kernels (ssl_amd/csrc/ssg_jpegcodec.hip) and ssl_amd.datapath's functions over them against the
integer restatement (tests/jpeg_codec_reference.py, held to Pillow by tests/test_cpu_jpeg_codec.py) and against the
bytes Pillow recorded (tests/golden/f31_jpeg_codec.npz).  Bit for bit throughout.

A workgroup codes a tile of 32 x 32 pixels; a colour call hands its reconstructed planes over in a workspace and
upsamples in a second launch, a grey call is one launch.  Shapes: one block, one MCU, odd sides, even heights with a
partial last MCU row (24 x 40, 72 x 72), two tiles plus a pixel (64 x 65, 65 x 65), five by three tiles with ragged edges
(130 x 70), sides below 8; 257 images, one more than a launch carries qualities for.  The grid is not capped: one
workgroup per tile and image.  The profiling build's two switches (the one-launch path that recomputes the chroma
blocks around each tile, and tiles of 64 x 64) are held to the same bytes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import jpeg_codec_cases as K
import jpeg_codec_reference as R

E_BADARG, E_WORKSPACE, E_ALIGN = -1, -3, -5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_amd import _lib
    _lib.lib()
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _fixture():
    return K.load_fixture()


@functools.lru_cache(maxsize=None)
def _want(case):
    """(input, the restatement's output) of a fixture case, computed once (the poison test runs the same cases)"""
    a, pillow = _fixture()[case]
    want = R.roundtrip(a, case[3])
    assert np.array_equal(want, pillow)
    want.setflags(write=False)
    return a, want


def _gpu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _roundtrip(dev, a, q):
    from ssl_amd import datapath
    return datapath.jpeg_roundtrip(_gpu(a, dev), q)


@functools.lru_cache(maxsize=None)
def _cycled(H, W, C, B):
    """B images cycling through three contents and three qualities, and the restatement's outputs"""
    kinds, qs = ("noise", "ramp", "saturated"), (85, 30, 100)
    ins = [K.content(kinds[i], H, W, C, seed=9) for i in range(3)]
    outs = [R.roundtrip(ins[i], qs[i]) for i in range(3)]
    idx = np.arange(B) % 3
    return np.stack([ins[i] for i in idx]), [qs[i] for i in idx], np.stack([outs[i] for i in idx])


@pytest.mark.gpu
@pytest.mark.parametrize("case", K.FIXTURE_CASES, ids=K.fixture_name)
def test_kernel_equals_restatement_and_fixture(dev, case):
    a, want = _want(case)
    got = _roundtrip(dev, a, case[3])
    assert got.dtype == torch.uint8 and got.shape == a.shape
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(65, 65, 3), (8, 8, 3), (40, 24, 1)], ids=lambda s: "%dx%d_c%d" % s)
def test_more_images_than_a_launch_carries(dev, shape):
    H, W, C = shape
    a, qs, want = _cycled(H, W, C, 257)
    got = _roundtrip(dev, a, qs)
    assert np.array_equal(got.cpu().numpy(), want)
    for b in (0, 1, 2, 256):                                                # the same images alone
        assert np.array_equal(_roundtrip(dev, a[b], qs[b]).cpu().numpy(), want[b])


@pytest.mark.gpu
def test_batch_of_four_qualities_alone_and_repeated(dev):
    qs = [5, 50, 90, 100]
    a = np.stack([K.content(k, 37, 53, 3, seed=2) for k in ("noise", "ramp", "saturated", "noise")])
    want = np.stack([R.roundtrip(a[b], qs[b]) for b in range(4)])
    got = _roundtrip(dev, a, qs)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(_roundtrip(dev, a, qs), got)                       # a repeated call
    assert torch.equal(_roundtrip(dev, a, torch.tensor(qs, device=dev)), got)
    for b in range(4):
        assert torch.equal(_roundtrip(dev, a[b], qs[b]), got[b])          # image b alone
    g = a[..., 0]                                                          # and grey, (B,H,W)
    got = _roundtrip(dev, g, qs)
    assert got.shape == g.shape
    assert np.array_equal(got.cpu().numpy(), np.stack([R.roundtrip(g[b], qs[b]) for b in range(4)]))


def _raw(dev, x, B, H, W, C, qs, in_f32, out_f32):
    from ssl_amd import datapath
    return datapath._jpeg_call(x, B, H, W, C, qs, in_f32, out_f32)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3])
def test_every_input_layout_and_epilogue(dev, C):
    """uint8 HWC or fp32 NCHW in (quantised as single2uint does, half to even, clipped), uint8 HWC or fp32 NCHW
    v / 255 out"""
    rng = np.random.default_rng(8)
    H, W = 72, 100
    f3 = rng.random((3, C, H, W), dtype=np.float32) * 1.5 - 0.25          # leaves [0, 1] on both sides
    f3[0, :, :4] = (np.arange(W * 4 * C).reshape(C, 4, W) % 256 + 0.5) / 255.         # halves: the rounding's ties
    u3 = np.uint8((f3.clip(0, 1) * 255).round()).transpose(0, 2, 3, 1)
    q3 = (30, 90, 75)
    w3 = np.stack([R.roundtrip(u3[b, ..., 0] if C == 1 else u3[b], q3[b]).reshape(H, W, C) for b in range(3)])
    for B in (2, 3):
        idx = np.arange(B) % 3
        f, u8, want = np.ascontiguousarray(f3[idx]), np.ascontiguousarray(u3[idx]), w3[idx]
        qs = [q3[i] for i in idx]
        want_f = np.float32(want.transpose(0, 3, 1, 2) / 255.)
        for in_f32 in (False, True):
            x = _gpu(f if in_f32 else u8, dev)
            for out_f32 in (False, True):
                got = _raw(dev, x, B, H, W, C, qs, in_f32, out_f32).cpu().numpy()
                if out_f32:
                    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want_f.view(np.uint32))
                else:
                    assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.gpu
def test_wrappers(dev):
    from ssl_amd import datapath as dp
    rng = np.random.default_rng(12)
    img = rng.random((40, 56, 3), dtype=np.float32) * 1.2 - 0.1
    single2uint = lambda x: np.uint8((x.clip(0, 1) * 255.).round())       # noqa: E731
    want = np.float32(R.roundtrip(single2uint(img), 83) / 255.)
    assert np.array_equal(dp.add_JPEG_noise(img, 83), want)
    got = dp.add_JPEG_noise(_gpu(img, dev), 83)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    want = np.float32(R.roundtrip(single2uint(img)[..., ::-1], 90)[..., ::-1]) / 255.
    assert np.array_equal(dp.add_jpg_compression(img), want)
    u8 = single2uint(img)
    assert np.array_equal(dp.jpeg_compress(u8, 40), R.roundtrip(u8, 40))
    assert np.array_equal(dp.jpeg_compress(_gpu(u8, dev), 40, chn_in='bgr').cpu().numpy(),
                          R.roundtrip(u8[..., ::-1], 40)[..., ::-1])
    got = dp.jpeg_compress(np.clip(img, 0, 1), 40)
    assert got.dtype == np.float32 and np.array_equal(got, np.float32(R.roundtrip(u8, 40) / 255.))


@pytest.mark.gpu
def test_every_status_code(dev):
    """decided before anything is launched: the output keeps what it held"""
    from ssl_amd import _lib
    L = _lib.lib()
    B, H, W = 2, 65, 65
    need = L.ssg_jpeg_roundtrip_workspace_bytes(B, H, W, 3)
    x = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev)
    out = torch.full_like(x, 7)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    qs = (ctypes.c_int * B)(*([75] * B))
    st = torch.cuda.current_stream().cuda_stream

    def call(xp=x.data_ptr(), op=out.data_ptr(), b=B, h=H, w=W, c=3, q=ctypes.addressof(qs), il=0, oe=0,
             wp=ws.data_ptr(), wb=need):
        return L.ssg_jpeg_roundtrip(xp, op, b, h, w, c, q, il, oe, wp, wb, st)

    assert call(xp=None) == E_BADARG and call(op=None) == E_BADARG and call(q=None) == E_BADARG
    assert call(wp=None) == E_BADARG and call(op=x.data_ptr()) == E_BADARG
    assert call(c=2) == E_BADARG and call(c=0) == E_BADARG and call(b=0) == E_BADARG and call(h=0) == E_BADARG
    assert call(il=2) == E_BADARG and call(oe=-1) == E_BADARG
    for bad in (0, 101):
        qb = (ctypes.c_int * B)(*([75] * (B - 1) + [bad]))
        assert call(q=ctypes.addressof(qb)) == E_BADARG
    assert need == 2 * 256 * -(-(65 * 65 + 2 * 33 * 33) // 256) and L.ssg_jpeg_roundtrip_workspace_bytes(B, H, W, 1) == 0
    assert call(wb=need - 1) == E_WORKSPACE and call(wb=0) == E_WORKSPACE
    assert call(wp=ws.data_ptr() + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), R.roundtrip(np.zeros((H, W, 3), np.uint8), 75))
    assert _lib.lib().ssg_status_string(E_WORKSPACE) and _lib.lib().ssg_status_string(E_ALIGN)


@pytest.mark.gpu
@pytest.mark.parametrize("switches", [{"SSG_JPEG_FUSED": "1"}, {"SSG_JPEG_TM": "4"}, {"SSG_JPEG_FUSED": "1", "SSG_JPEG_TM": "4"}],
                         ids=lambda d: "-".join(sorted(d)))
def test_profiling_build_switches_give_the_same_bytes(dev, switches):
    """profiles/jpeg_codec_tile_ab.txt times these variants; they have to compute the same thing"""
    import os
    from ssl_amd import _lib
    cases = [c for c in K.FIXTURE_CASES if (c[0], c[1]) in ((130, 70), (65, 65), (72, 72), (31, 47), (40, 4), (1, 40), (3, 2))]
    assert len(cases) >= 9
    saved = {k: os.environ.get(k) for k in switches}
    try:
        os.environ.update(switches)
        with _lib.profile_build() as L:
            if "SSG_JPEG_FUSED" in switches:
                assert L.ssg_jpeg_roundtrip_workspace_bytes(1, 65, 65, 3) == 0
            for case in cases:
                a, want = _want(case)
                assert np.array_equal(_roundtrip(dev, a, case[3]).cpu().numpy(), want), case
            torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def poison_cases(dev=None):
    """the outputs tests/test_gpu_jpeg_codec_poison.py compares between the product build and the poisoned profiling
    build: every fixture case, 257 images of 65 x 65, and every layout"""
    dev = dev or torch.device("cuda")
    outs = [_roundtrip(dev, _want(c)[0], c[3]) for c in K.FIXTURE_CASES]
    a, qs, _ = _cycled(65, 65, 3, 257)
    outs.append(_roundtrip(dev, a, qs))
    f = torch.from_numpy(np.float32(a[:3].transpose(0, 3, 1, 2) / 255.)).to(dev)
    for in_f32 in (False, True):
        x = f if in_f32 else _gpu(a[:3], dev)
        outs.append(_raw(dev, x.contiguous(), 3, 65, 65, 3, qs[:3], in_f32, True))
    torch.cuda.synchronize()
    return outs
