"""libjpeg's baseline JPEG round trip: the integer restatement (tests/jpeg_codec_reference.py, the specification of
ssl_amd/csrc/ssg_jpegcodec.hip) against Pillow, live and as recorded (tests/golden/f31_jpeg_codec.npz), and the host
side of ssl_amd.datapath's wrappers.  Equality everywhere: the codec is integer arithmetic from end to end.

Pillow calls libjpeg as OpenCV does (jpeg_set_quality(q, force_baseline), 4:2:0, JDCT_ISLOW, fancy upsampling), so it
stands in for the reference's cv2.imencode / cv2.imdecode, which is not installed; that the two agree is supposed.

The range limit: libjpeg's portable inverse DCT indexes its range-limit table through a 10-bit mask, so an output
beyond -512 .. 511 around the centre would wrap, where libjpeg-turbo's vector code saturates.  On every case here, the
+-255 checkerboards of period 1 and 8 at quality 1 and 100 included, the two give the same bytes as Pillow: nothing in
the set comes near the wrap, the restatement clamps, and `wrong='wrap'` is asserted to be indistinguishable
(test_range_limit_checkerboards) instead of being in the sensitivity list."""
import functools

import numpy as np
import pytest
import torch

import jpeg_codec_cases as K
import jpeg_codec_reference as R


def _jpeg_pillow():
    try:
        from PIL import features
        return bool(features.check("jpg"))
    except Exception:
        return False


needs_pillow = pytest.mark.skipif(not _jpeg_pillow(), reason="Pillow with JPEG support is not installed")


@functools.lru_cache(maxsize=None)
def _live(H, W, C, q, kind):
    a = K.content(kind, H, W, C, seed=7)
    want = K.pillow_roundtrip(a, q)
    a.setflags(write=False)
    want.setflags(write=False)
    return a, want


def _all_cases(sizes):
    for (H, W) in sizes:
        for C in (1, 3):
            for q in K.QUALITIES:
                for kind in K.CONTENTS:
                    yield H, W, C, q, kind


@needs_pillow
@pytest.mark.parametrize("size", K.SIZES + K.SMALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_pillow(size):
    bad = []
    for case in _all_cases([size]):
        a, want = _live(*case)
        got = R.roundtrip(a, case[3])
        assert got.shape == want.shape and got.dtype == np.uint8
        if not np.array_equal(got, want):
            bad.append((case, int((got != want).sum())))
    assert not bad, bad


def test_restatement_equals_the_fixture():
    fix = K.load_fixture()
    assert len(fix) == len(K.FIXTURE_CASES) >= 36
    for case, (a, want) in fix.items():
        H, W, C, q, kind = case
        assert a.shape == ((H, W) if C == 1 else (H, W, 3)) and np.array_equal(a, K.content(kind, H, W, C, seed=31))
        assert np.array_equal(R.roundtrip(a, q), want), case


@needs_pillow
def test_fixture_is_what_this_pillow_gives():
    for case, (a, want) in K.load_fixture().items():
        assert np.array_equal(K.pillow_roundtrip(a, case[3]), want), case


@needs_pillow
@pytest.mark.parametrize("wrong", ["bias2", "fullres_rows", "box", "upsample_uncropped", "half_even"])
def test_wrong_rules_are_told_apart(wrong):
    """Each plausible wrong rule must change a byte somewhere in the case set; inputs that cannot tell the rules apart
    would prove nothing about the right one."""
    differing = 0
    for case in _all_cases([(24, 16), (72, 72), (17, 33), (31, 47), (24, 40)]):
        if case[2] == 1:
            continue            # the chroma rules do not touch a grey image; the quantiser's does, colour shows it too
        a, want = _live(*case)
        differing += not np.array_equal(R.roundtrip(a, case[3], wrong=wrong), want)
    assert differing > 0


@needs_pillow
def test_full_resolution_row_replication_shows_at_partial_mcu_rows_only():
    """24 x 16 and 72 x 72 (even height, partial last MCU row) tell 'fullres_rows' apart; 16 x 16 cannot."""
    for (H, W), shows in (((24, 16), True), ((72, 72), True), ((16, 16), False)):
        hit = False
        for q in K.QUALITIES:
            a, want = _live(H, W, 3, q, "noise")
            hit |= not np.array_equal(R.roundtrip(a, q, wrong="fullres_rows"), want)
        assert hit == shows, (H, W)


@needs_pillow
def test_range_limit_checkerboards():
    for (H, W) in ((16, 16), (40, 40), (17, 33)):
        for C in (1, 3):
            for kind in ("checker1", "checker8"):
                for q in (1, 100):
                    a, want = _live(H, W, C, q, kind)
                    assert np.array_equal(R.roundtrip(a, q), want)
                    assert np.array_equal(R.roundtrip(a, q, wrong="wrap"), want)


def test_int32_and_int64_dcts_agree_on_saturated_input():
    """libjpeg declares its DCT arithmetic safe in 32 bits for 8-bit samples; numpy's int32 wraps silently, so equal
    results mean no intermediate left the range.  The kernel computes in int32."""
    for (H, W) in ((16, 16), (40, 40), (31, 47)):
        for C in (1, 3):
            for kind in ("saturated", "checker1", "checker8"):
                a = K.content(kind, H, W, C, seed=3)
                for q in (1, 5, 50, 100):
                    assert np.array_equal(R.roundtrip(a, q, dtype=np.int32), R.roundtrip(a, q, dtype=np.int64))
    # and stage by stage on the extreme blocks: every sample 0 or 255, any pattern
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 2, (512, 8, 8)) * 255
    blocks[0], blocks[1] = 0, 255
    c32, c64 = R.fdct(blocks, np.int32), R.fdct(blocks, np.int64)
    assert np.array_equal(c32, c64) and np.abs(c64).max() <= 1 << 15
    for q in (1, 100):
        t = R.quant_tables(q)[0]
        deq = R.quantise(c64, t) * t
        assert np.array_equal(R.idct(deq, np.int32), R.idct(deq, np.int64))


def test_quant_tables():
    lum, chrom = R.quant_tables(50)
    assert np.array_equal(lum, R.LUMA_BASE) and np.array_equal(chrom, R.CHROMA_BASE)
    for q in (1, 2, 10):
        assert R.quant_tables(q)[0].max() == 255
    assert all((t == 1).all() for t in R.quant_tables(100))
    assert R.quant_tables(75)[0][0, 0] == 8 and R.quant_tables(95)[1][7, 7] == 10
    for q in (0, 101):
        with pytest.raises(ValueError):
            R.quant_tables(q)


def test_stages_alone():
    # a constant block has a DC coefficient only, eight times its offset from 128, and comes back unchanged
    blk = np.full((8, 8), 200)
    c = R.fdct(blk)
    assert c[0, 0] == 8 * 8 * (200 - 128) and not c.ravel()[1:].any()
    assert np.array_equal(R.idct(R.quantise(c, np.ones((8, 8), np.int64))), blk)
    # the quantiser rounds half away from zero on the x 8 scaled coefficient
    assert R.quantise(np.array([12, -12, 11, -11, 36, -36]), np.array([3])).tolist() == [1, -1, 0, 0, 2, -2]
    assert R.quantise(np.array([12, 36]), np.array([3]), half_even=True).tolist() == [0, 2]
    # grey: Y 128 +- 127, Cb = Cr = 128
    y, cb, cr = R.rgb_to_ycc(np.array([[[0, 0, 0], [255, 255, 255], [9, 9, 9]]], np.uint8))
    assert y.tolist() == [[0, 255, 9]] and cb.tolist() == [[128] * 3] and cr.tolist() == [[128] * 3]
    assert np.array_equal(R.ycc_to_rgb(y, cb, cr)[0], [[0] * 3, [255] * 3, [9] * 3])
    # the downsample's bias alternates 1, 2 along the output columns
    assert R.downsample(np.array([[1, 0, 1, 0], [0, 0, 0, 0]])).tolist() == [[0, 0]]
    assert R.downsample(np.array([[1, 1, 1, 0], [0, 0, 1, 0]])).tolist() == [[0, 1]]
    # fancy upsampling keeps a constant plane, blends 3 : 1 both ways, and replicates a plane two samples wide
    assert (R.upsample(np.full((3, 5), 77)) == 77).all()
    up = R.upsample(np.array([[0, 16, 32]] * 2))
    assert up[0].tolist() == [0, 4, 12, 20, 28, 32]
    assert R.upsample(np.array([[1, 9]])).tolist() == [[1, 1, 9, 9]] * 2


# ---------------------------------------------------------------------------------------- the Python surface ----
@pytest.fixture
def on_cpu(monkeypatch):
    """ssl_amd.datapath's JPEG functions with the launch replaced by the restatement: what is left is the wrappers' own
    work (layouts, quantisation, channel order, dtypes, draws), which needs no GPU."""
    from ssl_amd import datapath

    def call(x, B, H, W, C, quality, in_f32, out_f32):
        qs = list(datapath._jpeg_qualities(quality, B))
        a = x.numpy()
        if in_f32:
            a = np.uint8((a.clip(0, 1) * 255).round()).transpose(0, 2, 3, 1)
        out = np.stack([R.roundtrip(a[b, ..., 0] if C == 1 else a[b], qs[b]).reshape(H, W, C) for b in range(B)])
        if out_f32:
            out = np.float32(out.transpose(0, 3, 1, 2) / 255.)
        return torch.from_numpy(np.ascontiguousarray(out))

    monkeypatch.setattr(datapath, "_jpeg_call", call)
    monkeypatch.setattr(datapath, "_jpeg_device", lambda: torch.device("cpu"))
    return datapath


def _codec(u8, q):
    return K.pillow_roundtrip(u8, q) if _jpeg_pillow() else R.roundtrip(u8, q)


def test_wrappers_equal_the_reference_one_liners(on_cpu):
    dp = on_cpu
    rng = np.random.default_rng(11)
    img = rng.random((37, 53, 3), dtype=np.float32) * 1.2 - 0.1          # leaves [0, 1] on both sides
    single2uint = lambda x: np.uint8((x.clip(0, 1) * 255.).round())     # noqa: E731  (KAIR's utils_image)
    uint2single = lambda x: np.float32(x / 255.)                        # noqa: E731
    # add_JPEG_noise: the RGB -> BGR -> RGB swaps around cv2 cancel
    want = uint2single(_codec(single2uint(img), 83))
    got = dp.add_JPEG_noise(img, 83)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want)
    got = dp.add_JPEG_noise(torch.from_numpy(img), 83)
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), want)
    got = dp.add_JPEG_noise(img.astype(np.float64), 83)                 # quantised in the image's own dtype
    assert got.dtype == np.float32 and np.array_equal(got, uint2single(_codec(single2uint(img.astype(np.float64)), 83)))
    # add_jpg_compression: cv2 reads the array as BGR
    bgr = np.clip(img, 0, 1)
    want = np.float32(_codec(np.uint8((bgr * 255.).round())[..., ::-1], 90)[..., ::-1]) / 255.
    assert np.array_equal(dp.add_jpg_compression(img), want)
    assert not np.array_equal(dp.add_jpg_compression(img), dp.add_JPEG_noise(img, 90))
    assert np.array_equal(dp.add_jpg_compression(img, 90.7), want)      # int(quality), as the diffusion fork's copy
    # jpeg_compress: bytes and floats, both channel orders, the same dtype out
    u8 = single2uint(img)
    assert np.array_equal(dp.jpeg_compress(u8, 40), _codec(u8, 40))
    assert np.array_equal(dp.jpeg_compress(u8, 40, chn_in='bgr'), _codec(u8[..., ::-1], 40)[..., ::-1])
    got = dp.jpeg_compress(np.clip(img, 0, 1).astype(np.float64), 40)
    assert got.dtype == np.float64
    assert np.array_equal(got, uint2single(_codec(single2uint(np.clip(img, 0, 1).astype(np.float64)), 40)).astype(np.float64))
    got = dp.jpeg_compress(torch.from_numpy(u8), 40)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), _codec(u8, 40))


def test_add_jpeg_noise_draws_its_quality(on_cpu):
    dp = on_cpu
    img = np.random.default_rng(2).random((16, 24, 3), dtype=np.float32)

    class Fixed(dp.Draws):
        calls = []

        def randint(self, lo, hi):
            self.calls.append((lo, hi))
            return 77

    assert np.array_equal(dp.add_JPEG_noise(img, draws=Fixed()), dp.add_JPEG_noise(img, 77))
    assert Fixed.calls == [(75, 95)]
    import random
    random.seed(4)
    want_q = random.randint(75, 95)
    random.seed(4)
    assert np.array_equal(dp.add_JPEG_noise(img), dp.add_JPEG_noise(img, want_q))


def test_jpeg_roundtrip_layouts(on_cpu):
    dp = on_cpu
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (2, 17, 33, 3), dtype=np.uint8)
    t = torch.from_numpy(a)
    want = np.stack([R.roundtrip(a[0], 30), R.roundtrip(a[1], 90)])
    assert np.array_equal(dp.jpeg_roundtrip(t, [30, 90]).numpy(), want)
    assert np.array_equal(dp.jpeg_roundtrip(t, torch.tensor([30, 90])).numpy(), want)
    assert np.array_equal(dp.jpeg_roundtrip(t[0], 30).numpy(), want[0])
    g = t[..., 1].contiguous()                                          # (B,H,W) grey
    assert np.array_equal(dp.jpeg_roundtrip(g, 30).numpy(), np.stack([R.roundtrip(a[b, ..., 1], 30) for b in range(2)]))
    assert dp.jpeg_roundtrip(g[0], 30).shape == (17, 33)
    f = (t.permute(0, 3, 1, 2).float() / 255).requires_grad_()
    out = dp.jpeg_roundtrip(f, [30, 90])
    assert out.dtype == torch.float32 and out.shape == f.shape and not out.requires_grad
    assert np.array_equal(out.numpy(), np.float32(want.transpose(0, 3, 1, 2) / 255.))
    assert dp.jpeg_roundtrip(f.detach().double(), 30).dtype == torch.float64


def test_argument_errors(on_cpu):
    dp = on_cpu
    u8 = torch.zeros(16, 16, 3, dtype=torch.uint8)
    for q in (0, 101, 75.5, True, "90", None):
        with pytest.raises((ValueError, TypeError), match="quality"):
            dp.jpeg_roundtrip(u8, q)
    with pytest.raises(ValueError, match="one per image"):
        dp.jpeg_roundtrip(u8[None], [75, 80])
    with pytest.raises(ValueError, match="uint8"):
        dp.jpeg_roundtrip(torch.zeros(2, 16, 16, 4, dtype=torch.uint8), 75)
    with pytest.raises(ValueError, match="float"):
        dp.jpeg_roundtrip(torch.zeros(16, 16, 3), 75)
    with pytest.raises(ValueError, match="float"):
        dp.jpeg_roundtrip(torch.zeros(1, 2, 16, 16), 75)
    with pytest.raises(TypeError):
        dp.jpeg_roundtrip(torch.zeros(16, 16, dtype=torch.int32), 75)
    with pytest.raises(TypeError):
        dp.jpeg_roundtrip(np.zeros((16, 16), np.uint8), 75)
    with pytest.raises(ValueError, match="H,W,3"):
        dp.add_JPEG_noise(np.zeros((16, 16), np.float32), 80)
    with pytest.raises(TypeError, match="float"):
        dp.add_jpg_compression(np.zeros((16, 16, 3), np.uint8))
    with pytest.raises(ValueError, match="chn_in"):
        dp.jpeg_compress(np.zeros((16, 16, 3), np.uint8), 50, chn_in='yuv')


def test_no_cpu_path():
    from ssl_amd import datapath
    with pytest.raises(RuntimeError, match="GPU"):
        datapath.jpeg_roundtrip(torch.zeros(16, 16, 3, dtype=torch.uint8), 75)


# ------------------------------------------------------------------------------------------- the library's host side ----
@pytest.fixture(scope="module")
def L():
    from ssl_amd import _lib
    return _lib.lib()


def test_unit_table_is_numpy_float32_of_v_over_255(L):
    table = np.zeros(256, np.float32)
    assert L.ssg_jpeg_unit_table(table.ctypes.data) == 0
    want = np.array([np.float32(v / 255.) for v in range(256)], np.float32)
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    assert L.ssg_jpeg_unit_table(None) == -1


def test_exports_and_workspace_size(L):
    from ssl_amd import _lib
    header = open(_lib.HEADER).read()
    for name in ("ssg_jpeg_roundtrip", "ssg_jpeg_roundtrip_workspace_bytes", "ssg_jpeg_unit_table"):
        assert hasattr(L, name) and name in _lib.PROTOTYPES and f"{name}(" in header
    size = L.ssg_jpeg_roundtrip_workspace_bytes
    assert size(4, 2040, 1356, 1) == 0                                     # grey: nothing to hand over
    assert size(0, 64, 64, 3) == 0 and size(1, 64, 64, 2) == 0 and size(1, 0, 64, 3) == 0
    assert size(1, 1, 1, 3) == 256 and size(3, 17, 33, 3) == 3 * 1024     # 17 * 33 + 2 * 9 * 17 = 867 bytes an image
    per = 2040 * 1356 + 2 * 1020 * 678                                     # Y, Cb and Cr of an image
    assert size(16, 2040, 1356, 3) == 16 * ((per + 255) // 256 * 256)


def test_status_codes_that_need_no_device(L):
    """every refusal is decided on the host before anything is launched"""
    import ctypes
    a = np.zeros((1, 16, 16, 3), np.uint8)
    o = np.zeros_like(a)
    q = (ctypes.c_int * 1)(75)
    qa = ctypes.addressof(q)
    call = L.ssg_jpeg_roundtrip
    E_BADARG = -1
    assert call(None, o.ctypes.data, 1, 16, 16, 3, qa, 0, 0, None, 0, None) == E_BADARG
    assert call(a.ctypes.data, None, 1, 16, 16, 3, qa, 0, 0, None, 0, None) == E_BADARG
    assert call(a.ctypes.data, o.ctypes.data, 1, 16, 16, 3, None, 0, 0, None, 0, None) == E_BADARG
    assert call(a.ctypes.data, a.ctypes.data, 1, 16, 16, 3, qa, 0, 0, None, 0, None) == E_BADARG
    for ch in (0, 2, 4):
        assert call(a.ctypes.data, o.ctypes.data, 1, 16, 16, ch, qa, 0, 0, None, 0, None) == E_BADARG
    for bad in (0, 101, -5):
        qb = (ctypes.c_int * 1)(bad)
        assert call(a.ctypes.data, o.ctypes.data, 1, 16, 16, 3, ctypes.addressof(qb), 0, 0, None, 0, None) == E_BADARG
    assert call(a.ctypes.data, o.ctypes.data, 1, 16, 16, 3, qa, 2, 0, None, 0, None) == E_BADARG
    assert call(a.ctypes.data, o.ctypes.data, 1, 16, 16, 3, qa, 0, 2, None, 0, None) == E_BADARG
    assert call(a.ctypes.data, o.ctypes.data, 0, 16, 16, 3, qa, 0, 0, None, 0, None) == E_BADARG
    # (the workspace's refusals need a call of the two-launch path and real buffers: tests/test_gpu_jpeg_codec.py)
