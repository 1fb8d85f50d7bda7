"""jpeg_kernel (ssl_amd/csrc/ssg_datapath.hip, behind ssg_diffjpeg / datapath.DiffJPEG) held to the fp64 oracle on EVERY
macroblock of every case of tests/jpeg_cases.py: odd and 1-pixel sides, flat / saturated / hard-edged / checkerboard
content, quality tensors on both sides of 50 up to 99, scalar qualities.  The comparison is tests/jpeg_reference.jpeg_match:
a rounding that fp32 does not decide may go either way, consistently within its macroblock; everything else is held to
3e-6, the project's F14 bound.  tests/test_cpu_jpeg.py pins the cases (no macroblock over the cap), shows that the
reference's own fp32 output passes and that wrong outputs do not.  Every comparison prints one `DPSWEEP jpeg` line
(pytest -s): worst error, bound, macroblocks, how many held undecided quotients, how many needed the other rounding.
"""
import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_reference as jr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from ssl_amd import _lib
    _lib.lib()  # raises if libssg_hip.so is missing: no silent fallback
    return torch.device("cuda:0")


def T(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype, device=dev)          # (a copy: the cases are read-only arrays)


def run(dev, x, quality):
    from ssl_amd import datapath
    q = T(quality, dev) if np.ndim(quality) else quality
    return datapath.DiffJPEG()(T(x, dev), q)


@pytest.mark.parametrize("tag", jc.TAGS)
def test_every_case_on_every_macroblock(dev, tag):
    """datapath.DiffJPEG()(x, quality) through jpeg_match, tensor and scalar quality (a Python int among them)."""
    x, quality = jc.case(tag)
    y = run(dev, x, quality)
    assert y.dtype == torch.float32 and y.shape == x.shape and y.is_contiguous()
    r = jr.jpeg_match(y.cpu().numpy(), x, quality, oracle=jc.oracle(tag))
    print(jr.report_line("jpeg", tag, r))
    assert r["ok"] and r["worst"] <= jr.BOUND, (tag, r["failed"])


@pytest.mark.parametrize("tag", ["random2_33x31_QA", "natural_33x31_q72.3", "random2_1x1_QB", "grey_8x8_17x15_QA"])
def test_c_abi_in_place_inside_a_nan_buffer(dev, tag):
    """ssg_diffjpeg with out == img, the B images in the middle of a NaN-filled buffer: everything before and after
    them stays NaN and the images are bit-equal to the out-of-place result."""
    from ssl_amd import _lib, engine
    x, quality = jc.case(tag)
    B, _, H, W = x.shape
    n, guard = x.size, 4099
    buf = torch.full((guard + n + guard,), float("nan"), device=dev)
    region = buf[guard:guard + n]
    region.copy_(T(x, dev).reshape(-1))
    qd = T(quality, dev) if np.ndim(quality) else None
    want = run(dev, x, quality)
    rc = _lib.lib().ssg_diffjpeg(engine._ptr(region), engine._ptr(region), B, H, W, engine._ptr(qd),
                                 0.0 if qd is not None else float(quality), engine._stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())
    assert torch.equal(region.view(B, 3, H, W), want)
    # (torch.equal is false for NaN: no NaN inside either)


def test_wrapper_layouts_dtypes_and_quality_tensor(dev):
    """Non-contiguous and half-precision x give the result of the contiguous fp32 copy (the half result cast back);
    the quality tensor is read, in whatever layout or dtype, and left unmodified; numel != B is refused."""
    from ssl_amd import datapath
    jp = datapath.DiffJPEG()
    x, quality = jc.case("random2_33x31_QA")
    B = x.shape[0]
    xg, q = T(x, dev), T(quality, dev)
    want = jp(xg, q)
    assert torch.equal(q.cpu(), torch.as_tensor(np.array(quality)))                     # (not overwritten with the factors)
    # strided view of a larger tensor, and a channels-last permutation
    big = torch.full((B, 3, 2 * 33 + 1, 2 * 31 + 3), 0.5, device=dev)
    big[:, :, 1::2, 2:2 + 2 * 31:2] = xg
    view = big[:, :, 1::2, 2:2 + 2 * 31:2]
    assert not view.is_contiguous() and torch.equal(view, xg)
    assert torch.equal(jp(view, q), want)
    nhwc = xg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not nhwc.is_contiguous() and torch.equal(jp(nhwc, q), want)
    assert torch.equal(view, xg) and torch.equal(big[:, :, 0], torch.full_like(big[:, :, 0], 0.5))   # inputs untouched
    # half and bfloat16: computed on the fp32 copy, cast back
    for dt in (torch.float16, torch.bfloat16):
        xh = xg.to(dt)
        yh = jp(xh, q)
        assert yh.dtype == dt and torch.equal(yh, jp(xh.float(), q).to(dt))
    # the quality tensor: every second element of a longer one, float64, on the CPU
    q2 = torch.stack([q, torch.full_like(q, 7.0)], 1).reshape(-1)[::2]
    assert not q2.is_contiguous() and torch.equal(jp(xg, q2), want)
    assert torch.equal(jp(xg, q.double()), want) and torch.equal(jp(xg, q.cpu()), want)
    assert torch.equal(q.cpu(), torch.as_tensor(np.array(quality)))
    for bad in (q[:-1], torch.cat([q, q[:1]]), q[:1]):
        with pytest.raises(ValueError):
            jp(xg, bad)
    # a scalar as int and as float
    assert torch.equal(jp(xg, 30), jp(xg, 30.0))


def test_two_runs_are_bit_equal(dev):
    for tag in ("natural_45x83_QA", "grey_mb_32x48_q50"):
        x, quality = jc.case(tag)
        a, b = run(dev, x, quality), run(dev, x, quality)
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())
